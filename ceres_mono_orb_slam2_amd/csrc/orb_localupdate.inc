// orb_localupdate.inc -- Tracking::UpdateLocalMap (src/Tracking.cc:838-977) in one call: UpdateLocalKeyFrames (:874-977: the frame's
// map points vote for keyframes, the voted set is extended through the covisibility graph and the spanning tree) and UpdateLocalPoints
// (:847-872: the first-occurrence union of the local keyframes' map points), followed by the gather of what SearchLocalPoints
// (:793-826) fixes from that state, so that the result is orbt_track_local_map's input as it stands.  Textually included by
// orb_track.hip.  Integers and copies only: every output is exact.
//
// The two places where the reference's result depends on pointer order (std::map<KeyFrame*, int> keyframeCounter, std::set<KeyFrame*>
// GetChilds()) are INPUTS here: kf_rank[] is the position of a keyframe in the caller's map order, the child lists come in the
// caller's set order.
//
// Seven launches on one stream, no workgroup waits for another:
//   k_ulm_init     first[] = none, held[] = votes[] = mark[] = 0, order[] = -1 (the workspace is CLEARED per call, no epochs).
//   k_ulm_marks    one lane per frame slot: a slot whose point is bad is cleared (frame_pt_out), every other held point is marked
//                  `held` and adds one vote to each observer (integer atomicAdd: order-free, so deterministic); one lane per seen_pt
//                  entry: held; one lane per keyframe: order[kf_rank[k]] = k.
//   k_ulm_kflist   ONE workgroup: a block scan in rank order emits the voted keyframes that are not bad, a block arg-max picks the
//                  lowest rank among the maxima (= the first strictly greater count, :913), then wave 0 runs the sequential walk of
//                  :924-971 (a ballot finds the first free neighbour / child), then the block scans the slot counts of the list.
//   k_ulm_first    one lane per (list position, slot), ordinal = the position's slot prefix + the slot: atomicMin into first[point].
//   k_ulm_count    the lanes with first[point] == ordinal, counted per tile.
//   k_ulm_scatter  every tile sums the counts of the tiles before it (a read of finished data, not a wait) and scatters in order.
//   k_ulm_gather   the packed mp_* / slot_* arrays with 16-byte stores, the mp_state padding up to cap_pt.
namespace orbhip {

#define ULM_B 256                 /* k_ulm_marks: frame slots per workgroup */
#define ULM_T 256                 /* compaction tile: ordinals per workgroup of k_ulm_first / k_ulm_count / k_ulm_scatter */
#define ULM_KWG 1024              /* k_ulm_kflist: one workgroup */
#define ULM_MAX_LOCAL 80          /* (:928) */
#define ULM_NONE 0x7FFFFFFF
#define ULM_ST_OFFSETS 1u         /* *status bits of the device form */
#define ULM_ST_INDEX 2u
#define ULM_ST_CAP_KF 4u
#define ULM_ST_CAP_PT 8u
#define ULM_ST_SLOTS 16u

struct UlmArgs {
  int n_kp, n_seen, n_prev, npts, nobs, nkf, ncov, nchild, nslots, max_slots, cap_kf, cap_pt;
  int host_n_list, host_total;                                      // >= 0: the points stage alone over positions 0..host_n_list-1
  const int32_t *frame_pt, *seen_pt, *prev_kf;
  const uint8_t* pt_bad; const int32_t *pt_nobs, *obs_off, *obs_kf;
  const double *pt_Xw, *pt_normal; const float *pt_min, *pt_max; const uint8_t* pt_desc;
  const uint8_t* kf_bad; const int32_t *kf_rank, *kf_parent, *cov_off, *cov_kf, *child_off, *child_kf, *slot_off, *slot_pt;
  int32_t *frame_pt_out, *local_kf, *local_pt, *counts, *votes_out;
  double *mp_Xw, *mp_normal; float *mp_min, *mp_max; uint8_t *mp_desc, *mp_state; double* slot_Xw; uint8_t* slot_state;
  uint32_t* status;
  // workspace: votes | mark | order | list [nkf], pos_off [nkf + 1], first | held [npts], blk [tiles], dyn [2] = {list length, slots of the list}
  int32_t *votes, *mark, *order, *list, *pos_off, *first, *held, *blk, *dyn;
};

__device__ __forceinline__ void ulm_flag(const UlmArgs& a, uint32_t bits) { if (a.status) atomicOr(a.status, bits); }

// [off[i], off[i + 1]) when it lies in [0, total] and ascends; an empty range and a status bit otherwise
__device__ __forceinline__ void ulm_range(const UlmArgs& a, const int32_t* off, int i, int total, int* lo, int* hi) {
  const int l = off[i], h = off[i + 1];
  const bool ok = l >= 0 && l <= h && h <= total;
  if (!ok) ulm_flag(a, ULM_ST_OFFSETS);
  *lo = ok ? l : 0; *hi = ok ? h : 0;
}

// the frame's slot f after the clearing of :888-890: the point id, or -1
__device__ __forceinline__ int ulm_frame_point(const UlmArgs& a, int f) {
  const int p = a.frame_pt[f];
  return (p < 0 || p >= a.npts || a.pt_bad[p]) ? -1 : p;
}

__global__ __launch_bounds__(256) void k_ulm_init(UlmArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.npts) { a.first[i] = ULM_NONE; a.held[i] = 0; }
  if (i < a.nkf) { a.votes[i] = 0; a.mark[i] = 0; a.order[i] = -1; }
  if (i == 0 && a.status) *a.status = 0u;
}

__global__ __launch_bounds__(ULM_B) void k_ulm_marks(UlmArgs a, int do_votes) {
  const int i = blockIdx.x * ULM_B + threadIdx.x;
  if (do_votes && i < a.nkf) {
    const int r = a.kf_rank ? a.kf_rank[i] : i;
    if (r < 0 || r >= a.nkf || atomicCAS(&a.order[r], -1, i) != -1) ulm_flag(a, ULM_ST_INDEX);      // (not a permutation)
  }
  if (i < a.n_seen) {
    const int p = a.seen_pt[i];
    if (p < 0 || p >= a.npts) ulm_flag(a, ULM_ST_INDEX);
    else a.held[p] = 1;
  }
  if (i < a.n_kp) {
    const int p = a.frame_pt[i];
    int out = -1;
    if (p < -1 || p >= a.npts) ulm_flag(a, ULM_ST_INDEX);
    else if (p >= 0 && !a.pt_bad[p]) {                              // (:880; a bad point's slot is cleared, :889)
      out = p;
      a.held[p] = 1;
      if (do_votes) {
        int lo, hi;
        ulm_range(a, a.obs_off, p, a.nobs, &lo, &hi);
        for (int e = lo; e < hi; e++) {                             // (:883-887)
          const int k = a.obs_kf[e];
          if (k < 0 || k >= a.nkf) ulm_flag(a, ULM_ST_INDEX);
          else atomicAdd(&a.votes[k], 1);
        }
      }
    }
    if (a.frame_pt_out) a.frame_pt_out[i] = out;
  }
  if (i == 0 && a.host_n_list >= 0) { a.dyn[0] = a.host_n_list; a.dyn[1] = a.host_total; }
}

// exclusive prefix of `v` over the workgroup (ULM_KWG lanes) and the workgroup's total; s_w: one int per wave
__device__ __forceinline__ int ulm_block_scan(int v, int* s_w, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int inc = v;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const int t = __shfl_up(inc, m); if (lane >= m) inc += t; }
  __syncthreads();                                                  // (s_w may still be read from the round before)
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int j = 0; j < ULM_KWG / 64; j++) { const int c = s_w[j]; if (j < w) before += c; all += c; }
  *total = all;
  return before + inc - v;
}

// the first entry of row kf of a keyframe CSR that is not bad and not marked (:935-947, :950-961), or -1; the whole wave calls it
__device__ __forceinline__ int ulm_first_free(const UlmArgs& a, const int32_t* off, const int32_t* arr, int total, int kf, int lane) {
  int lo, hi;
  ulm_range(a, off, kf, total, &lo, &hi);
  for (int e0 = lo; e0 < hi; e0 += 64) {
    const int e = e0 + lane;
    int c = -1; bool ok = false;
    if (e < hi) {
      c = arr[e];
      if (c < 0 || c >= a.nkf) ulm_flag(a, ULM_ST_INDEX);
      else ok = !a.kf_bad[c] && !*(volatile int32_t*)(a.mark + c);
    }
    const unsigned long long m = __ballot(ok);
    if (m) return __shfl(c, __ffsll(m) - 1);
  }
  return -1;
}

__global__ __launch_bounds__(ULM_KWG) void k_ulm_kflist(UlmArgs a) {
  __shared__ int s_w[ULM_KWG / 64];
  __shared__ long long s_key[ULM_KWG / 64];
  __shared__ int s_any[ULM_KWG / 64];
  __shared__ int s_n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // the voted keyframes that are not bad, in rank order (:906-920); key = (count, lowest rank first)
  int base = 0, any = 0;
  long long key = -1;
  for (int r0 = 0; r0 < a.nkf; r0 += ULM_KWG) {
    const int r = r0 + tid;
    const int k = r < a.nkf ? a.order[r] : -1;
    const int v = k >= 0 ? a.votes[k] : 0;
    any |= v > 0;
    const bool emit = v > 0 && !a.kf_bad[k];
    int chunk;
    const int at = base + ulm_block_scan(emit ? 1 : 0, s_w, &chunk);
    if (emit) {
      a.list[at] = k; a.mark[k] = 1;
      const long long mine = ((long long)v << 32) | (long long)(ULM_NONE - r);
      key = mine > key ? mine : key;
    }
    base += chunk;
  }
  if (a.votes_out) for (int k = tid; k < a.nkf; k += ULM_KWG) a.votes_out[k] = a.votes[k];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const long long o = __shfl_xor(key, m); key = o > key ? o : key;
    any |= __shfl_xor(any, m);
  }
  __syncthreads();
  if (lane == 0) { s_key[w] = key; s_any[w] = any; }
  __syncthreads();
  key = -1; any = 0;
  for (int j = 0; j < ULM_KWG / 64; j++) { key = s_key[j] > key ? s_key[j] : key; any |= s_any[j]; }
  int n = base;
  if (!any) {                                                       // (:894-896) nobody got a vote: the previous list stays
    n = a.n_prev;
    for (int i = tid; i < n; i += ULM_KWG) {
      int k = a.prev_kf[i];
      if (k < 0 || k >= a.nkf) { ulm_flag(a, ULM_ST_INDEX); k = -1; }
      a.list[i] = k;
    }
  } else if (w == 0) {                                              // (:924-971) sequential; the marks are re-read after every append
    __threadfence_block();
    const int n_voted = n;                                          // (:924-925: itEndKF is taken BEFORE the appends - the walk visits the voted keyframes only)
    for (int i = 0; i < n_voted; i++) {
      if (n > ULM_MAX_LOCAL) break;                                 // (:928)
      const int kf = a.list[i];
      int c = ulm_first_free(a, a.cov_off, a.cov_kf, a.ncov, kf, lane);
      if (c >= 0) { if (lane == 0) { a.list[n] = c; a.mark[c] = 1; } __threadfence_block(); n++; }
      c = ulm_first_free(a, a.child_off, a.child_kf, a.nchild, kf, lane);
      if (c >= 0) { if (lane == 0) { a.list[n] = c; a.mark[c] = 1; } __threadfence_block(); n++; }
      const int par = a.kf_parent[kf];
      if (par < -1 || par >= a.nkf) { ulm_flag(a, ULM_ST_INDEX); continue; }
      if (par >= 0 && !*(volatile int32_t*)(a.mark + par)) {        // (:963-969: isBad() is not asked of the parent)
        if (lane == 0) { a.list[n] = par; a.mark[par] = 1; }
        __threadfence_block(); n++;
        break;                                                      // (:968)
      }
    }
    if (lane == 0) s_n = n;
  }
  __syncthreads();
  if (any) n = s_n;
  if (tid == 0) {
    a.counts[0] = n;
    a.counts[1] = (any && key >= 0) ? a.order[ULM_NONE - (int)(key & 0x7FFFFFFFll)] : -1;
    a.counts[3] = any ? 0 : 1;
    if (n > a.cap_kf) ulm_flag(a, ULM_ST_CAP_KF);
  }
  int n_list = n > a.cap_kf ? 0 : n;                                // (a list that does not fit: nothing of it is used)
  for (int i = tid; i < n_list; i += ULM_KWG) a.local_kf[i] = a.list[i];
  // the slot prefix of the list positions
  int sbase = 0;
  for (int i0 = 0; a.slot_off && i0 < n_list; i0 += ULM_KWG) {      // (no slot tables: the keyframes stage alone)
    const int i = i0 + tid;
    int cnt = 0;
    if (i < n_list) {
      const int k = a.list[i];
      if (k >= 0) { int lo, hi; ulm_range(a, a.slot_off, k, a.nslots, &lo, &hi); cnt = hi - lo; }
    }
    int chunk;
    const int ex = ulm_block_scan(cnt, s_w, &chunk);
    if (i < n_list) a.pos_off[i] = sbase + ex;
    sbase += chunk;
    if (sbase > a.max_slots) break;                                 // (uniform: sbase is the same in every lane)
  }
  if (tid == 0) {
    if (sbase > a.max_slots) { ulm_flag(a, ULM_ST_SLOTS); n_list = 0; sbase = 0; }
    a.pos_off[n_list] = sbase;
    a.dyn[0] = n_list; a.dyn[1] = sbase;
  }
}

// the point (not bad, in range) that ordinal o of the list's slots names, or -1
__device__ __forceinline__ int ulm_slot_point(const UlmArgs& a, int o) {
  const int n_list = a.dyn[0];
  if (o >= a.dyn[1]) return -1;
  int b = 0, t = n_list;                                            // the last position whose prefix is <= o
  while (b < t) { const int m = (b + t) >> 1; if (a.pos_off[m] <= o) b = m + 1; else t = m; }
  const int pos = b - 1;
  int s = o;                                                        // (the points stage alone: positions ARE the rows of slot_off)
  if (a.host_n_list < 0) {
    const int k = a.list[pos];
    if (k < 0) return -1;
    s = a.slot_off[k] + (o - a.pos_off[pos]);
  }
  if (s < 0 || s >= a.nslots) return -1;
  const int p = a.slot_pt[s];
  if (p < -1 || p >= a.npts) { ulm_flag(a, ULM_ST_INDEX); return -1; }
  return (p < 0 || a.pt_bad[p]) ? -1 : p;                           // (:860-866: bad points are never marked)
}

__global__ __launch_bounds__(ULM_T) void k_ulm_first(UlmArgs a) {
  const int o = blockIdx.x * ULM_T + threadIdx.x;
  const int p = ulm_slot_point(a, o);
  if (p >= 0) atomicMin(&a.first[p], o);
}

// exclusive prefix of `keep` inside the tile and the tile's count
__device__ __forceinline__ int ulm_tile_scan(bool keep, int* s_w, int* count) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int j = 0; j < ULM_T / 64; j++) { const int c = s_w[j]; if (j < w) before += c; all += c; }
  *count = all;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(ULM_T) void k_ulm_count(UlmArgs a) {
  __shared__ int s_w[ULM_T / 64];
  const int o = blockIdx.x * ULM_T + threadIdx.x;
  const int p = ulm_slot_point(a, o);
  int count;
  ulm_tile_scan(p >= 0 && a.first[p] == o, s_w, &count);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = count;
}

__global__ __launch_bounds__(ULM_T) void k_ulm_scatter(UlmArgs a) {
  __shared__ int s_w[ULM_T / 64];
  __shared__ int s_off[ULM_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int before = 0;                                                   // the kept lanes of the tiles before this one
  for (int b = tid; b < (int)blockIdx.x; b += ULM_T) before += a.blk[b];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) before += __shfl_xor(before, m);
  if (lane == 0) s_off[w] = before;
  __syncthreads();
  before = 0;
#pragma unroll
  for (int j = 0; j < ULM_T / 64; j++) before += s_off[j];
  const int o = blockIdx.x * ULM_T + tid;
  const int p = ulm_slot_point(a, o);
  const bool keep = p >= 0 && a.first[p] == o;
  int count;
  const int j = before + ulm_tile_scan(keep, s_w, &count);
  if (keep && j < a.cap_pt) a.local_pt[j] = p;
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    a.counts[2] = before + count;
    if (before + count > a.cap_pt) ulm_flag(a, ULM_ST_CAP_PT);
  }
}

// chunk c (two doubles, one 16-byte store) of out[3 n] = src[3 idx(j) + k], zeros where idx(j) < 0
template <class Idx>
__device__ __forceinline__ void ulm_gather_triples(double* out, const double* src, int n, int c, Idx idx) {
  const int d0 = 2 * c;
  if (d0 >= 3 * n) return;
  double v[2] = {0.0, 0.0};
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int d = d0 + h;
    if (d < 3 * n) { const int p = idx(d / 3); if (p >= 0) v[h] = src[3 * (size_t)p + d % 3]; }
  }
  if (d0 + 1 < 3 * n) *(double2*)(out + d0) = make_double2(v[0], v[1]);
  else out[d0] = v[0];
}

__global__ __launch_bounds__(256) void k_ulm_gather(UlmArgs a) {
  int i = blockIdx.x * 256 + threadIdx.x;
  int n = a.counts[2];
  if (n > a.cap_pt) n = 0;                                          // (a list that does not fit: every row is padding)
  const int cap = a.cap_pt, t_pt = (3 * cap + 1) / 2, t_kp = (3 * a.n_kp + 1) / 2;
  auto local = [&](int j) { return a.local_pt[j]; };
  auto slot = [&](int f) { return ulm_frame_point(a, f); };
  if (i < 2 * cap) {                                                // descriptors: two lanes of 16 bytes per point
    if ((i >> 1) < n) ((uint4*)a.mp_desc)[i] = ((const uint4*)a.pt_desc)[2 * (size_t)a.local_pt[i >> 1] + (i & 1)];
    return;
  }
  i -= 2 * cap;
  if (i < t_pt) { ulm_gather_triples(a.mp_Xw, a.pt_Xw, n, i, local); return; }
  i -= t_pt;
  if (i < t_pt) { ulm_gather_triples(a.mp_normal, a.pt_normal, n, i, local); return; }
  i -= t_pt;
  if (i < cap) {                                                    // distances, and the state of :816-819 (padding rows: 0)
    uint8_t st = 0;
    if (i < n) {
      const int p = a.local_pt[i];
      a.mp_min[i] = a.pt_min[p]; a.mp_max[i] = a.pt_max[p];
      st = a.held[p] ? 0 : (a.pt_nobs[p] > 0 ? 1 : 3);
    }
    a.mp_state[i] = st;
    return;
  }
  i -= cap;
  if (i < a.n_kp) {
    const int p = ulm_frame_point(a, i);
    a.slot_state[i] = p < 0 ? 0 : (a.pt_nobs[p] > 0 ? 1 : 3);
    return;
  }
  i -= a.n_kp;
  if (i < t_kp) ulm_gather_triples(a.slot_Xw, a.pt_Xw, a.n_kp, i, slot);
}

// workspace sections, each rounded up to 256 bytes
struct UlmWs { size_t votes, mark, order, list, pos_off, first, held, blk, dyn, total; };
static int ulm_tiles(int max_slots) { return std::max(1, (max_slots + ULM_T - 1) / ULM_T); }
static UlmWs ulm_workspace(int nkf, int npts, int max_slots) {
  UlmWs w; Carve ws;
  const size_t kfs = 4 * (size_t)nkf, pts = 4 * (size_t)npts;
  w.votes = ws.take(kfs); w.mark = ws.take(kfs); w.order = ws.take(kfs); w.list = ws.take(kfs); w.pos_off = ws.take(kfs + 4);
  w.first = ws.take(pts); w.held = ws.take(pts); w.blk = ws.take(4 * (size_t)ulm_tiles(max_slots)); w.dyn = ws.take(8);
  w.total = ws.total;
  return w;
}
static void ulm_bind(UlmArgs& A, void* workspace) {
  const UlmWs ws = ulm_workspace(A.nkf, A.npts, A.max_slots);
  uint8_t* wb = (uint8_t*)workspace;
  A.votes = (int32_t*)(wb + ws.votes); A.mark = (int32_t*)(wb + ws.mark); A.order = (int32_t*)(wb + ws.order); A.list = (int32_t*)(wb + ws.list);
  A.pos_off = (int32_t*)(wb + ws.pos_off); A.first = (int32_t*)(wb + ws.first); A.held = (int32_t*)(wb + ws.held); A.blk = (int32_t*)(wb + ws.blk);
  A.dyn = (int32_t*)(wb + ws.dyn);
}

// stages: 1 = UpdateLocalKeyFrames, 2 = UpdateLocalPoints (+ the gather when A.mp_state is given)
static int ulm_enqueue(const UlmArgs& A, int stages, hipStream_t st) {
  const int n_init = std::max(std::max(A.npts, A.nkf), 1);
  hipLaunchKernelGGL(k_ulm_init, dim3((n_init + 255) / 256), dim3(256), 0, st, A);
  const int n_marks = std::max(std::max(std::max(A.n_kp, A.n_seen), (stages & 1) ? A.nkf : 0), 1);
  hipLaunchKernelGGL(k_ulm_marks, dim3((n_marks + ULM_B - 1) / ULM_B), dim3(ULM_B), 0, st, A, stages & 1);
  if (stages & 1) hipLaunchKernelGGL(k_ulm_kflist, dim3(1), dim3(ULM_KWG), 0, st, A);
  if (stages & 2) {
    const dim3 tiles(ulm_tiles(A.max_slots)), wg(ULM_T);
    hipLaunchKernelGGL(k_ulm_first, tiles, wg, 0, st, A);
    hipLaunchKernelGGL(k_ulm_count, tiles, wg, 0, st, A);
    hipLaunchKernelGGL(k_ulm_scatter, tiles, wg, 0, st, A);
    if (A.mp_state) {
      const size_t lanes = 2 * (size_t)A.cap_pt + 2 * (size_t)((3 * A.cap_pt + 1) / 2) + (size_t)A.cap_pt + (size_t)A.n_kp + (size_t)((3 * A.n_kp + 1) / 2);
      hipLaunchKernelGGL(k_ulm_gather, dim3((unsigned)((std::max<size_t>(lanes, 1) + 255) / 256)), dim3(256), 0, st, A);
    }
  }
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

// host checks of one CSR of entry point E: the offsets (argcheck), every entry in [0, n_ids) or -1 where none_ok, rows of at most max_row
// entries (0 = any)
static int ulm_check_csr(const char* E, const char* off_name, const char* val_name, const int32_t* off, const int32_t* val, int rows, bool none_ok, int n_ids,
                         int max_row, int* total) {
  *total = 0;
  if (rows == 0) return 0;
  if (!off) { set_error("%s: %s is NULL", E, off_name); return ORBHIP_EINVAL; }
  ORBHIP_ARG(check_csr(E, off_name, off, rows, total));
  for (int r = 0; max_row && r < rows; r++)
    if (off[r + 1] - off[r] > max_row) { set_error("%s: more than %d entries in row %d of %s", E, max_row, r, off_name); return ORBHIP_EINVAL; }
  if (*total && !val) { set_error("%s: %s is NULL", E, val_name); return ORBHIP_EINVAL; }
  ORBHIP_ARG(check_index(E, val_name, val, *total, n_ids, none_ok));
  return 0;
}

static bool ulm_packed_all_or_none(const void* const* q, int n, bool* all) {
  int have = 0;
  for (int i = 0; i < n; i++) have += q[i] != nullptr;
  *all = have == n;
  return have == 0 || have == n;
}

}  // namespace orbhip

extern "C" {

int orbt_update_local_map_workspace(int nkf, int npts, int max_local_slots, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && npts >= 0 && max_local_slots >= 0 && bytes, ORBHIP_EINVAL, "orbt_update_local_map_workspace: bad argument");
  *bytes = orbhip::ulm_workspace(nkf, npts, max_local_slots).total;
  return 0;
}

int orbt_update_local_map_device(int n_kp, const int32_t* frame_pt, int n_seen, const int32_t* seen_pt, int n_prev, const int32_t* prev_local_kf, int npts,
                                 const uint8_t* pt_bad, const int32_t* pt_nobs, int nobs, const int32_t* obs_off, const int32_t* obs_kf, const double* pt_Xw,
                                 const double* pt_normal, const float* pt_min_dist, const float* pt_max_dist, const uint8_t* pt_desc, int nkf, const uint8_t* kf_bad,
                                 const int32_t* kf_rank, const int32_t* kf_parent, int ncov, const int32_t* cov_off, const int32_t* cov_kf, int nchild,
                                 const int32_t* child_off, const int32_t* child_kf, int nslots, const int32_t* kf_slot_off, const int32_t* kf_slot_pt,
                                 int max_local_slots, int cap_kf, int cap_pt, int32_t* frame_pt_out, int32_t* local_kf, int32_t* local_pt, int32_t* counts,
                                 int32_t* votes, double* mp_Xw, double* mp_normal, float* mp_min_dist, float* mp_max_dist, uint8_t* mp_desc, uint8_t* mp_state,
                                 double* slot_Xw, uint8_t* slot_state, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(n_kp >= 0 && n_seen >= 0 && n_prev >= 0 && npts >= 0 && nobs >= 0 && nkf >= 0 && ncov >= 0 && nchild >= 0 && nslots >= 0 && max_local_slots >= 0 &&
                 cap_kf >= 0 && cap_pt >= 0, ORBHIP_EINVAL, "orbt_update_local_map_device: negative count");
  ORBHIP_REQUIRE(n_prev <= nkf, ORBHIP_EINVAL, "orbt_update_local_map_device: more previous local keyframes than keyframes");
  ORBHIP_REQUIRE(workspace && counts, ORBHIP_EINVAL, "orbt_update_local_map_device: NULL workspace or counts");
  ORBHIP_REQUIRE((n_kp == 0 || frame_pt) && (n_seen == 0 || seen_pt) && (n_prev == 0 || prev_local_kf), ORBHIP_EINVAL, "orbt_update_local_map_device: NULL frame argument");
  ORBHIP_REQUIRE(npts == 0 || (pt_bad && obs_off), ORBHIP_EINVAL, "orbt_update_local_map_device: NULL point argument");
  ORBHIP_REQUIRE(nobs == 0 || (npts > 0 && obs_kf), ORBHIP_EINVAL, "orbt_update_local_map_device: NULL obs_kf");
  ORBHIP_REQUIRE(nkf == 0 || (kf_bad && kf_parent && cov_off && child_off && kf_slot_off), ORBHIP_EINVAL, "orbt_update_local_map_device: NULL keyframe argument");
  ORBHIP_REQUIRE((ncov == 0 || cov_kf) && (nchild == 0 || child_kf) && (nslots == 0 || kf_slot_pt), ORBHIP_EINVAL, "orbt_update_local_map_device: NULL CSR entries");
  ORBHIP_REQUIRE((cap_kf == 0 || local_kf) && (cap_pt == 0 || local_pt), ORBHIP_EINVAL, "orbt_update_local_map_device: NULL list output");
  const void* packed[] = {mp_Xw, mp_normal, mp_min_dist, mp_max_dist, mp_desc, mp_state, slot_Xw, slot_state};
  bool all = false;
  ORBHIP_REQUIRE(ulm_packed_all_or_none(packed, 8, &all), ORBHIP_EINVAL, "orbt_update_local_map_device: the packed outputs are given all or none");
  ORBHIP_REQUIRE(!all || npts == 0 || (pt_nobs && pt_Xw && pt_normal && pt_min_dist && pt_max_dist && pt_desc), ORBHIP_EINVAL,
                 "orbt_update_local_map_device: NULL point record argument");
  const void* words[] = {frame_pt, seen_pt, prev_local_kf, pt_nobs, obs_off, obs_kf, pt_min_dist, pt_max_dist, kf_rank, kf_parent, cov_off, cov_kf, child_off, child_kf,
                         kf_slot_off, kf_slot_pt, frame_pt_out, local_kf, local_pt, counts, votes, mp_min_dist, mp_max_dist, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbt_update_local_map_device: 32-bit arrays must be 4-byte aligned");
  const void* quads[] = {pt_Xw, pt_normal, pt_desc, mp_Xw, mp_normal, mp_desc, slot_Xw, workspace};
  for (const void* q : quads) ORBHIP_REQUIRE((uintptr_t)q % 16 == 0, ORBHIP_EINVAL, "orbt_update_local_map_device: records and workspace must be 16-byte aligned");
  UlmArgs A; std::memset(&A, 0, sizeof(A));
  A.n_kp = n_kp; A.n_seen = n_seen; A.n_prev = n_prev; A.npts = npts; A.nobs = nobs; A.nkf = nkf; A.ncov = ncov; A.nchild = nchild; A.nslots = nslots;
  A.max_slots = max_local_slots; A.cap_kf = cap_kf; A.cap_pt = cap_pt; A.host_n_list = -1; A.host_total = -1;
  A.frame_pt = frame_pt; A.seen_pt = seen_pt; A.prev_kf = prev_local_kf; A.pt_bad = pt_bad; A.pt_nobs = pt_nobs; A.obs_off = obs_off; A.obs_kf = obs_kf;
  A.pt_Xw = pt_Xw; A.pt_normal = pt_normal; A.pt_min = pt_min_dist; A.pt_max = pt_max_dist; A.pt_desc = pt_desc;
  A.kf_bad = kf_bad; A.kf_rank = kf_rank; A.kf_parent = kf_parent; A.cov_off = cov_off; A.cov_kf = cov_kf; A.child_off = child_off; A.child_kf = child_kf;
  A.slot_off = kf_slot_off; A.slot_pt = kf_slot_pt;
  A.frame_pt_out = frame_pt_out; A.local_kf = local_kf; A.local_pt = local_pt; A.counts = counts; A.votes_out = votes;
  A.mp_Xw = mp_Xw; A.mp_normal = mp_normal; A.mp_min = mp_min_dist; A.mp_max = mp_max_dist; A.mp_desc = mp_desc; A.mp_state = mp_state;
  A.slot_Xw = slot_Xw; A.slot_state = slot_state; A.status = status;
  ulm_bind(A, workspace);
  return ulm_enqueue(A, 3, (hipStream_t)stream);
}

int orbt_update_local_keyframes(int n_kp, const int32_t* frame_pt, int npts, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, int nkf,
                                const uint8_t* kf_bad, const int32_t* kf_rank, const int32_t* kf_parent, const int32_t* cov_off, const int32_t* cov_kf,
                                const int32_t* child_off, const int32_t* child_kf, int n_prev, const int32_t* prev_local_kf, int cap_kf, int32_t* frame_pt_out,
                                int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf, int32_t* status, int32_t* votes) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(n_kp >= 0 && npts >= 0 && nkf >= 0 && n_prev >= 0 && cap_kf >= 0, ORBHIP_EINVAL, "orbt_update_local_keyframes: negative count");
  ORBHIP_REQUIRE(n_prev <= nkf, ORBHIP_EINVAL, "orbt_update_local_keyframes: more previous local keyframes than keyframes");
  ORBHIP_REQUIRE(n_local_kf && ref_kf && status && (cap_kf == 0 || local_kf), ORBHIP_EINVAL, "orbt_update_local_keyframes: NULL output");
  ORBHIP_REQUIRE(n_kp == 0 || (frame_pt && frame_pt_out), ORBHIP_EINVAL, "orbt_update_local_keyframes: NULL frame argument");
  ORBHIP_REQUIRE(npts == 0 || pt_bad, ORBHIP_EINVAL, "orbt_update_local_keyframes: NULL pt_bad");
  ORBHIP_REQUIRE(nkf == 0 || (kf_bad && kf_parent), ORBHIP_EINVAL, "orbt_update_local_keyframes: NULL keyframe argument");
  ORBHIP_REQUIRE(n_prev == 0 || prev_local_kf, ORBHIP_EINVAL, "orbt_update_local_keyframes: NULL prev_local_kf");
  static const char E[] = "orbt_update_local_keyframes";
  int nobs = 0, ncov = 0, nchild = 0, rc = 0;
  if ((rc = ulm_check_csr(E, "obs_off", "obs_kf", obs_off, obs_kf, npts, false, nkf, 0, &nobs)) ||
      (rc = ulm_check_csr(E, "cov_off", "cov_kf", cov_off, cov_kf, nkf, false, nkf, 10, &ncov)) ||
      (rc = ulm_check_csr(E, "child_off", "child_kf", child_off, child_kf, nkf, false, nkf, 0, &nchild))) return rc;
  ORBHIP_ARG(check_index(E, "frame_pt", frame_pt, n_kp, npts, true));
  ORBHIP_ARG(check_index(E, "prev_local_kf", prev_local_kf, n_prev, nkf));
  ORBHIP_ARG(check_index(E, "kf_parent", kf_parent, nkf, nkf, true));
  if (kf_rank) ORBHIP_ARG(check_permutation(E, "kf_rank", kf_rank, nkf));
  ThreadWs& W = thread_ws();
  if ((rc = W.begin())) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts;
  RoundTrip R(W);
  const HostIn<int32_t> d_frame = R.in(frame_pt, (size_t)n_kp), d_prev = R.in(prev_local_kf, (size_t)n_prev), d_rank = R.in(kf_rank, nk), d_parent = R.in(kf_parent, nk);
  const HostIn<int32_t> d_obs_off = R.csr(obs_off, np), d_cov_off = R.csr(cov_off, nk), d_child_off = R.csr(child_off, nk);
  const HostIn<int32_t> d_obs_kf = R.in(obs_kf, (size_t)nobs), d_cov_kf = R.in(cov_kf, (size_t)ncov), d_child_kf = R.in(child_kf, (size_t)nchild);
  const HostIn<uint8_t> d_pt_bad = R.in(pt_bad, np), d_kf_bad = R.in(kf_bad, nk);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4), o_frame = R.out<int32_t>((size_t)n_kp), o_local = R.out<int32_t>((size_t)cap_kf), o_votes = R.out<int32_t>(nk, votes != nullptr);
  R.scratch(std::max<size_t>(ulm_workspace(nkf, npts, 0).total, 256));
  if ((rc = R.commit())) return rc;
  UlmArgs A; std::memset(&A, 0, sizeof(A));
  A.n_kp = n_kp; A.n_prev = n_prev; A.npts = npts; A.nobs = nobs; A.nkf = nkf; A.ncov = ncov; A.nchild = nchild; A.cap_kf = cap_kf; A.host_n_list = -1; A.host_total = -1;
  A.frame_pt = d_frame.dev(); A.prev_kf = d_prev.dev(); A.pt_bad = d_pt_bad.dev(); A.obs_off = d_obs_off.dev(); A.obs_kf = d_obs_kf.dev();
  A.kf_bad = d_kf_bad.dev(); A.kf_rank = d_rank.dev(); A.kf_parent = d_parent.dev(); A.cov_off = d_cov_off.dev(); A.cov_kf = d_cov_kf.dev();
  A.child_off = d_child_off.dev(); A.child_kf = d_child_kf.dev();
  A.frame_pt_out = o_frame.dev(); A.local_kf = o_local.dev(); A.counts = o_counts.dev(); A.votes_out = o_votes.dev();
  ulm_bind(A, R.scratch_dev());
  if ((rc = ulm_enqueue(A, 1, R.stream())) || (rc = R.finish())) return rc;
  *n_local_kf = o_counts[0];
  ORBHIP_REQUIRE(o_counts[0] <= cap_kf, ORBHIP_ECAP, "orbt_update_local_keyframes: more local keyframes than cap_kf");
  *ref_kf = o_counts[1]; *status = o_counts[3];
  R.copy_out(o_frame, frame_pt_out, (size_t)n_kp); R.copy_out(o_local, local_kf, (size_t)o_counts[0]); R.copy_out(o_votes, votes, nk);
  return 0;
}

int orbt_update_local_points(int n_local_kf, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const uint8_t* pt_bad, const int32_t* pt_nobs,
                             const double* pt_Xw, const double* pt_normal, const float* pt_min_dist, const float* pt_max_dist, const uint8_t* pt_desc, int n_kp,
                             const int32_t* frame_pt, int n_seen, const int32_t* seen_pt, int cap_pt, int32_t* local_pt, int32_t* n_local_pt, double* mp_Xw,
                             double* mp_normal, float* mp_min_dist, float* mp_max_dist, uint8_t* mp_desc, uint8_t* mp_state, double* slot_Xw, uint8_t* slot_state) {
  using namespace orbhip;
  ORBHIP_REQUIRE(n_local_kf >= 0 && npts >= 0 && n_kp >= 0 && n_seen >= 0 && cap_pt >= 0, ORBHIP_EINVAL, "orbt_update_local_points: negative count");
  ORBHIP_REQUIRE(n_local_pt && (cap_pt == 0 || local_pt), ORBHIP_EINVAL, "orbt_update_local_points: NULL output");
  ORBHIP_REQUIRE(npts == 0 || pt_bad, ORBHIP_EINVAL, "orbt_update_local_points: NULL pt_bad");
  ORBHIP_REQUIRE((n_kp == 0 || frame_pt) && (n_seen == 0 || seen_pt), ORBHIP_EINVAL, "orbt_update_local_points: NULL frame argument");
  const void* packed[] = {mp_Xw, mp_normal, mp_min_dist, mp_max_dist, mp_desc, mp_state, slot_Xw, slot_state};
  bool all = false;
  ORBHIP_REQUIRE(ulm_packed_all_or_none(packed, 8, &all), ORBHIP_EINVAL, "orbt_update_local_points: the packed outputs are given all or none");
  ORBHIP_REQUIRE(!all || npts == 0 || (pt_nobs && pt_Xw && pt_normal && pt_min_dist && pt_max_dist && pt_desc), ORBHIP_EINVAL, "orbt_update_local_points: NULL point record argument");
  static const char E[] = "orbt_update_local_points";
  int nslots = 0, rc = 0;
  if ((rc = ulm_check_csr(E, "kf_slot_off", "kf_slot_pt", kf_slot_off, kf_slot_pt, n_local_kf, true, npts, 0, &nslots))) return rc;
  ORBHIP_ARG(check_index(E, "frame_pt", frame_pt, n_kp, npts, true));
  ORBHIP_ARG(check_index(E, "seen_pt", seen_pt, n_seen, npts));
  ThreadWs& W = thread_ws();
  if ((rc = W.begin())) return rc;
  const size_t np = (size_t)npts, cap = (size_t)cap_pt, nf = (size_t)n_kp;
  RoundTrip R(W);
  const HostIn<int32_t> d_slot_off = R.csr(kf_slot_off, (size_t)n_local_kf), d_slot_pt = R.in(kf_slot_pt, (size_t)nslots);
  const HostIn<int32_t> d_frame = R.in(frame_pt, nf), d_seen = R.in(seen_pt, (size_t)n_seen), d_nobs = R.in(all ? pt_nobs : nullptr, np);
  const HostIn<uint8_t> d_bad = R.in(pt_bad, np), d_desc = R.in(all ? pt_desc : nullptr, 32 * np);
  const HostIn<double> d_Xw = R.in(all ? pt_Xw : nullptr, 3 * np), d_normal = R.in(all ? pt_normal : nullptr, 3 * np);
  const HostIn<float> d_min = R.in(all ? pt_min_dist : nullptr, np), d_max = R.in(all ? pt_max_dist : nullptr, np);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4), o_local = R.out<int32_t>(cap);
  const HostOut<double> o_Xw = R.out<double>(3 * cap, all), o_normal = R.out<double>(3 * cap, all), o_slot_Xw = R.out<double>(3 * nf, all);
  const HostOut<float> o_min = R.out<float>(cap, all), o_max = R.out<float>(cap, all);
  const HostOut<uint8_t> o_desc = R.out<uint8_t>(32 * cap, all), o_state = R.out<uint8_t>(cap, all), o_slot_state = R.out<uint8_t>(nf, all);
  R.scratch(std::max<size_t>(ulm_workspace(0, npts, nslots).total, 256));
  if ((rc = R.commit())) return rc;
  UlmArgs A; std::memset(&A, 0, sizeof(A));
  A.n_kp = n_kp; A.n_seen = n_seen; A.npts = npts; A.nslots = nslots; A.max_slots = nslots; A.cap_pt = cap_pt; A.host_n_list = n_local_kf; A.host_total = nslots;
  A.frame_pt = d_frame.dev(); A.seen_pt = d_seen.dev(); A.pt_bad = d_bad.dev(); A.pt_nobs = d_nobs.dev();
  A.pt_Xw = d_Xw.dev(); A.pt_normal = d_normal.dev(); A.pt_min = d_min.dev(); A.pt_max = d_max.dev(); A.pt_desc = d_desc.dev();
  A.slot_off = d_slot_off.dev(); A.slot_pt = d_slot_pt.dev();
  A.local_pt = o_local.dev(); A.counts = o_counts.dev();
  A.mp_Xw = o_Xw.dev(); A.mp_normal = o_normal.dev(); A.mp_min = o_min.dev(); A.mp_max = o_max.dev(); A.mp_desc = o_desc.dev();
  A.mp_state = o_state.dev(); A.slot_Xw = o_slot_Xw.dev(); A.slot_state = o_slot_state.dev();
  ulm_bind(A, R.scratch_dev());
  A.pos_off = const_cast<int32_t*>(A.slot_off);                     // (positions are the rows: the slot prefix IS the CSR; the points stage only reads it)
  if ((rc = ulm_enqueue(A, 2, R.stream())) || (rc = R.finish())) return rc;
  const int n = o_counts[2];
  *n_local_pt = n;
  ORBHIP_REQUIRE(n <= cap_pt, ORBHIP_ECAP, "orbt_update_local_points: more local map points than cap_pt");
  // the lists up to n: what lies behind them in the caller's arrays is not touched (mp_state is padded up to cap_pt by the gather)
  const size_t nn = (size_t)n;
  R.copy_out(o_local, local_pt, nn);
  R.copy_out(o_Xw, mp_Xw, 3 * nn); R.copy_out(o_normal, mp_normal, 3 * nn); R.copy_out(o_min, mp_min_dist, nn); R.copy_out(o_max, mp_max_dist, nn);
  R.copy_out(o_desc, mp_desc, 32 * nn); R.copy_out(o_state, mp_state, cap); R.copy_out(o_slot_Xw, slot_Xw, 3 * nf); R.copy_out(o_slot_state, slot_state, nf);
  return 0;
}

}  // extern "C"
