// orb_updateconn.inc -- KeyFrame::UpdateConnections (src/KeyFrame.cc:314-398) with AddConnection / UpdateBestCovisibles (:158-193) for a
// whole list of keyframes in one call (orbl_update_connections*), and the new loop links LoopClosing::CorrectLoop derives while it
// walks that list (src/LoopClosing.cc:551-573).  Textually included by orb_localmap.hip.
//
// The reference's loop is sequential: target A's AddConnection re-sorts the ordered list of every neighbour it reaches, and a later
// target overwrites what earlier ones sent to it.  The kernels use the closed form of that loop (DESIGN.md section 2, "UpdateConnections"),
// in which nothing waits for an earlier keyframe:
//   cnt[t][k]        votes of target t for keyframe k: inputs only.
//   send(t -> B)     defined when cnt[t] is not empty and cnt[t][B] >= th, or no entry of cnt[t] reaches th and B = kmax(t).
//   base(B)          cnt[tB] when B is target tB with a non-empty counter ("own"), else B's input row.  With an own base only the sends
//                    of targets AFTER tB apply, otherwise all do.  A send is effective iff base.get(A) != cnt[t][B].
//   final map of B   base overwritten by the applicable sends (an ineffective one rewrites the value it finds).
//   final list of B  every entry of the final map by descending (weight, rank) if a send was effective, else B's own step-4 list.
// All integer.  Six launches on one stream after the workspace is cleared; no workgroup waits for another:
//   k_uc_init     one lane per target / keyframe / point: the checks of the device form, tpos[k] = the target that names keyframe k.
//   k_uc_votes    one lane per slot: cnt[t][k]++ by integer atomicAdd (order-free, hence deterministic); one lane per entry of the input
//                 tables: inpos[B][t] = where B's input row names the keyframe of target t.
//   k_uc_summary  one workgroup per target: size of the counter, entries >= th, kmax (lowest rank among the maxima), the front of the
//                 step-4 list (highest rank among the maxima); tgt_status / tgt_parent.
//   k_uc_count    one workgroup per keyframe: affected?, any effective send?, sizes of its final map and list; one workgroup per
//                 target: the candidates of its links.
//   k_uc_scan     ONE workgroup: exclusive scans over the keyframes and the targets, the wanted counts, the capacity bits.
//   k_uc_emit     one workgroup per affected keyframe: gathers its final entries, then places each by COUNTING - the keys
//                 (weight << 32) | rank are unique inside a row, so an entry's position is the number of greater keys (lesser ranks for
//                 the map's own order): exact, no comparison network, rows of any length tiled through LDS; one workgroup per target
//                 for its links in rank order.
// Outputs are written with vector stores only, each element by the one lane that owns it; nothing is written beyond a capacity.
#include "orb_maptable.h"

namespace orbhip {

#define UC_WG 256                 /* every kernel but the scan; also the sort tile */
#define UC_SWG 1024               /* k_uc_scan: one workgroup */
#define UC_ST_OFFSETS 1u          /* *status bits of the device form */
#define UC_ST_INDEX 2u
#define UC_ST_CAP_AFF 4u
#define UC_ST_CAP_CONN 8u
#define UC_ST_CAP_ORD 16u
#define UC_ST_CAP_LINK 32u

struct UcArgs {
  int ntgt, nslots, nkf, npts, nobs, nconn, nprev, th, cap_aff, cap_conn, cap_ord, cap_link;
  const int32_t* tgt_kf; const uint8_t* tgt_flags; const int32_t* slot_off; const int32_t* slot_pt; const int32_t* obs_off; const int32_t* obs_kf;
  const uint8_t* pt_bad; const int32_t* kf_rank; const int32_t* conn_off; const int32_t* conn_kf; const int32_t* conn_w; const int32_t* prev_off;
  const int32_t* prev_kf;
  int32_t *tgt_status, *tgt_parent, *aff_kf, *oconn_off, *oconn_kf, *oconn_w, *oord_off, *oord_kf, *oord_w, *link_off, *link_kf, *counts;
  uint32_t* status;
  // workspace: cnt[ntgt][nkf] | inpos[nkf][ntgt] | pmark[ntgt][nkf] (bytes) | rhit[nkf] (cleared per call), tpos[nkf] (set to -1 per call),
  // per target t_nkeys | t_npairs | t_kmax | t_front | t_nlink | t_loff, per keyframe k_aff | k_eff | k_nmap | k_nord | k_aidx | k_coff | k_ooff,
  // the gathered entries ent_kf | ent_key [ent_cap] and the link candidates lnk[ntgt][nkf]
  int32_t *cnt, *inpos, *rhit, *tpos, *t_nkeys, *t_npairs, *t_kmax, *t_front, *t_nlink, *t_loff;
  int32_t *k_aff, *k_eff, *k_nmap, *k_nord, *k_aidx, *k_coff, *k_ooff, *ent_kf, *lnk;
  uint8_t* pmark; long long* ent_key; size_t ent_cap;
};

// the row of CSR `off` (rows of them, `total` entries) that holds entry s, or -1
__device__ __forceinline__ int uc_row_of(const int32_t* off, int rows, int total, int s) {
  int b = 0, t = rows;
  while (b < t) { const int m = (b + t) >> 1; if (off[m] <= s) b = m + 1; else t = m; }
  const int c = b - 1;
  int lo, hi;
  if (c < 0 || !mt_range(off, c, total, &lo, &hi) || s < lo || s >= hi) return -1;
  return c;
}

__device__ __forceinline__ uint32_t uc_rank(const UcArgs& a, int k) { return (uint32_t)(a.kf_rank ? a.kf_rank[k] : k); }
__device__ __forceinline__ bool uc_kf_ok(const UcArgs& a, int k) { return k >= 0 && k < a.nkf; }
// target t names a keyframe in range and is the one instance of it that counts
__device__ __forceinline__ bool uc_tgt_ok(const UcArgs& a, int t) { const int k = a.tgt_kf[t]; return uc_kf_ok(a, k) && a.tpos[k] == t; }
__device__ __forceinline__ int32_t& uc_cnt(const UcArgs& a, int t, int k) { return a.cnt[(size_t)t * a.nkf + k]; }

__device__ __forceinline__ unsigned long long uc_shfl_xor64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

// sum over the workgroup (UC_WG lanes), the same value in every lane; s: UC_WG / 64 words of LDS, reusable at once
__device__ __forceinline__ int uc_block_sum(int v, int* s) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int i = 0; i < UC_WG / 64; i++) r += s[i];
  return r;
}

__device__ __forceinline__ unsigned long long uc_block_max(unsigned long long v, unsigned long long* s) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const unsigned long long o = uc_shfl_xor64(v, m); v = o > v ? o : v; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long r = 0;
#pragma unroll
  for (int i = 0; i < UC_WG / 64; i++) r = s[i] > r ? s[i] : r;
  return r;
}

__global__ __launch_bounds__(UC_WG) void k_uc_init(UcArgs a) {
  const int i = blockIdx.x * UC_WG + threadIdx.x;
  int lo, hi;
  if (i < a.ntgt) {
    if (!mt_range(a.slot_off, i, a.nslots, &lo, &hi)) mt_flag(a.status, UC_ST_OFFSETS);
    if (a.prev_off && !mt_range(a.prev_off, i, a.nprev, &lo, &hi)) mt_flag(a.status, UC_ST_OFFSETS);
    const int k = a.tgt_kf[i];
    if (!uc_kf_ok(a, k)) mt_flag(a.status, UC_ST_INDEX);
    else if (atomicMax(&a.tpos[k], i) != -1) mt_flag(a.status, UC_ST_INDEX);         // (a keyframe listed twice: its last instance counts)
  }
  if (i < a.nkf) {
    if (!mt_range(a.conn_off, i, a.nconn, &lo, &hi)) mt_flag(a.status, UC_ST_OFFSETS);
    if (a.kf_rank) {
      const int r = a.kf_rank[i];
      if (r < 0 || r >= a.nkf) mt_flag(a.status, UC_ST_INDEX);
      else if (atomicAdd(&a.rhit[r], 1) != 0) mt_flag(a.status, UC_ST_INDEX);        // (not a permutation)
    }
  }
  if (i < a.npts && !mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, UC_ST_OFFSETS);
}

__global__ __launch_bounds__(UC_WG) void k_uc_votes(UcArgs a) {
  const int i = blockIdx.x * UC_WG + threadIdx.x;
  if (i < a.nslots) {                                               // (:326-343)
    const int t = uc_row_of(a.slot_off, a.ntgt, a.nslots, i);
    if (t >= 0 && uc_tgt_ok(a, t)) {
      const int A = a.tgt_kf[t], p = a.slot_pt[i];
      if (p < -1 || p >= a.npts) mt_flag(a.status, UC_ST_INDEX);
      else if (p >= 0 && !(a.pt_bad && a.pt_bad[p])) {
        int lo, hi;
        mt_range(a.obs_off, p, a.nobs, &lo, &hi);
        for (int e = lo; e < hi; e++) {
          const int k = a.obs_kf[e];
          if (!uc_kf_ok(a, k)) { mt_flag(a.status, UC_ST_INDEX); continue; }
          if (k != A) atomicAdd(&uc_cnt(a, t, k), 1);
        }
      }
    }
  }
  if (i < a.nconn) {
    const int B = uc_row_of(a.conn_off, a.nkf, a.nconn, i);
    if (B >= 0) {
      const int k = a.conn_kf[i];
      if (!uc_kf_ok(a, k) || k == B) mt_flag(a.status, UC_ST_INDEX);
      else if (a.tpos[k] >= 0) a.inpos[(size_t)B * a.ntgt + a.tpos[k]] = i + 1;
    }
  }
}

__global__ __launch_bounds__(UC_WG) void k_uc_summary(UcArgs a) {
  __shared__ int s_sum[UC_WG / 64];
  __shared__ unsigned long long s_max[UC_WG / 64];
  __shared__ int s_kf[2];
  const int t = blockIdx.x, tid = threadIdx.x;
  int nkeys = 0, npairs = 0, kf_lo = -1, kf_hi = -1;
  unsigned long long key_lo = 0, key_hi = 0;                         // (a count is >= 1, so a key of an entry is never 0)
  if (uc_tgt_ok(a, t))
    for (int k = tid; k < a.nkf; k += UC_WG) {
      const int c = uc_cnt(a, t, k);
      if (c <= 0) continue;
      nkeys++; npairs += c >= a.th;
      const uint32_t r = uc_rank(a, k);
      const unsigned long long lo = ((unsigned long long)(uint32_t)c << 32) | (0xFFFFFFFFu - r), hi = ((unsigned long long)(uint32_t)c << 32) | r;
      if (lo > key_lo) { key_lo = lo; kf_lo = k; }                   // (:360 `>`: the first of the maxima in map order)
      if (hi > key_hi) { key_hi = hi; kf_hi = k; }                   // (the front of the descending (weight, pointer) list)
    }
  nkeys = uc_block_sum(nkeys, s_sum);
  npairs = uc_block_sum(npairs, s_sum);
  const unsigned long long best_lo = uc_block_max(key_lo, s_max), best_hi = uc_block_max(key_hi, s_max);
  if (nkeys > 0 && key_lo == best_lo) s_kf[0] = kf_lo;
  if (nkeys > 0 && key_hi == best_hi) s_kf[1] = kf_hi;
  __syncthreads();
  if (tid == 0) {
    const int kmax = nkeys > 0 ? s_kf[0] : -1, front = nkeys > 0 ? (npairs > 0 ? s_kf[1] : kmax) : -1;
    a.t_nkeys[t] = nkeys; a.t_npairs[t] = npairs; a.t_kmax[t] = kmax; a.t_front[t] = front;
    a.tgt_status[t] = nkeys > 0 ? 0 : 1;                             // (:346)
    a.tgt_parent[t] = (nkeys > 0 && a.tgt_flags && (a.tgt_flags[t] & 1)) ? front : -1;      // (:392-396)
  }
}

// is AddConnection(B <- keyframe of target t, cnt[t][B]) part of target t's turn (:364-373)
__device__ __forceinline__ bool uc_send(const UcArgs& a, int t, int B) {
  if (a.t_nkeys[t] <= 0) return false;
  return uc_cnt(a, t, B) >= a.th || (a.t_npairs[t] == 0 && a.t_kmax[t] == B);
}

// where B's input row names the keyframe of target t: the entry index, or -1
__device__ __forceinline__ int uc_input_entry(const UcArgs& a, int B, int lo, int hi, int t) {
  const int e = a.inpos[(size_t)B * a.ntgt + t] - 1;
  return e >= lo && e < hi ? e : -1;
}

struct UcRow { int tB, lo, hi; bool own; };
__device__ __forceinline__ UcRow uc_row(const UcArgs& a, int B) {
  UcRow R;
  R.tB = a.tpos[B];
  R.own = R.tB >= 0 && a.t_nkeys[R.tB] > 0;
  mt_range(a.conn_off, B, a.nconn, &R.lo, &R.hi);
  return R;
}

__device__ __forceinline__ void uc_push(const UcArgs& a, int* s_n, size_t base, int k, int w) {
  const size_t at = base + (size_t)atomicAdd(s_n, 1);
  if (at < a.ent_cap) { a.ent_kf[at] = k; a.ent_key[at] = (long long)(((unsigned long long)(uint32_t)w << 32) | uc_rank(a, k)); }
}

// This lane's share of keyframe B's final map: *nent entries, *eff = a send that changed something.  EMIT: the entries are pushed too.
template <bool EMIT>
__device__ __forceinline__ void uc_kf_walk(const UcArgs& a, int B, const UcRow& R, int tid, int* nent, int* eff, int* s_n, size_t base) {
  for (int t = tid; t < a.ntgt; t += UC_WG) {                        // the sends, as far as they name a keyframe the base does not hold
    if ((R.own && t <= R.tB) || !uc_send(a, t, B)) continue;
    const int A = a.tgt_kf[t], w = uc_cnt(a, t, B);
    bool present; int b = 0;
    if (R.own) { b = uc_cnt(a, R.tB, A); present = b > 0; }
    else { const int e = uc_input_entry(a, B, R.lo, R.hi, t); present = e >= 0; if (present) b = a.conn_w[e]; }
    if (present) { *eff |= b != w; continue; }
    *eff = 1; *nent += 1;
    if (EMIT) uc_push(a, s_n, base, A, w);
  }
  if (R.own) {                                                      // the base, a held entry taking the weight of a send that applies to it
    for (int k = tid; k < a.nkf; k += UC_WG) {
      const int c = uc_cnt(a, R.tB, k);
      if (c <= 0) continue;
      *nent += 1;
      if (EMIT) { const int t = a.tpos[k]; uc_push(a, s_n, base, k, t > R.tB && uc_send(a, t, B) ? uc_cnt(a, t, B) : c); }
    }
  } else {
    for (int e = R.lo + tid; e < R.hi; e += UC_WG) {
      const int k = a.conn_kf[e];
      if (!uc_kf_ok(a, k) || k == B) continue;
      *nent += 1;
      if (EMIT) { const int t = a.tpos[k]; uc_push(a, s_n, base, k, t >= 0 && uc_send(a, t, B) ? uc_cnt(a, t, B) : a.conn_w[e]); }
    }
  }
}

// K(A) \ P(A) \ targets of target t into lnk[t][..] (LoopClosing.cc:556-572); returns the number kept
__device__ __forceinline__ void uc_link_candidates(const UcArgs& a, int t, int tid, int* s_sum, int* s_n) {
  if (!uc_tgt_ok(a, t)) { if (tid == 0) a.t_nlink[t] = 0; return; }
  const int A = a.tgt_kf[t];
  int lo, hi, plo, phi;
  mt_range(a.conn_off, A, a.nconn, &lo, &hi);
  mt_range(a.prev_off, t, a.nprev, &plo, &phi);
  // was A's list re-sorted before its turn: an effective send of an earlier target, judged against A's input row
  int pre = 0;
  for (int u = tid; u < t; u += UC_WG) {
    if (!uc_send(a, u, A)) continue;
    const int e = uc_input_entry(a, A, lo, hi, u);
    pre |= e < 0 || a.conn_w[e] != uc_cnt(a, u, A);
  }
  pre = uc_block_sum(pre, s_sum);
  uint8_t* mark = a.pmark + (size_t)t * a.nkf;
  if (pre)                                                          // P(A) = every key of the row (the senders are targets, dropped below)
    for (int e = lo + tid; e < hi; e += UC_WG) { const int k = a.conn_kf[e]; if (uc_kf_ok(a, k)) mark[k] = 1; }
  for (int e = plo + tid; e < phi; e += UC_WG) {                    // (the previous list is checked even where the re-sorted row replaces it)
    const int k = a.prev_kf[e];
    if (!uc_kf_ok(a, k)) mt_flag(a.status, UC_ST_INDEX);
    else if (!pre) mark[k] = 1;
  }
  if (tid == 0) *s_n = 0;
  __syncthreads();
  int32_t* out = a.lnk + (size_t)t * a.nkf;
  if (a.t_nkeys[t] > 0) {
    for (int k = tid; k < a.nkf; k += UC_WG)
      if (uc_cnt(a, t, k) > 0 && a.tpos[k] < 0 && !mark[k]) { const int at = atomicAdd(s_n, 1); if (at < a.nkf) out[at] = k; }
  } else {
    for (int e = lo + tid; e < hi; e += UC_WG) {
      const int k = a.conn_kf[e];
      if (uc_kf_ok(a, k) && k != A && a.tpos[k] < 0 && !mark[k]) { const int at = atomicAdd(s_n, 1); if (at < a.nkf) out[at] = k; }
    }
  }
  __syncthreads();
  if (tid == 0) a.t_nlink[t] = min(*s_n, a.nkf);
}

__global__ __launch_bounds__(UC_WG) void k_uc_count(UcArgs a) {
  __shared__ int s_sum[UC_WG / 64];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.nkf) { uc_link_candidates(a, blockIdx.x - a.nkf, tid, s_sum, &s_n); return; }
  const int B = blockIdx.x;
  const UcRow R = uc_row(a, B);
  int nent = 0, eff = 0;
  uc_kf_walk<false>(a, B, R, tid, &nent, &eff, nullptr, 0);
  nent = uc_block_sum(nent, s_sum);
  eff = uc_block_sum(eff, s_sum) != 0;
  if (tid == 0) {
    const int aff = R.own || eff;
    a.k_aff[B] = aff; a.k_eff[B] = eff;
    a.k_nmap[B] = aff ? nent : 0;
    a.k_nord[B] = !aff ? 0 : eff ? nent : max(a.t_npairs[R.tB], 1);   // (:370-373: the maximum alone when nothing reaches th)
  }
}

// out[i] = in[0] + ... + in[i - 1] over n entries by the whole workgroup; returns the total.  s: UC_SWG words of LDS.
__device__ __forceinline__ int uc_scan(const int32_t* in, int32_t* out, int n, int* s) {
  const int tid = threadIdx.x, per = (n + UC_SWG - 1) / UC_SWG;
  const int b = min(n, tid * per), e = min(n, b + per);
  int sum = 0;
  for (int i = b; i < e; i++) sum += in[i];
  __syncthreads();
  s[tid] = sum;
  __syncthreads();
  for (int d = 1; d < UC_SWG; d <<= 1) {
    const int v = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int run = s[tid] - sum;
  const int total = s[UC_SWG - 1];
  for (int i = b; i < e; i++) { const int v = in[i]; out[i] = run; run += v; }
  return total;
}

__global__ __launch_bounds__(UC_SWG) void k_uc_scan(UcArgs a) {
  __shared__ int s[UC_SWG];
  const int n_aff = uc_scan(a.k_aff, a.k_aidx, a.nkf, s), n_conn = uc_scan(a.k_nmap, a.k_coff, a.nkf, s), n_ord = uc_scan(a.k_nord, a.k_ooff, a.nkf, s);
  const int n_link = a.link_off ? uc_scan(a.t_nlink, a.t_loff, a.ntgt, s) : 0;
  __syncthreads();
  if (a.link_off)
    for (int t = threadIdx.x; t <= a.ntgt; t += UC_SWG) a.link_off[t] = t < a.ntgt ? a.t_loff[t] : n_link;
  if (threadIdx.x == 0) {
    a.counts[0] = n_aff; a.counts[1] = n_conn; a.counts[2] = n_ord; a.counts[3] = n_link;
    if (n_aff <= a.cap_aff) { a.oconn_off[n_aff] = n_conn; a.oord_off[n_aff] = n_ord; }      // (the offset arrays hold cap_aff + 1 entries)
    const uint32_t bits = (n_aff > a.cap_aff ? UC_ST_CAP_AFF : 0u) | (n_conn > a.cap_conn ? UC_ST_CAP_CONN : 0u) | (n_ord > a.cap_ord ? UC_ST_CAP_ORD : 0u) |
                          (n_link > a.cap_link ? UC_ST_CAP_LINK : 0u);
    if (bits) mt_flag(a.status, bits);
  }
}

__global__ __launch_bounds__(UC_WG) void k_uc_emit(UcArgs a) {
  __shared__ long long s_key[UC_WG];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= a.nkf) {                                   // the links of one target, in ascending rank (the order of std::set)
    const int t = blockIdx.x - a.nkf, n = a.t_nlink[t], off = a.t_loff[t];
    const int32_t* in = a.lnk + (size_t)t * a.nkf;
    uint32_t* s_rank = (uint32_t*)s_key;
    for (int ib = 0; ib < n; ib += UC_WG) {
      const int i = ib + tid;
      const int k = i < n ? in[i] : 0;
      const uint32_t r = i < n ? uc_rank(a, k) : 0u;
      int pos = 0;
      for (int jb = 0; jb < n; jb += UC_WG) {
        __syncthreads();
        if (jb + tid < n) s_rank[tid] = uc_rank(a, in[jb + tid]);
        __syncthreads();
        const int m = min(UC_WG, n - jb);
        for (int j = 0; j < m; j++) pos += s_rank[j] < r;
      }
      if (i < n && pos < n && off + pos < a.cap_link) a.link_kf[off + pos] = k;
    }
    return;
  }
  const int B = blockIdx.x;
  if (!a.k_aff[B]) return;
  const UcRow R = uc_row(a, B);
  const int aidx = a.k_aidx[B], coff = a.k_coff[B], ooff = a.k_ooff[B], nord = a.k_nord[B];
  const size_t base = (size_t)coff;
  const int n = (int)min((size_t)a.k_nmap[B], base < a.ent_cap ? a.ent_cap - base : (size_t)0);
  if (tid == 0) {
    s_n = 0;
    if (aidx < a.cap_aff) { a.aff_kf[aidx] = B; a.oconn_off[aidx] = coff; a.oord_off[aidx] = ooff; }
  }
  __syncthreads();
  int nent = 0, eff = 0;
  uc_kf_walk<true>(a, B, R, tid, &nent, &eff, &s_n, base);
  __syncthreads();                                                  // (the entries are read back by this workgroup only)
  // without an effective send the list is the target's own: the entries >= th, which are the first nord of the full order, or - when
  // nothing reaches th - kmax alone, which is the LOWEST rank among the maxima while the full order starts with the highest
  const bool kmax_only = !a.k_eff[B] && a.t_npairs[R.tB] == 0;
  const int kmax = kmax_only ? a.t_kmax[R.tB] : -1;
  for (int ib = 0; ib < n; ib += UC_WG) {
    const int i = ib + tid;
    const long long key = i < n ? a.ent_key[base + i] : 0;
    const uint32_t r = (uint32_t)key;
    int below = 0, above = 0;
    for (int jb = 0; jb < n; jb += UC_WG) {
      __syncthreads();
      if (jb + tid < n) s_key[tid] = a.ent_key[base + jb + tid];
      __syncthreads();
      const int m = min(UC_WG, n - jb);
      for (int j = 0; j < m; j++) { const long long kj = s_key[j]; below += (uint32_t)kj < r; above += kj > key; }
    }
    if (i >= n) continue;
    const int k = a.ent_kf[base + i], w = (int)(key >> 32);
    if (below < n && coff + below < a.cap_conn) { a.oconn_kf[coff + below] = k; a.oconn_w[coff + below] = w; }
    const int at = kmax_only ? (k == kmax ? 0 : nord) : above;
    if (at < nord && ooff + at < a.cap_ord) { a.oord_kf[ooff + at] = k; a.oord_w[ooff + at] = w; }
  }
}

// workspace sections, each rounded up to 256 bytes; [0, cleared) is zeroed and tpos set to -1 by every call
struct UcWs { size_t cnt, inpos, pmark, rhit, cleared, tpos, tgt, kfs, ent_kf, ent_key, lnk, ent_cap, total; };
static UcWs uc_workspace(int ntgt, int nkf, int nconn) {
  UcWs w; Carve ws;
  const size_t cells = (size_t)ntgt * (size_t)nkf;
  w.cnt = ws.take(4 * cells); w.inpos = ws.take(4 * cells); w.pmark = ws.take(cells); w.rhit = ws.take(4 * (size_t)nkf);
  w.cleared = ws.total;
  w.tpos = ws.take(4 * (size_t)nkf);
  w.tgt = ws.take(6 * 4 * (size_t)ntgt); w.kfs = ws.take(7 * 4 * (size_t)nkf);
  // a final map is a counter (at most nkf entries, ntgt of them) or an input row plus the sends that reach it (at most one per cell)
  w.ent_cap = (size_t)nconn + 2 * cells;
  w.ent_kf = ws.take(4 * w.ent_cap); w.ent_key = ws.take(8 * w.ent_cap); w.lnk = ws.take(4 * cells);
  w.total = ws.total > 0 ? ws.total : 256;
  return w;
}

}  // namespace orbhip

extern "C" {

int orbl_update_connections_workspace(int ntgt, int nkf, int npts, int nslots, int nconn, size_t* bytes) {
  ORBHIP_REQUIRE(ntgt >= 0 && nkf >= 0 && npts >= 0 && nslots >= 0 && nconn >= 0 && bytes, ORBHIP_EINVAL, "orbl_update_connections_workspace: bad argument");
  *bytes = orbhip::uc_workspace(ntgt, nkf, nconn).total;
  return 0;
}

int orbl_update_connections_device(int ntgt, const int32_t* tgt_kf, const uint8_t* tgt_flags, int nslots, const int32_t* slot_off, const int32_t* slot_pt, int nkf,
                                   int npts, int nobs, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* pt_bad, const int32_t* kf_rank, int nconn,
                                   const int32_t* conn_off, const int32_t* conn_kf, const int32_t* conn_w, int nprev, const int32_t* prev_off,
                                   const int32_t* prev_kf, int th, int cap_aff, int cap_conn, int cap_ord, int cap_link, int32_t* tgt_status, int32_t* tgt_parent,
                                   int32_t* aff_kf, int32_t* oconn_off, int32_t* oconn_kf, int32_t* oconn_w, int32_t* oord_off, int32_t* oord_kf, int32_t* oord_w,
                                   int32_t* link_off, int32_t* link_kf, int32_t* counts, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(ntgt >= 0 && nslots >= 0 && nkf >= 0 && npts >= 0 && nobs >= 0 && nconn >= 0 && nprev >= 0, ORBHIP_EINVAL, "orbl_update_connections: negative count");
  ORBHIP_REQUIRE(cap_aff >= 0 && cap_conn >= 0 && cap_ord >= 0 && cap_link >= 0, ORBHIP_EINVAL, "orbl_update_connections: negative capacity");
  ORBHIP_REQUIRE(th >= 1, ORBHIP_EINVAL, "orbl_update_connections: th must be >= 1");
  ORBHIP_REQUIRE(workspace && counts && oconn_off && oord_off, ORBHIP_EINVAL, "orbl_update_connections: NULL workspace, counts or offset output");
  ORBHIP_REQUIRE(ntgt == 0 || (tgt_kf && slot_off && tgt_status && tgt_parent), ORBHIP_EINVAL, "orbl_update_connections: NULL target argument");
  ORBHIP_REQUIRE(nslots == 0 || (ntgt > 0 && slot_pt), ORBHIP_EINVAL, "orbl_update_connections: NULL slot_pt");
  ORBHIP_REQUIRE(npts == 0 || obs_off, ORBHIP_EINVAL, "orbl_update_connections: NULL obs_off");
  ORBHIP_REQUIRE(nobs == 0 || (npts > 0 && obs_kf), ORBHIP_EINVAL, "orbl_update_connections: NULL obs_kf");
  ORBHIP_REQUIRE(nkf == 0 || conn_off, ORBHIP_EINVAL, "orbl_update_connections: NULL conn_off");
  ORBHIP_REQUIRE(nconn == 0 || (nkf > 0 && conn_kf && conn_w), ORBHIP_EINVAL, "orbl_update_connections: NULL table argument");
  ORBHIP_REQUIRE(nprev == 0 || (prev_off && prev_kf), ORBHIP_EINVAL, "orbl_update_connections: prev_off and prev_kf are given together");
  ORBHIP_REQUIRE(!prev_kf || prev_off, ORBHIP_EINVAL, "orbl_update_connections: prev_kf without prev_off");
  ORBHIP_REQUIRE(!link_off || prev_off, ORBHIP_EINVAL, "orbl_update_connections: the links need the previous ordered lists");
  ORBHIP_REQUIRE(link_off || !link_kf, ORBHIP_EINVAL, "orbl_update_connections: link_kf without link_off");
  ORBHIP_REQUIRE((cap_aff == 0 || aff_kf) && (cap_conn == 0 || (oconn_kf && oconn_w)) && (cap_ord == 0 || (oord_kf && oord_w)) && (!link_off || cap_link == 0 || link_kf),
                 ORBHIP_EINVAL, "orbl_update_connections: NULL list output");
  const void* words[] = {tgt_kf, slot_off, slot_pt, obs_off, obs_kf, kf_rank, conn_off, conn_kf, conn_w, prev_off, prev_kf, tgt_status, tgt_parent, aff_kf,
                         oconn_off, oconn_kf, oconn_w, oord_off, oord_kf, oord_w, link_off, link_kf, counts, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_update_connections: 32-bit arrays must be 4-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)workspace % 8 == 0, ORBHIP_EINVAL, "orbl_update_connections: workspace must be 8-byte aligned");
  const UcWs ws = uc_workspace(ntgt, nkf, nconn);
  uint8_t* wb = (uint8_t*)workspace;
  UcArgs A; std::memset(&A, 0, sizeof(A));
  A.ntgt = ntgt; A.nslots = nslots; A.nkf = nkf; A.npts = npts; A.nobs = nobs; A.nconn = nconn; A.nprev = nprev; A.th = th;
  A.cap_aff = cap_aff; A.cap_conn = cap_conn; A.cap_ord = cap_ord; A.cap_link = link_off ? cap_link : 0;
  A.tgt_kf = tgt_kf; A.tgt_flags = tgt_flags; A.slot_off = slot_off; A.slot_pt = slot_pt; A.obs_off = obs_off; A.obs_kf = obs_kf; A.pt_bad = pt_bad;
  A.kf_rank = kf_rank; A.conn_off = conn_off; A.conn_kf = conn_kf; A.conn_w = conn_w; A.prev_off = prev_off; A.prev_kf = prev_kf;
  A.tgt_status = tgt_status; A.tgt_parent = tgt_parent; A.aff_kf = aff_kf; A.oconn_off = oconn_off; A.oconn_kf = oconn_kf; A.oconn_w = oconn_w;
  A.oord_off = oord_off; A.oord_kf = oord_kf; A.oord_w = oord_w; A.link_off = link_off; A.link_kf = link_kf; A.counts = counts; A.status = status;
  A.cnt = (int32_t*)(wb + ws.cnt); A.inpos = (int32_t*)(wb + ws.inpos); A.pmark = wb + ws.pmark; A.rhit = (int32_t*)(wb + ws.rhit); A.tpos = (int32_t*)(wb + ws.tpos);
  int32_t* tg = (int32_t*)(wb + ws.tgt); int32_t* kq = (int32_t*)(wb + ws.kfs);
  A.t_nkeys = tg; A.t_npairs = tg + ntgt; A.t_kmax = tg + 2 * (size_t)ntgt; A.t_front = tg + 3 * (size_t)ntgt; A.t_nlink = tg + 4 * (size_t)ntgt; A.t_loff = tg + 5 * (size_t)ntgt;
  A.k_aff = kq; A.k_eff = kq + nkf; A.k_nmap = kq + 2 * (size_t)nkf; A.k_nord = kq + 3 * (size_t)nkf; A.k_aidx = kq + 4 * (size_t)nkf; A.k_coff = kq + 5 * (size_t)nkf;
  A.k_ooff = kq + 6 * (size_t)nkf;
  A.ent_kf = (int32_t*)(wb + ws.ent_kf); A.ent_key = (long long*)(wb + ws.ent_key); A.lnk = (int32_t*)(wb + ws.lnk); A.ent_cap = ws.ent_cap;
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  if (ws.cleared > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0, ws.cleared, st));
  if (nkf > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.tpos, 0xFF, 4 * (size_t)nkf, st));
  const int n_init = std::max(std::max(ntgt, nkf), npts), n_votes = std::max(nslots, nconn);
  const unsigned n_links = link_off ? (unsigned)ntgt : 0u;
  if (n_init > 0) hipLaunchKernelGGL(k_uc_init, dim3((n_init + UC_WG - 1) / UC_WG), dim3(UC_WG), 0, st, A);
  if (n_votes > 0) hipLaunchKernelGGL(k_uc_votes, dim3((n_votes + UC_WG - 1) / UC_WG), dim3(UC_WG), 0, st, A);
  if (ntgt > 0) hipLaunchKernelGGL(k_uc_summary, dim3(ntgt), dim3(UC_WG), 0, st, A);
  if (nkf + n_links > 0) hipLaunchKernelGGL(k_uc_count, dim3(nkf + n_links), dim3(UC_WG), 0, st, A);
  hipLaunchKernelGGL(k_uc_scan, dim3(1), dim3(UC_SWG), 0, st, A);
  if (nkf + n_links > 0) hipLaunchKernelGGL(k_uc_emit, dim3(nkf + n_links), dim3(UC_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_update_connections(int ntgt, const int32_t* tgt_kf, const uint8_t* tgt_flags, const int32_t* slot_off, const int32_t* slot_pt, int nkf, int npts,
                            const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* pt_bad, const int32_t* kf_rank, const int32_t* conn_off,
                            const int32_t* conn_kf, const int32_t* conn_w, const int32_t* prev_off, const int32_t* prev_kf, int th, int cap_aff, int cap_conn,
                            int cap_ord, int cap_link, int32_t* tgt_status, int32_t* tgt_parent, int32_t* aff_kf, int32_t* oconn_off, int32_t* oconn_kf,
                            int32_t* oconn_w, int32_t* oord_off, int32_t* oord_kf, int32_t* oord_w, int32_t* link_off, int32_t* link_kf, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(ntgt >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_update_connections: negative count");
  ORBHIP_REQUIRE(cap_aff >= 0 && cap_conn >= 0 && cap_ord >= 0 && cap_link >= 0, ORBHIP_EINVAL, "orbl_update_connections: negative capacity");
  ORBHIP_REQUIRE(th >= 1, ORBHIP_EINVAL, "orbl_update_connections: th must be >= 1");
  ORBHIP_REQUIRE(counts && oconn_off && oord_off, ORBHIP_EINVAL, "orbl_update_connections: NULL counts or offset output");
  ORBHIP_REQUIRE(ntgt == 0 || (tgt_kf && slot_off && tgt_status && tgt_parent), ORBHIP_EINVAL, "orbl_update_connections: NULL target argument");
  ORBHIP_REQUIRE(npts == 0 || obs_off, ORBHIP_EINVAL, "orbl_update_connections: NULL obs_off");
  ORBHIP_REQUIRE(nkf == 0 || conn_off, ORBHIP_EINVAL, "orbl_update_connections: NULL conn_off");
  ORBHIP_REQUIRE((prev_off != nullptr) == (prev_kf != nullptr), ORBHIP_EINVAL, "orbl_update_connections: prev_off and prev_kf are given together");
  ORBHIP_REQUIRE((!link_off && !link_kf) || prev_off, ORBHIP_EINVAL, "orbl_update_connections: the links need the previous ordered lists");
  ORBHIP_REQUIRE(link_off || !link_kf, ORBHIP_EINVAL, "orbl_update_connections: link_kf without link_off");
  ORBHIP_REQUIRE((cap_aff == 0 || aff_kf) && (cap_conn == 0 || (oconn_kf && oconn_w)) && (cap_ord == 0 || (oord_kf && oord_w)) && (!link_off || cap_link == 0 || link_kf),
                 ORBHIP_EINVAL, "orbl_update_connections: NULL list output");
  static const char E[] = "orbl_update_connections";
  int nslots = 0, nobs = 0, nconn = 0, nprev = 0;
  ORBHIP_ARG(check_csr(E, "slot_off", slot_off, ntgt, &nslots));
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_ARG(check_csr(E, "conn_off", conn_off, nkf, &nconn));
  ORBHIP_ARG(check_csr(E, "prev_off", prev_off, prev_off ? ntgt : 0, &nprev));
  ORBHIP_REQUIRE((nslots == 0 || slot_pt) && (nobs == 0 || obs_kf) && (nconn == 0 || (conn_kf && conn_w)), ORBHIP_EINVAL, "orbl_update_connections: NULL CSR entries");
  ORBHIP_ARG(check_listed_once(E, "tgt_kf", tgt_kf, ntgt, nkf));
  ORBHIP_ARG(check_index(E, "slot_pt", slot_pt, nslots, npts, true));
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  ORBHIP_ARG(check_index(E, "prev_kf", prev_kf, nprev, nkf));
  if (kf_rank) ORBHIP_ARG(check_permutation(E, "kf_rank", kf_rank, nkf));
  ORBHIP_ARG(check_index(E, "conn_kf", conn_kf, nconn, nkf));
  std::vector<int32_t> seen((size_t)nkf, -1);                       // (per ROW of the table: the last row that named the keyframe)
  for (int k = 0; k < nkf; k++)
    for (int e = conn_off[k]; e < conn_off[k + 1]; e++) {
      ORBHIP_REQUIRE(conn_kf[e] != k && seen[conn_kf[e]] != k, ORBHIP_EINVAL, "orbl_update_connections: a row of conn_kf names itself or a keyframe twice");
      seen[conn_kf[e]] = k;
    }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const bool links = link_off != nullptr;
  const size_t nt = (size_t)ntgt, nk = (size_t)nkf, np = (size_t)npts;
  RoundTrip R(W);
  const HostIn<int32_t> d_tgt = R.in(tgt_kf, nt), d_slot_off = R.csr(slot_off, nt), d_slot_pt = R.in(slot_pt, (size_t)nslots), d_rank = R.in(kf_rank, nk);
  const HostIn<int32_t> d_obs_off = R.csr(obs_off, np), d_obs_kf = R.in(obs_kf, (size_t)nobs), d_prev_off = R.csr(prev_off, nt), d_prev_kf = R.in(prev_kf, (size_t)nprev);
  const HostIn<int32_t> d_conn_off = R.csr(conn_off, nk), d_conn_kf = R.in(conn_kf, (size_t)nconn), d_conn_w = R.in(conn_w, (size_t)nconn);
  const HostIn<uint8_t> d_flags = R.in(tgt_flags, nt), d_bad = R.in(pt_bad, np);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4), o_tgt_status = R.out<int32_t>(nt), o_parent = R.out<int32_t>(nt), o_aff = R.out<int32_t>((size_t)cap_aff);
  const HostOut<int32_t> o_conn_off = R.out<int32_t>((size_t)cap_aff + 1), o_conn_kf = R.out<int32_t>((size_t)cap_conn), o_conn_w = R.out<int32_t>((size_t)cap_conn);
  const HostOut<int32_t> o_ord_off = R.out<int32_t>((size_t)cap_aff + 1), o_ord_kf = R.out<int32_t>((size_t)cap_ord), o_ord_w = R.out<int32_t>((size_t)cap_ord);
  const HostOut<int32_t> o_link_off = R.out<int32_t>(nt + 1, links), o_link_kf = R.out<int32_t>((size_t)cap_link, links);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(uc_workspace(ntgt, nkf, nconn).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_update_connections_device(ntgt, d_tgt.dev(), d_flags.dev(), nslots, d_slot_off.dev(), d_slot_pt.dev(), nkf, npts, nobs, d_obs_off.dev(), d_obs_kf.dev(),
                                           d_bad.dev(), d_rank.dev(), nconn, d_conn_off.dev(), d_conn_kf.dev(), d_conn_w.dev(), nprev, d_prev_off.dev(), d_prev_kf.dev(),
                                           th, cap_aff, cap_conn, cap_ord, links ? cap_link : 0, o_tgt_status.dev(), o_parent.dev(), o_aff.dev(), o_conn_off.dev(),
                                           o_conn_kf.dev(), o_conn_w.dev(), o_ord_off.dev(), o_ord_kf.dev(), o_ord_w.dev(), o_link_off.dev(), o_link_kf.dev(),
                                           o_counts.dev(), o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 4);
  const size_t n_aff = (size_t)o_counts[0], n_conn = (size_t)o_counts[1], n_ord = (size_t)o_counts[2], n_link = (size_t)o_counts[3];
  if (n_aff > (size_t)cap_aff || n_conn > (size_t)cap_conn || n_ord > (size_t)cap_ord || (links && n_link > (size_t)cap_link)) {
    set_error("orbl_update_connections: wanted %d affected keyframes, %d map entries, %d list entries, %d links; capacities %d, %d, %d, %d", o_counts[0], o_counts[1],
              o_counts[2], o_counts[3], cap_aff, cap_conn, cap_ord, links ? cap_link : 0);
    return ORBHIP_ECAP;
  }
  // the lists up to their counts: what lies behind them in the caller's arrays is not touched
  R.copy_out(o_tgt_status, tgt_status, nt); R.copy_out(o_parent, tgt_parent, nt); R.copy_out(o_aff, aff_kf, n_aff);
  R.copy_out(o_conn_off, oconn_off, n_aff + 1); R.copy_out(o_ord_off, oord_off, n_aff + 1);
  R.copy_out(o_conn_kf, oconn_kf, n_conn); R.copy_out(o_conn_w, oconn_w, n_conn); R.copy_out(o_ord_kf, oord_kf, n_ord); R.copy_out(o_ord_w, oord_w, n_ord);
  R.copy_out(o_link_off, link_off, nt + 1); R.copy_out(o_link_kf, link_kf, n_link);
  return 0;
}

}  // extern "C"
