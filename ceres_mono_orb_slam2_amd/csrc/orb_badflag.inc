// orb_badflag.inc -- KeyFrame::SetBadFlag (src/KeyFrame.cc:460-553) with EraseConnection (:560-573), UpdateBestCovisibles (:172-193) and
// MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:140-191) for a whole list of keyframes in one call (orbl_set_bad_keyframes*).
// Textually included by orb_localmap.hip.
//
// The reference's loop is sequential.  The kernels use its partly closed form (DESIGN.md section 2, "SetBadFlag on the tables"):
//   connections  entry (k -> B) of the input tables goes iff B is a status-0 target and B's input row names k ("mutual"); it goes at B's
//                turn.  A target's own row and list end empty.  k's list is ALL of what is left of its row by descending (weight, rank)
//                from the first turn that took an entry, and its input list before that.
//   points       a point changes only at the turns of the status-0 targets that hold it in a slot AND observe it, in target order: one
//                lane per point replays exactly those.
//   tree         only the spanning-tree repair needs the state the earlier targets left: ONE workgroup walks the targets in order.
// All integer except the one 3x4 product per target.  Seven launches on one stream after the workspace is cleared, whatever the data;
// no workgroup waits for another:
//   k_bf_init    one lane per target / keyframe / point: the offsets, the rank permutation, each target's tentative status, the FIRST
//                status-0 instance of every keyframe (integer atomicMax: order-free).
//   k_bf_mark    one lane per target: tgt_status, the zero rows of tgt_Tcp; per conn entry: its mutual target's turn and, per row, the
//                first turn that takes an entry (atomicMin); per child entry: is it there (in range, not the row itself, not a repeat);
//                per slot of a target: marks the observations of its point by that target.
//   k_bf_points  one lane per point: step 2 for the targets that hold and observe it, in target order.
//   k_bf_tree    ONE workgroup: steps 4 and 5 target after target.  Children rows are sets kept as the input entries plus an append-only
//                list of memberships, each with an alive byte; the argmax key is (weight, child rank ascending, list position ascending),
//                where the position inside a re-sorted list is its entry's rank descending.
//   k_bf_count   one workgroup per keyframe: the sizes of its three output rows.
//   k_bf_scan    ONE workgroup: the three offset arrays, counts[], the capacity bits.
//   k_bf_emit    one workgroup per keyframe: the conn row closed up in input order; the list copied, or placed by COUNTING - the keys
//                (weight << 32) | rank are unique inside a row, so an entry's position is the number of greater keys; the children
//                gathered and placed by the number of lesser ranks.  Rows of any length are tiled through LDS.
// Outputs are written with vector stores only, each element by the one lane that owns it; nothing is written beyond a capacity.
#include <climits>

#include "orb_maptable.h"

namespace orbhip {

#define BF_WG 256                 /* every kernel but the tree and the scan; also the sort tile */
#define BF_TWG 1024               /* k_bf_tree, k_bf_scan: one workgroup */
#define BF_ST_OFFSETS 1u          /* *status bits of the device form */
#define BF_ST_INDEX 2u
#define BF_ST_TARGET 4u
#define BF_ST_ROW 8u
#define BF_ST_CAP_ORD 16u
#define BF_ST_CAP_CHILD 32u
#define BF_NEVER 0x7F7F7F7F       /* k_first of a row no target takes an entry from (the byte the workspace is preset with) */

struct BfArgs {
  int ntgt, nkf, npts, nchild, nconn, nord, nslots, nobs, cap_ord, cap_child;
  const int32_t* tgt_kf; const uint8_t* tgt_flags; const uint8_t* tgt_mask;
  uint8_t* kf_bad; int32_t* kf_parent; const int32_t* kf_rank; const double* kf_Tcw;
  const int32_t *child_off, *child_kf, *conn_off, *conn_kf, *conn_w, *ord_off, *ord_kf, *ord_w;
  const int32_t* slot_off; int32_t* slot_pt; uint8_t* pt_bad; int32_t* pt_nobs; int32_t* pt_ref_kf;
  const int32_t *obs_off, *obs_kf, *obs_slot; uint8_t* obs_erased;
  int32_t* tgt_status; double* tgt_Tcp;
  int32_t *oconn_off, *oconn_kf, *oconn_w, *oord_off, *oord_kf, *oord_w, *ochild_off, *ochild_kf, *counts;
  uint32_t* status;
  // workspace.  Cleared per call: tfirst[nkf] (ntgt - t of the first status-0 target t naming the keyframe, 0 = none) | rhit[nkf] |
  // mark[nkf] | cand[nkf] | mut[nconn] (turn + 1 of the entry's mutual target) | n_add[1] | in_alive[nchild] | obs_mark[nobs].  Preset to
  // BF_NEVER: k_first[nkf].  Then t_st[ntgt], the memberships add_par | add_child | add_alive [add_cap], the children of the current
  // target chl | chl_src [nkf], the row sizes k_nconn | k_nord | k_nchild [nkf], the gathered children cg[nchild + add_cap].
  int32_t *tfirst, *rhit, *mark, *cand, *mut, *n_add, *k_first, *t_st, *add_par, *add_child, *chl, *chl_src, *k_nconn, *k_nord, *k_nchild, *cg;
  uint8_t *in_alive, *obs_mark, *add_alive;
  size_t add_cap;
};

// the row of CSR `off` (rows of them, `total` entries) that holds entry s, or -1
__device__ __forceinline__ int bf_row_of(const int32_t* off, int rows, int total, int s) {
  int b = 0, t = rows;
  while (b < t) { const int m = (b + t) >> 1; if (off[m] <= s) b = m + 1; else t = m; }
  const int c = b - 1;
  int lo, hi;
  if (c < 0 || !mt_range(off, c, total, &lo, &hi) || s < lo || s >= hi) return -1;
  return c;
}

__device__ __forceinline__ uint32_t bf_rank(const BfArgs& a, int k) { return (uint32_t)(a.kf_rank ? a.kf_rank[k] : k); }
__device__ __forceinline__ bool bf_kf_ok(const BfArgs& a, int k) { return k >= 0 && k < a.nkf; }
// the turn at which keyframe k goes bad in this call, or -1
__device__ __forceinline__ int bf_turn(const BfArgs& a, int k) { const int v = a.tfirst[k]; return v > 0 ? a.ntgt - v : -1; }
// steps 1 to 5 run for target t
__device__ __forceinline__ bool bf_active(const BfArgs& a, int t) { return a.t_st[t] == 0 && bf_turn(a, a.tgt_kf[t]) == t; }
// (weight, rank) as one signed key: unique inside a row
__device__ __forceinline__ long long bf_key(int w, uint32_t r) { return (long long)w * 4294967296LL + (long long)r; }

template <int WG>
__device__ __forceinline__ mt_u64 bf_block_max(mt_u64 v, mt_u64* s) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
    const mt_u64 o = ((mt_u64)hi << 32) | lo;
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  mt_u64 r = 0;
#pragma unroll
  for (int i = 0; i < WG / 64; i++) r = s[i] > r ? s[i] : r;
  return r;
}

template <int WG>
__device__ __forceinline__ int bf_block_sum(int v, int* s) {
  v = mt_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int i = 0; i < WG / 64; i++) r += s[i];
  return r;
}

__global__ __launch_bounds__(BF_WG) void k_bf_init(BfArgs a) {
  const int i = blockIdx.x * BF_WG + threadIdx.x;
  int lo, hi;
  if (i < a.ntgt) {
    const int B = a.tgt_kf[i];
    int st = (a.tgt_mask && !a.tgt_mask[i]) ? 3 : (a.tgt_flags && (a.tgt_flags[i] & 1)) ? 1 : (a.tgt_flags && (a.tgt_flags[i] & 2)) ? 2 : 0;
    if (!bf_kf_ok(a, B)) st = 4;
    else if (st == 0) {
      const int P = a.kf_parent[B];
      if (a.kf_bad[B] || !bf_kf_ok(a, P) || P == B) st = 4;         // (:490 dereferences the parent)
      else atomicMax(&a.tfirst[B], a.ntgt - i);
    }
    if (st == 4) mt_flag(a.status, BF_ST_TARGET);
    a.t_st[i] = st;
  }
  if (i < a.nkf) {
    bool ok = mt_range(a.child_off, i, a.nchild, &lo, &hi);
    ok &= mt_range(a.conn_off, i, a.nconn, &lo, &hi);
    ok &= mt_range(a.ord_off, i, a.nord, &lo, &hi);
    if (a.slot_off) ok &= mt_range(a.slot_off, i, a.nslots, &lo, &hi);
    if (!ok) mt_flag(a.status, BF_ST_OFFSETS);
    if (a.kf_rank) {
      const int r = a.kf_rank[i];
      if (r < 0 || r >= a.nkf) mt_flag(a.status, BF_ST_INDEX);
      else if (atomicAdd(&a.rhit[r], 1) != 0) mt_flag(a.status, BF_ST_INDEX);        // (not a permutation)
    }
  }
  if (a.slot_off && i < a.npts && !mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, BF_ST_OFFSETS);
}

__global__ __launch_bounds__(BF_WG) void k_bf_mark(BfArgs a) {
  const int i = blockIdx.x * BF_WG + threadIdx.x;
  int lo, hi;
  if (i < a.ntgt) {
    int st = a.t_st[i];
    if (st == 0 && !bf_active(a, i)) { st = 4; mt_flag(a.status, BF_ST_TARGET); }  // (a keyframe listed twice: its first status-0 instance counts)
    a.tgt_status[i] = st;
    if (st != 0)
      for (int q = 0; q < 12; q++) a.tgt_Tcp[12 * (size_t)i + q] = 0.0;
  }
  if (i < a.nconn) {                                                // (:471-476, EraseConnection :560-573)
    const int k = bf_row_of(a.conn_off, a.nkf, a.nconn, i);
    if (k >= 0) {
      const int B = a.conn_kf[i];
      if (!bf_kf_ok(a, B) || B == k) mt_flag(a.status, B == k ? BF_ST_ROW : BF_ST_INDEX);
      else {
        const int t = bf_turn(a, B);
        if (t >= 0) {
          mt_range(a.conn_off, B, a.nconn, &lo, &hi);
          bool mutual = false;
          for (int e = lo; e < hi; e++) mutual |= a.conn_kf[e] == k;
          if (mutual) { a.mut[i] = t + 1; atomicMin(&a.k_first[k], t); }
        }
      }
    }
  }
  if (i < a.nchild) {
    const int r = bf_row_of(a.child_off, a.nkf, a.nchild, i);
    if (r >= 0) {
      const int c = a.child_kf[i];
      bool there = bf_kf_ok(a, c);
      if (!there) mt_flag(a.status, BF_ST_INDEX);
      else {
        there = c != r;
        for (int e = a.child_off[r]; e < i; e++) there &= a.child_kf[e] != c;
        if (!there) mt_flag(a.status, BF_ST_ROW);
      }
      a.in_alive[i] = there;
    }
  }
  if (a.slot_off && i < a.nslots) {                                 // which observations step 2 can reach (:478-480)
    const int B = bf_row_of(a.slot_off, a.nkf, a.nslots, i);
    if (B >= 0 && bf_turn(a, B) >= 0) {
      const int p = a.slot_pt[i];
      if (p < -1 || p >= a.npts) mt_flag(a.status, BF_ST_INDEX);
      else if (p >= 0) {
        mt_range(a.obs_off, p, a.nobs, &lo, &hi);
        for (int e = lo; e < hi; e++)
          if (a.obs_kf[e] == B) a.obs_mark[e] = 1;
      }
    }
  }
}

// Step 2 for one point: the targets that hold it in a slot and observe it, in target order (MapPoint::EraseObservation, src/MapPoint.cc:140-162)
__global__ __launch_bounds__(BF_WG) void k_bf_points(BfArgs a) {
  const int p = blockIdx.x * BF_WG + threadIdx.x;
  if (p >= a.npts) return;
  int lo, hi;
  mt_range(a.obs_off, p, a.nobs, &lo, &hi);
  bool any = false;
  for (int e = lo; e < hi; e++) {
    a.obs_erased[e] = 0;
    const int k = a.obs_kf[e];
    if (!bf_kf_ok(a, k)) mt_flag(a.status, BF_ST_INDEX);
    else any |= a.obs_mark[e] != 0;
  }
  if (!any) return;
  int nobs = a.pt_nobs[p], ref = a.pt_ref_kf[p], last = -1;
  for (;;) {
    int t = a.ntgt;                                                 // the next target that still has a live observation of p
    for (int e = lo; e < hi; e++) {
      if (!a.obs_mark[e] || a.obs_erased[e]) continue;
      const int u = bf_turn(a, a.obs_kf[e]);
      if (u > last && u < t) t = u;
    }
    if (t >= a.ntgt) break;
    last = t;
    const int B = a.tgt_kf[t];
    for (int e = lo; e < hi; e++)
      if (a.obs_kf[e] == B) a.obs_erased[e] = 1;
    nobs--;
    if (ref == B)                                                   // (:150-151) observations_.begin()->first
      for (int e = lo; e < hi; e++)
        if (!a.obs_erased[e] && bf_kf_ok(a, a.obs_kf[e])) { ref = a.obs_kf[e]; break; }
    if (nobs <= 2) {                                                // (:154-155, MapPoint::SetBadFlag :170-191)
      a.pt_bad[p] = 1;
      for (int e = lo; e < hi; e++) {
        if (a.obs_erased[e]) continue;
        a.obs_erased[e] = 1;
        const int k = a.obs_kf[e], s = a.obs_slot[e];
        int slo, shi;
        if (!bf_kf_ok(a, k)) continue;
        mt_range(a.slot_off, k, a.nslots, &slo, &shi);
        if (s < 0 || s >= shi - slo) mt_flag(a.status, BF_ST_INDEX);
        else a.slot_pt[slo + s] = -1;                               // KeyFrame::EraseMapPointMatch(idx)
      }
      break;
    }
  }
  a.pt_nobs[p] = nobs; a.pt_ref_kf[p] = ref;
}

// the members of child row r get `stamp` in mark[]; the caller synchronises
__device__ __forceinline__ void bf_stamp_row(const BfArgs& a, int r, int n_add, int stamp) {
  int lo, hi;
  mt_range(a.child_off, r, a.nchild, &lo, &hi);
  for (int e = lo + (int)threadIdx.x; e < hi; e += BF_TWG)
    if (a.in_alive[e]) a.mark[a.child_kf[e]] = stamp;
  for (int j = threadIdx.x; j < n_add; j += BF_TWG)
    if (a.add_alive[j] && a.add_par[j] == r) a.mark[a.add_child[j]] = stamp;
}

// Steps 4 and 5 (:490-553), target after target
__global__ __launch_bounds__(BF_TWG) void k_bf_tree(BfArgs a) {
  __shared__ mt_u64 s_max[BF_TWG / 64];
  __shared__ int s_n, s_win[2];
  const int tid = threadIdx.x;
  int n_bad = 0, n_adopted = 0, n_fallback = 0, n_add = 0, stamp = 0;       // (workgroup-uniform)
  for (int t = 0; t < a.ntgt; t++) {
    if (!bf_active(a, t)) continue;
    const int B = a.tgt_kf[t], P = a.kf_parent[B], round = t + 1;
    int lo, hi;
    if (tid == 0) { s_n = 0; a.cand[P] = round; }
    __syncthreads();
    mt_range(a.child_off, B, a.nchild, &lo, &hi);                   // B's children as they stand now
    for (int e = lo + tid; e < hi; e += BF_TWG)
      if (a.in_alive[e]) { const int at = atomicAdd(&s_n, 1); if (at < a.nkf) { a.chl[at] = a.child_kf[e]; a.chl_src[at] = e; } }
    for (int j = tid; j < n_add; j += BF_TWG)
      if (a.add_alive[j] && a.add_par[j] == B) { const int at = atomicAdd(&s_n, 1); if (at < a.nkf) { a.chl[at] = a.add_child[j]; a.chl_src[at] = -1 - j; } }
    __syncthreads();
    const int nch = min(s_n, a.nkf);
    int remaining = nch;
    while (remaining > 0) {
      mt_u64 best_hi = 0, best_lo = 0; int best_ci = -1, best_entry = -1;
      for (int ci = 0; ci < nch; ci++) {                            // (workgroup-uniform)
        const int c = a.chl[ci];
        if (c < 0 || a.kf_bad[c]) continue;                         // (:503)
        const mt_u64 ckey = 0xFFFFFFFFu - bf_rank(a, c);
        int clo, chi;
        mt_range(a.conn_off, c, a.nconn, &clo, &chi);
        if (a.k_first[c] <= t) {                                    // c's list was re-sorted: all that is left of its row, position = rank descending
          for (int e = clo + tid; e < chi; e += BF_TWG) {
            const int k = a.conn_kf[e], m = a.mut[e], w = a.conn_w[e];
            if (!bf_kf_ok(a, k) || k == c || (m && m - 1 <= t) || a.cand[k] != round || w < 0) continue;
            const mt_u64 khi = (((mt_u64)(uint32_t)w + 1) << 32) | ckey, klo = (mt_u64)bf_rank(a, k) + 1;
            if (khi > best_hi || (khi == best_hi && klo > best_lo)) { best_hi = khi; best_lo = klo; best_ci = ci; best_entry = k; }
          }
        } else {                                                    // c's input list, the weight from c's row (0 when it is not there, :518)
          int olo, ohi;
          mt_range(a.ord_off, c, a.nord, &olo, &ohi);
          for (int i = olo + tid; i < ohi; i += BF_TWG) {
            const int k = a.ord_kf[i];
            if (!bf_kf_ok(a, k)) { mt_flag(a.status, BF_ST_INDEX); continue; }
            if (a.cand[k] != round) continue;
            int w = 0;
            for (int e = clo; e < chi; e++)
              if (a.conn_kf[e] == k) { w = a.conn_w[e]; break; }
            if (w < 0) continue;
            const mt_u64 khi = (((mt_u64)(uint32_t)w + 1) << 32) | ckey, klo = 0xFFFFFFFFull - (mt_u64)(i - olo) + 1;
            if (khi > best_hi || (khi == best_hi && klo > best_lo)) { best_hi = khi; best_lo = klo; best_ci = ci; best_entry = k; }
          }
        }
      }
      const mt_u64 top_hi = bf_block_max<BF_TWG>(best_hi, s_max);
      if (top_hi == 0) break;                                       // (:531 no candidate reaches any child)
      const mt_u64 top_lo = bf_block_max<BF_TWG>(best_hi == top_hi ? best_lo : 0, s_max);
      if (best_hi == top_hi && best_lo == top_lo) { s_win[0] = best_ci; s_win[1] = best_entry; }
      __syncthreads();
      const int ci = s_win[0], entry = s_win[1], c = a.chl[ci];
      bf_stamp_row(a, entry, n_add, ++stamp);
      __syncthreads();
      const bool fresh = a.mark[c] != stamp && (size_t)n_add < a.add_cap;
      __syncthreads();
      if (tid == 0) {                                               // (:521-527)
        if (fresh) { a.add_par[n_add] = entry; a.add_child[n_add] = c; a.add_alive[n_add] = 1; }
        const int src = a.chl_src[ci];
        if (src >= 0) a.in_alive[src] = 0; else a.add_alive[-1 - src] = 0;
        a.kf_parent[c] = entry; a.cand[c] = round; a.chl[ci] = -1;
      }
      __syncthreads();
      n_add += fresh; remaining--; n_adopted++;
    }
    if (remaining > 0) {                                            // (:535-542) the rest goes to P and stays in B's row
      bf_stamp_row(a, P, n_add, ++stamp);
      if (tid == 0) s_n = 0;
      __syncthreads();
      for (int ci = tid; ci < nch; ci += BF_TWG) {
        const int c = a.chl[ci];
        if (c < 0) continue;
        a.kf_parent[c] = P;
        if (a.mark[c] == stamp) continue;
        const size_t at = (size_t)n_add + (size_t)atomicAdd(&s_n, 1);
        if (at < a.add_cap) { a.add_par[at] = P; a.add_child[at] = c; a.add_alive[at] = 1; }
      }
      __syncthreads();
      n_add = (int)min((size_t)n_add + (size_t)s_n, a.add_cap);
      n_fallback += remaining;
    }
    mt_range(a.child_off, P, a.nchild, &lo, &hi);                   // (:544) B leaves P's children
    for (int e = lo + tid; e < hi; e += BF_TWG)
      if (a.in_alive[e] && a.child_kf[e] == B) a.in_alive[e] = 0;
    for (int j = tid; j < n_add; j += BF_TWG)
      if (a.add_alive[j] && a.add_par[j] == P && a.add_child[j] == B) a.add_alive[j] = 0;
    if (tid == 0) {
      double Twc[12], T[12];
      mc_pose_inverse(a.kf_Tcw + 12 * (size_t)P, Twc);
      mc_affine_mul(a.kf_Tcw + 12 * (size_t)B, Twc, T);             // (:545) Tcw * parent->GetPoseInverse()
      for (int q = 0; q < 12; q++) a.tgt_Tcp[12 * (size_t)t + q] = T[q];
      a.kf_bad[B] = 1;
    }
    n_bad++;
    __syncthreads();
  }
  if (tid == 0) { a.counts[0] = n_bad; a.counts[4] = n_adopted; a.counts[5] = n_fallback; a.n_add[0] = n_add; }
}

// is entry e of keyframe k's conn row part of its final row
__device__ __forceinline__ bool bf_conn_kept(const BfArgs& a, int k, int e) { const int q = a.conn_kf[e]; return bf_kf_ok(a, q) && q != k && a.mut[e] == 0; }

__global__ __launch_bounds__(BF_WG) void k_bf_count(BfArgs a) {
  __shared__ int s_sum[BF_WG / 64];
  const int k = blockIdx.x, tid = threadIdx.x, n_add = a.n_add[0];
  const bool gone = bf_turn(a, k) >= 0;                             // (:486-487) a target's row and list end empty
  int lo, hi, nconn = 0, nord = 0, nchild = 0;
  mt_range(a.conn_off, k, a.nconn, &lo, &hi);
  if (!gone)
    for (int e = lo + tid; e < hi; e += BF_WG) nconn += bf_conn_kept(a, k, e);
  const bool resorted = a.k_first[k] != BF_NEVER;
  mt_range(a.ord_off, k, a.nord, &lo, &hi);
  if (!gone && !resorted)
    for (int e = lo + tid; e < hi; e += BF_WG) {
      const bool ok = bf_kf_ok(a, a.ord_kf[e]);
      if (!ok) mt_flag(a.status, BF_ST_INDEX);
      nord += ok;
    }
  mt_range(a.child_off, k, a.nchild, &lo, &hi);
  for (int e = lo + tid; e < hi; e += BF_WG) nchild += a.in_alive[e];
  for (int j = tid; j < n_add; j += BF_WG) nchild += a.add_alive[j] && a.add_par[j] == k;
  nconn = bf_block_sum<BF_WG>(nconn, s_sum); nord = bf_block_sum<BF_WG>(nord, s_sum); nchild = bf_block_sum<BF_WG>(nchild, s_sum);
  if (tid == 0) { a.k_nconn[k] = nconn; a.k_nord[k] = gone ? 0 : resorted ? nconn : nord; a.k_nchild[k] = nchild; }
}

// out[i] = in[0] + ... + in[i - 1] for i in [0, n], by the whole workgroup; returns the total
__device__ __forceinline__ int bf_scan(const int32_t* in, int32_t* out, int n, int* sw) {
  int carry = 0;
  for (int b0 = 0; b0 < n; b0 += BF_TWG) {                          // (workgroup-uniform)
    const int i = b0 + (int)threadIdx.x;
    int tot;
    const int ex = mt_block_excl<BF_TWG>(i < n ? in[i] : 0, sw, &tot);
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) out[n] = carry;
  return carry;
}

__global__ __launch_bounds__(BF_TWG) void k_bf_scan(BfArgs a) {
  __shared__ int sw[BF_TWG / 64];
  const int n_conn = bf_scan(a.k_nconn, a.oconn_off, a.nkf, sw), n_ord = bf_scan(a.k_nord, a.oord_off, a.nkf, sw), n_child = bf_scan(a.k_nchild, a.ochild_off, a.nkf, sw);
  if (threadIdx.x == 0) {
    a.counts[1] = n_conn; a.counts[2] = n_ord; a.counts[3] = n_child;
    const uint32_t bits = (n_ord > a.cap_ord ? BF_ST_CAP_ORD : 0u) | (n_child > a.cap_child ? BF_ST_CAP_CHILD : 0u);
    if (bits) mt_flag(a.status, bits);
  }
}

__global__ __launch_bounds__(BF_WG) void k_bf_emit(BfArgs a) {
  __shared__ long long s_key[BF_WG];
  __shared__ int sw[BF_WG / 64];
  __shared__ int s_n;
  const int k = blockIdx.x, tid = threadIdx.x, n_add = a.n_add[0];
  const bool gone = bf_turn(a, k) >= 0, resorted = a.k_first[k] != BF_NEVER;
  const int coff = a.oconn_off[k], ooff = a.oord_off[k], choff = a.ochild_off[k];
  int lo, hi;
  mt_range(a.conn_off, k, a.nconn, &lo, &hi);
  if (!gone) {
    int run = 0;
    for (int eb = lo; eb < hi; eb += BF_WG) {                       // the row in its input order, the removed entries closed up
      const int e = eb + tid;
      const bool keep = e < hi && bf_conn_kept(a, k, e);
      int tot;
      const int at = coff + run + mt_block_excl<BF_WG>((int)keep, sw, &tot);
      if (keep && at < a.nconn) { a.oconn_kf[at] = a.conn_kf[e]; a.oconn_w[at] = a.conn_w[e]; }
      run += tot;
    }
    if (resorted) {                                                 // UpdateBestCovisibles (:172-193): everything left, descending (weight, rank)
      for (int ib = lo; ib < hi; ib += BF_WG) {
        const int i = ib + tid;
        const bool mine = i < hi && bf_conn_kept(a, k, i);
        const long long key = mine ? bf_key(a.conn_w[i], bf_rank(a, a.conn_kf[i])) : 0;
        int above = 0;
        for (int jb = lo; jb < hi; jb += BF_WG) {
          __syncthreads();
          const int j = jb + tid;
          s_key[tid] = j < hi && bf_conn_kept(a, k, j) ? bf_key(a.conn_w[j], bf_rank(a, a.conn_kf[j])) : LLONG_MIN;
          __syncthreads();
          const int m = min(BF_WG, hi - jb);
          for (int j2 = 0; j2 < m; j2++) above += s_key[j2] > key;
        }
        if (mine && above < a.k_nord[k] && ooff + above < a.cap_ord) { a.oord_kf[ooff + above] = a.conn_kf[i]; a.oord_w[ooff + above] = a.conn_w[i]; }
      }
    } else {                                                        // nobody touched it: the input list
      int olo, ohi, orun = 0;
      mt_range(a.ord_off, k, a.nord, &olo, &ohi);
      for (int eb = olo; eb < ohi; eb += BF_WG) {
        const int e = eb + tid;
        const bool keep = e < ohi && bf_kf_ok(a, a.ord_kf[e]);
        int tot;
        const int at = ooff + orun + mt_block_excl<BF_WG>((int)keep, sw, &tot);
        if (keep && at < a.cap_ord) { a.oord_kf[at] = a.ord_kf[e]; a.oord_w[at] = a.ord_w[e]; }
        orun += tot;
      }
    }
  }
  // the children: gathered (this workgroup's own stretch of cg), then placed in ascending rank
  const int n = a.k_nchild[k];
  const size_t cg_cap = (size_t)a.nchild + a.add_cap;
  if (n == 0 || (size_t)choff + (size_t)n > cg_cap) return;         // (workgroup-uniform)
  int32_t* g = a.cg + choff;
  __syncthreads();
  if (tid == 0) s_n = 0;
  __syncthreads();
  mt_range(a.child_off, k, a.nchild, &lo, &hi);
  for (int e = lo + tid; e < hi; e += BF_WG)
    if (a.in_alive[e]) { const int at = atomicAdd(&s_n, 1); if (at < n) g[at] = a.child_kf[e]; }
  for (int j = tid; j < n_add; j += BF_WG)
    if (a.add_alive[j] && a.add_par[j] == k) { const int at = atomicAdd(&s_n, 1); if (at < n) g[at] = a.add_child[j]; }
  __syncthreads();                                                  // (the entries are read back by this workgroup only)
  uint32_t* s_rank = (uint32_t*)s_key;
  for (int ib = 0; ib < n; ib += BF_WG) {
    const int i = ib + tid;
    const int c = i < n ? g[i] : 0;
    const uint32_t r = i < n ? bf_rank(a, c) : 0u;
    int pos = 0;
    for (int jb = 0; jb < n; jb += BF_WG) {
      __syncthreads();
      if (jb + tid < n) s_rank[tid] = bf_rank(a, g[jb + tid]);
      __syncthreads();
      const int m = min(BF_WG, n - jb);
      for (int j = 0; j < m; j++) pos += s_rank[j] < r;
    }
    if (i < n && pos < n && choff + pos < a.cap_child) a.ochild_kf[choff + pos] = c;
  }
}

// workspace sections, each rounded up to 256 bytes; [0, cleared) is zeroed and k_first preset by every call
struct BfWs { size_t tfirst, rhit, mark, cand, mut, n_add, in_alive, obs_mark, cleared, k_first, t_st, add_par, add_child, add_alive, chl, chl_src, k_n, cg, add_cap, total; };
static BfWs bf_workspace(int ntgt, int nkf, int nchild, int nconn, int nobs) {
  BfWs w; Carve ws;
  const size_t nk = (size_t)nkf;
  w.tfirst = ws.take(4 * nk); w.rhit = ws.take(4 * nk); w.mark = ws.take(4 * nk); w.cand = ws.take(4 * nk); w.mut = ws.take(4 * (size_t)nconn);
  w.n_add = ws.take(4); w.in_alive = ws.take((size_t)nchild); w.obs_mark = ws.take((size_t)nobs);
  w.cleared = ws.total;
  w.k_first = ws.take(4 * nk); w.t_st = ws.take(4 * (size_t)ntgt);
  // a turn hands every child of its target to ONE new row, and a row is a set: at most nkf new memberships per target
  w.add_cap = (size_t)ntgt * nk;
  w.add_par = ws.take(4 * w.add_cap); w.add_child = ws.take(4 * w.add_cap); w.add_alive = ws.take(w.add_cap);
  w.chl = ws.take(4 * nk); w.chl_src = ws.take(4 * nk); w.k_n = ws.take(3 * 4 * nk); w.cg = ws.take(4 * ((size_t)nchild + w.add_cap));
  w.total = ws.total;
  return w;
}

}  // namespace orbhip

extern "C" {

int orbl_set_bad_keyframes_workspace(int ntgt, int nkf, int nchild, int nconn, int nobs, size_t* bytes) {
  ORBHIP_REQUIRE(ntgt >= 0 && nkf >= 0 && nchild >= 0 && nconn >= 0 && nobs >= 0 && bytes, ORBHIP_EINVAL, "orbl_set_bad_keyframes_workspace: bad argument");
  *bytes = orbhip::bf_workspace(ntgt, nkf, nchild, nconn, nobs).total;
  return 0;
}

int orbl_set_bad_keyframes_device(int ntgt, const int32_t* tgt_kf, const uint8_t* tgt_flags, const uint8_t* tgt_mask, int nkf, uint8_t* kf_bad, int32_t* kf_parent,
                                  const int32_t* kf_rank, const double* kf_Tcw, int nchild, const int32_t* child_off, const int32_t* child_kf, int nconn,
                                  const int32_t* conn_off, const int32_t* conn_kf, const int32_t* conn_w, int nord, const int32_t* ord_off, const int32_t* ord_kf,
                                  const int32_t* ord_w, int npts, int nslots, const int32_t* kf_slot_off, int32_t* kf_slot_pt, uint8_t* pt_bad, int32_t* pt_nobs,
                                  int32_t* pt_ref_kf, int nobs, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot, uint8_t* obs_erased,
                                  int cap_ord, int cap_child, int32_t* tgt_status, double* tgt_Tcp, int32_t* oconn_off, int32_t* oconn_kf, int32_t* oconn_w,
                                  int32_t* oord_off, int32_t* oord_kf, int32_t* oord_w, int32_t* ochild_off, int32_t* ochild_kf, int32_t* counts, uint32_t* status,
                                  void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(ntgt >= 0 && nkf >= 0 && nchild >= 0 && nconn >= 0 && nord >= 0 && npts >= 0 && nslots >= 0 && nobs >= 0, ORBHIP_EINVAL,
                 "orbl_set_bad_keyframes: negative count");
  ORBHIP_REQUIRE(cap_ord >= 0 && cap_child >= 0, ORBHIP_EINVAL, "orbl_set_bad_keyframes: negative capacity");
  ORBHIP_REQUIRE(workspace && counts && oconn_off && oord_off && ochild_off, ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL workspace, counts or offset output");
  ORBHIP_REQUIRE(ntgt == 0 || (tgt_kf && tgt_status && tgt_Tcp), ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL target argument");
  ORBHIP_REQUIRE(nkf == 0 || (kf_bad && kf_parent && kf_Tcw && child_off && conn_off && ord_off), ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL keyframe table");
  ORBHIP_REQUIRE((nchild == 0 || (nkf > 0 && child_kf)) && (nconn == 0 || (nkf > 0 && conn_kf && conn_w)) && (nord == 0 || (nkf > 0 && ord_kf && ord_w)), ORBHIP_EINVAL,
                 "orbl_set_bad_keyframes: NULL table entries");
  const bool points = kf_slot_off != nullptr;
  ORBHIP_REQUIRE(points ? (obs_off && (nslots == 0 || kf_slot_pt) && (npts == 0 || (pt_bad && pt_nobs && pt_ref_kf)) && (nobs == 0 || (obs_kf && obs_slot && obs_erased)))
                        : (!kf_slot_pt && !pt_bad && !pt_nobs && !pt_ref_kf && !obs_off && !obs_kf && !obs_slot && !obs_erased),
                 ORBHIP_EINVAL, "orbl_set_bad_keyframes: the point tables are given together or not at all");
  ORBHIP_REQUIRE((nconn == 0 || (oconn_kf && oconn_w)) && (cap_ord == 0 || (oord_kf && oord_w)) && (cap_child == 0 || ochild_kf), ORBHIP_EINVAL,
                 "orbl_set_bad_keyframes: NULL list output");
  const void* words[] = {tgt_kf, kf_parent, kf_rank, child_off, child_kf, conn_off, conn_kf, conn_w, ord_off, ord_kf, ord_w, kf_slot_off, kf_slot_pt, pt_nobs, pt_ref_kf,
                         obs_off, obs_kf, obs_slot, tgt_status, oconn_off, oconn_kf, oconn_w, oord_off, oord_kf, oord_w, ochild_off, ochild_kf, counts, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_set_bad_keyframes: 32-bit arrays must be 4-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)kf_Tcw % 8 == 0 && (uintptr_t)tgt_Tcp % 8 == 0, ORBHIP_EINVAL, "orbl_set_bad_keyframes: the poses must be 8-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)workspace % 4 == 0, ORBHIP_EINVAL, "orbl_set_bad_keyframes: workspace must be 4-byte aligned");
  if (!points) npts = nslots = nobs = 0;
  const BfWs ws = bf_workspace(ntgt, nkf, nchild, nconn, nobs);
  uint8_t* wb = (uint8_t*)workspace;
  BfArgs A; std::memset(&A, 0, sizeof(A));
  A.ntgt = ntgt; A.nkf = nkf; A.npts = npts; A.nchild = nchild; A.nconn = nconn; A.nord = nord; A.nslots = nslots; A.nobs = nobs; A.cap_ord = cap_ord; A.cap_child = cap_child;
  A.tgt_kf = tgt_kf; A.tgt_flags = tgt_flags; A.tgt_mask = tgt_mask; A.kf_bad = kf_bad; A.kf_parent = kf_parent; A.kf_rank = kf_rank; A.kf_Tcw = kf_Tcw;
  A.child_off = child_off; A.child_kf = child_kf; A.conn_off = conn_off; A.conn_kf = conn_kf; A.conn_w = conn_w; A.ord_off = ord_off; A.ord_kf = ord_kf; A.ord_w = ord_w;
  A.slot_off = kf_slot_off; A.slot_pt = kf_slot_pt; A.pt_bad = pt_bad; A.pt_nobs = pt_nobs; A.pt_ref_kf = pt_ref_kf; A.obs_off = obs_off; A.obs_kf = obs_kf;
  A.obs_slot = obs_slot; A.obs_erased = obs_erased; A.tgt_status = tgt_status; A.tgt_Tcp = tgt_Tcp; A.oconn_off = oconn_off; A.oconn_kf = oconn_kf; A.oconn_w = oconn_w;
  A.oord_off = oord_off; A.oord_kf = oord_kf; A.oord_w = oord_w; A.ochild_off = ochild_off; A.ochild_kf = ochild_kf; A.counts = counts; A.status = status;
  A.tfirst = (int32_t*)(wb + ws.tfirst); A.rhit = (int32_t*)(wb + ws.rhit); A.mark = (int32_t*)(wb + ws.mark); A.cand = (int32_t*)(wb + ws.cand);
  A.mut = (int32_t*)(wb + ws.mut); A.n_add = (int32_t*)(wb + ws.n_add); A.in_alive = wb + ws.in_alive; A.obs_mark = wb + ws.obs_mark;
  A.k_first = (int32_t*)(wb + ws.k_first); A.t_st = (int32_t*)(wb + ws.t_st); A.add_par = (int32_t*)(wb + ws.add_par); A.add_child = (int32_t*)(wb + ws.add_child);
  A.add_alive = wb + ws.add_alive; A.chl = (int32_t*)(wb + ws.chl); A.chl_src = (int32_t*)(wb + ws.chl_src);
  int32_t* kn = (int32_t*)(wb + ws.k_n);
  A.k_nconn = kn; A.k_nord = kn + nkf; A.k_nchild = kn + 2 * (size_t)nkf; A.cg = (int32_t*)(wb + ws.cg); A.add_cap = ws.add_cap;
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0, ws.cleared, st));
  if (nkf > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.k_first, 0x7F, 4 * (size_t)nkf, st));
  const int n_init = std::max(std::max(ntgt, nkf), npts), n_mark = std::max(std::max(ntgt, nconn), std::max(nchild, nslots));
  if (n_init > 0) hipLaunchKernelGGL(k_bf_init, dim3((n_init + BF_WG - 1) / BF_WG), dim3(BF_WG), 0, st, A);
  if (n_mark > 0) hipLaunchKernelGGL(k_bf_mark, dim3((n_mark + BF_WG - 1) / BF_WG), dim3(BF_WG), 0, st, A);
  if (npts > 0) hipLaunchKernelGGL(k_bf_points, dim3((npts + BF_WG - 1) / BF_WG), dim3(BF_WG), 0, st, A);
  hipLaunchKernelGGL(k_bf_tree, dim3(1), dim3(BF_TWG), 0, st, A);
  if (nkf > 0) hipLaunchKernelGGL(k_bf_count, dim3(nkf), dim3(BF_WG), 0, st, A);
  hipLaunchKernelGGL(k_bf_scan, dim3(1), dim3(BF_TWG), 0, st, A);
  if (nkf > 0) hipLaunchKernelGGL(k_bf_emit, dim3(nkf), dim3(BF_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_set_bad_keyframes(int ntgt, const int32_t* tgt_kf, const uint8_t* tgt_flags, const uint8_t* tgt_mask, int nkf, uint8_t* kf_bad, int32_t* kf_parent,
                           const int32_t* kf_rank, const double* kf_Tcw, const int32_t* child_off, const int32_t* child_kf, const int32_t* conn_off,
                           const int32_t* conn_kf, const int32_t* conn_w, const int32_t* ord_off, const int32_t* ord_kf, const int32_t* ord_w, int npts,
                           const int32_t* kf_slot_off, int32_t* kf_slot_pt, uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_ref_kf, const int32_t* obs_off,
                           const int32_t* obs_kf, const int32_t* obs_slot, uint8_t* obs_erased, int cap_ord, int cap_child, int32_t* tgt_status, double* tgt_Tcp,
                           int32_t* oconn_off, int32_t* oconn_kf, int32_t* oconn_w, int32_t* oord_off, int32_t* oord_kf, int32_t* oord_w, int32_t* ochild_off,
                           int32_t* ochild_kf, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  static const char E[] = "orbl_set_bad_keyframes";
  ORBHIP_REQUIRE(ntgt >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_set_bad_keyframes: negative count");
  ORBHIP_REQUIRE(cap_ord >= 0 && cap_child >= 0, ORBHIP_EINVAL, "orbl_set_bad_keyframes: negative capacity");
  ORBHIP_REQUIRE(counts && oconn_off && oord_off && ochild_off, ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL counts or offset output");
  ORBHIP_REQUIRE(ntgt == 0 || (tgt_kf && tgt_status && tgt_Tcp), ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL target argument");
  ORBHIP_REQUIRE(nkf == 0 || (kf_bad && kf_parent && kf_Tcw && child_off && conn_off && ord_off), ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL keyframe table");
  const bool any_pt = kf_slot_off || kf_slot_pt || pt_bad || pt_nobs || pt_ref_kf || obs_off || obs_kf || obs_slot || obs_erased;
  const bool points = kf_slot_off && obs_off;
  ORBHIP_REQUIRE(!any_pt || points, ORBHIP_EINVAL, "orbl_set_bad_keyframes: the point tables are given together or not at all");
  if (!points) npts = 0;
  int nchild = 0, nconn = 0, nord = 0, nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "child_off", child_off, nkf, &nchild));
  ORBHIP_ARG(check_csr(E, "conn_off", conn_off, nkf, &nconn));
  ORBHIP_ARG(check_csr(E, "ord_off", ord_off, nkf, &nord));
  if (points) {
    ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
    ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
    ORBHIP_REQUIRE((nslots == 0 || kf_slot_pt) && (npts == 0 || (pt_bad && pt_nobs && pt_ref_kf)) && (nobs == 0 || (obs_kf && obs_slot && obs_erased)), ORBHIP_EINVAL,
                   "orbl_set_bad_keyframes: the point tables are given together or not at all");
  }
  ORBHIP_REQUIRE((nchild == 0 || child_kf) && (nconn == 0 || (conn_kf && conn_w && oconn_kf && oconn_w)) && (nord == 0 || (ord_kf && ord_w)), ORBHIP_EINVAL,
                 "orbl_set_bad_keyframes: NULL CSR entries");
  ORBHIP_REQUIRE((cap_ord == 0 || (oord_kf && oord_w)) && (cap_child == 0 || ochild_kf), ORBHIP_EINVAL, "orbl_set_bad_keyframes: NULL list output");
  ORBHIP_ARG(check_listed_once(E, "tgt_kf", tgt_kf, ntgt, nkf));
  if (kf_rank) ORBHIP_ARG(check_permutation(E, "kf_rank", kf_rank, nkf));
  ORBHIP_ARG(check_index(E, "kf_parent", kf_parent, nkf, nkf, true));
  ORBHIP_ARG(check_index(E, "child_kf", child_kf, nchild, nkf));
  ORBHIP_ARG(check_index(E, "conn_kf", conn_kf, nconn, nkf));
  ORBHIP_ARG(check_index(E, "ord_kf", ord_kf, nord, nkf));
  for (int t = 0; t < ntgt; t++) {
    const bool skipped = (tgt_mask && !tgt_mask[t]) || (tgt_flags && (tgt_flags[t] & 3));
    if (skipped) continue;
    const int B = tgt_kf[t];
    ORBHIP_REQUIRE(!kf_bad[B], ORBHIP_EINVAL, "orbl_set_bad_keyframes: a target is already bad");
    ORBHIP_REQUIRE(kf_parent[B] >= 0 && kf_parent[B] != B, ORBHIP_EINVAL, "orbl_set_bad_keyframes: a target has no parent or is its own (the reference dereferences it)");
  }
  {
    std::vector<int32_t> seen((size_t)nkf, -1);                     // (per ROW of a table: the last row that named the keyframe)
    for (int k = 0; k < nkf; k++)
      for (int e = conn_off[k]; e < conn_off[k + 1]; e++) {
        ORBHIP_REQUIRE(conn_kf[e] != k && seen[conn_kf[e]] != k, ORBHIP_EINVAL, "orbl_set_bad_keyframes: a row of conn_kf names itself or a keyframe twice");
        seen[conn_kf[e]] = k;
      }
    std::fill(seen.begin(), seen.end(), -1);
    for (int k = 0; k < nkf; k++)
      for (int e = child_off[k]; e < child_off[k + 1]; e++) {
        ORBHIP_REQUIRE(child_kf[e] != k && seen[child_kf[e]] != k, ORBHIP_EINVAL, "orbl_set_bad_keyframes: a row of child_kf names itself or a keyframe twice");
        seen[child_kf[e]] = k;
      }
  }
  if (points) {
    ORBHIP_ARG(check_index(E, "kf_slot_pt", kf_slot_pt, nslots, npts, true));
    ORBHIP_ARG(check_index(E, "pt_ref_kf", pt_ref_kf, npts, nkf, true));
    ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
    std::vector<int32_t> seen((size_t)nkf, -1);                     // (per point: the last point that named the keyframe)
    for (int p = 0; p < npts; p++)
      for (int e = obs_off[p]; e < obs_off[p + 1]; e++) {
        const int k = obs_kf[e], s = obs_slot[e];
        ORBHIP_REQUIRE(s >= 0 && s < kf_slot_off[k + 1] - kf_slot_off[k], ORBHIP_EINVAL, "orbl_set_bad_keyframes: an obs_slot lies outside its keyframe's slots");
        ORBHIP_REQUIRE(seen[k] != p, ORBHIP_EINVAL, "orbl_set_bad_keyframes: an observation list names a keyframe twice");
        ORBHIP_REQUIRE(kf_slot_pt[kf_slot_off[k] + s] == p, ORBHIP_EINVAL, "orbl_set_bad_keyframes: an observation's slot does not hold its point");
        seen[k] = p;
      }
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nt = (size_t)ntgt, nk = (size_t)nkf, np = (size_t)npts;
  RoundTrip R(W);
  const HostIn<int32_t> d_tgt = R.in(tgt_kf, nt), d_rank = R.in(kf_rank, nk), d_child_off = R.csr(child_off, nk), d_child_kf = R.in(child_kf, (size_t)nchild);
  const HostIn<int32_t> d_conn_off = R.csr(conn_off, nk), d_conn_kf = R.in(conn_kf, (size_t)nconn), d_conn_w = R.in(conn_w, (size_t)nconn);
  const HostIn<int32_t> d_ord_off = R.csr(ord_off, nk), d_ord_kf = R.in(ord_kf, (size_t)nord), d_ord_w = R.in(ord_w, (size_t)nord);
  const HostIn<int32_t> d_slot_off = R.csr(points ? kf_slot_off : nullptr, nk), d_obs_off = R.csr(points ? obs_off : nullptr, np);
  const HostIn<int32_t> d_obs_kf = R.in(obs_kf, (size_t)nobs), d_obs_slot = R.in(obs_slot, (size_t)nobs);
  const HostIn<uint8_t> d_flags = R.in(tgt_flags, nt), d_mask = R.in(tgt_mask, nt);
  const HostIn<double> d_Tcw = R.in(kf_Tcw, 12 * nk);
  const HostOut<uint8_t> io_kf_bad = R.inout(kf_bad, nk), io_pt_bad = R.inout(pt_bad, np);
  const HostOut<int32_t> io_parent = R.inout(kf_parent, nk), io_slot_pt = R.inout(kf_slot_pt, (size_t)nslots), io_nobs = R.inout(pt_nobs, np), io_ref = R.inout(pt_ref_kf, np);
  const HostOut<int32_t> o_counts = R.out<int32_t>(6), o_tgt_status = R.out<int32_t>(nt);
  const HostOut<double> o_Tcp = R.out<double>(12 * nt);
  const HostOut<uint8_t> o_erased = R.out<uint8_t>((size_t)nobs, points);
  const HostOut<int32_t> o_conn_off = R.out<int32_t>(nk + 1), o_conn_kf = R.out<int32_t>((size_t)nconn), o_conn_w = R.out<int32_t>((size_t)nconn);
  const HostOut<int32_t> o_ord_off = R.out<int32_t>(nk + 1), o_ord_kf = R.out<int32_t>((size_t)cap_ord), o_ord_w = R.out<int32_t>((size_t)cap_ord);
  const HostOut<int32_t> o_child_off = R.out<int32_t>(nk + 1), o_child_kf = R.out<int32_t>((size_t)cap_child);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(bf_workspace(ntgt, nkf, nchild, nconn, nobs).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_set_bad_keyframes_device(ntgt, d_tgt.dev(), d_flags.dev(), d_mask.dev(), nkf, io_kf_bad.dev(), io_parent.dev(), d_rank.dev(), d_Tcw.dev(), nchild,
                                          d_child_off.dev(), d_child_kf.dev(), nconn, d_conn_off.dev(), d_conn_kf.dev(), d_conn_w.dev(), nord, d_ord_off.dev(),
                                          d_ord_kf.dev(), d_ord_w.dev(), npts, nslots, d_slot_off.dev(), io_slot_pt.dev(), io_pt_bad.dev(), io_nobs.dev(), io_ref.dev(),
                                          nobs, d_obs_off.dev(), d_obs_kf.dev(), d_obs_slot.dev(), o_erased.dev(), cap_ord, cap_child, o_tgt_status.dev(), o_Tcp.dev(),
                                          o_conn_off.dev(), o_conn_kf.dev(), o_conn_w.dev(), o_ord_off.dev(), o_ord_kf.dev(), o_ord_w.dev(), o_child_off.dev(),
                                          o_child_kf.dev(), o_counts.dev(), o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 6);
  const size_t n_conn = (size_t)o_counts[1], n_ord = (size_t)o_counts[2], n_child = (size_t)o_counts[3];
  if (n_ord > (size_t)cap_ord || n_child > (size_t)cap_child) {
    set_error("orbl_set_bad_keyframes: wanted %d list entries and %d children; capacities %d, %d", o_counts[2], o_counts[3], cap_ord, cap_child);
    return ORBHIP_ECAP;
  }
  R.copy_out(io_kf_bad, kf_bad, nk); R.copy_out(io_parent, kf_parent, nk);
  R.copy_out(io_slot_pt, kf_slot_pt, (size_t)nslots); R.copy_out(io_pt_bad, pt_bad, np); R.copy_out(io_nobs, pt_nobs, np); R.copy_out(io_ref, pt_ref_kf, np);
  R.copy_out(o_erased, obs_erased, (size_t)nobs);
  R.copy_out(o_tgt_status, tgt_status, nt); R.copy_out(o_Tcp, tgt_Tcp, 12 * nt);
  R.copy_out(o_conn_off, oconn_off, nk + 1); R.copy_out(o_ord_off, oord_off, nk + 1); R.copy_out(o_child_off, ochild_off, nk + 1);
  R.copy_out(o_conn_kf, oconn_kf, n_conn); R.copy_out(o_conn_w, oconn_w, n_conn); R.copy_out(o_ord_kf, oord_kf, n_ord); R.copy_out(o_ord_w, oord_w, n_ord);
  R.copy_out(o_child_kf, ochild_kf, n_child);
  return 0;
}

}  // extern "C"
