// orb_essgraph.inc -- the two halves of CeresOptimizer::OptimizeEssentialGraph around the optimisation, on the flat map tables:
// orbl_essential_graph_assemble* numbers the vertices, takes their Sim(3) logarithms and lists the edges (src/CeresOptimizer.cc:769-905,
// in the reading csrc/compat/orbslam_dropin.h fixed), and orbl_essential_graph_apply* writes the optimised Sim(3)s back (:916-956): SetPose,
// the map points through their reference keyframe, UpdateNormalAndDepth.  Textually included by orb_localmap.hip.  FP64 throughout, no
// fused multiply-add (-ffp-contract=off); the Sim(3) arithmetic is sim3_math.h's (DESIGN.md section 2, "OptimizeEssentialGraph on the
// tables").
//
// assemble: both lists are ORDERED compactions.  One lane per kf_rank position holds a flag (vertex) or a pair of counts (its
// loop-connection edges, its per-keyframe edges); an exclusive scan (mt_block_excl per workgroup, k_mt_scan_sums across them) gives the
// lane its places, and the lane writes them in the order the reference walks its keyframe.  Atomics only take order-free maxima, ors
// and integer sums.
//   k_eg_stamp     one lane per keyframe / group entry / target / table entry: the inverse of kf_rank, where the group and the targets
//                  name a keyframe (atomicMax: a repeat is flagged), the checks of the device form
//   k_eg_vscan     one lane per kf_rank position: the vertex flags;   k_eg_vertices: kf_vtx, vtx_kf, lie7, vtx_fixed, and per keyframe
//                  exp of its block and the pose it enters the per-keyframe edges with (to the workspace), counts[0]
//   k_eg_escan     one lane per kf_rank position: the walk of eg_walk, counting;   k_eg_emit: the same walk, writing
// apply: keyframes and points are independent of each other once the vertex of every keyframe is known.
//   k_ea_stamp     one lane per vertex: vtx_of[k] (atomicMax)
//   k_ea_pose      one lane per vertex: exp(lie_orig), exp(lie_opt)^-1 (to the workspace), the new pose and centre
//   k_ea_points    one lane per point: the new position, then the normal / depth walk (mt_normal_depth) over the NEW centres
// Outputs are written with vector stores only.
#include "orb_maptable.h"
#include "sim3_math.h"

namespace orbhip {

#define EG_WG 256
#define EG_ST_OFFSETS 1u          /* *status bits of orbl_essential_graph_assemble_device and orbl_essential_graph_apply_device */
#define EG_ST_KF 2u
#define EG_ST_PT 4u               /* (kept free: the meaning of orbl_local_ba_assemble_device) */
#define EG_ST_RANK 8u
#define EG_ST_LEVEL 16u
#define EG_ST_CAP_VTX 32u
#define EG_ST_CAP_EDGES 64u
#define EG_ST_SIM3 512u           /* a corrected / non_corrected row (assemble) or a tangent (apply) that is not finite, or |q|^2 = 0 */

struct EgArgs {
  int nkf, nconn, ntgt, n_child, n_loop, n_cw, n_ord, n_link, loop_kf, cur_kf, min_weight, cap_vtx, cap_edges, nb;
  const int32_t* kf_id; const uint8_t* kf_bad; const int32_t* kf_rank; const double* kf_Tcw; const int32_t* kf_parent;
  const int32_t *child_off, *child_kf, *loop_off, *loop_edge, *conn_off, *conn_kf, *conn_w, *ord_off, *ord_kf, *ord_w;
  const int32_t* group_kf; const double *corrected, *non_corrected; const int32_t *tgt_kf, *link_off, *link_kf;
  int32_t *counts, *vtx_kf, *kf_vtx; double* lie7; uint8_t* vtx_fixed; int32_t *edge_j, *edge_i; double* edge_S; uint8_t* edge_kind; uint32_t* status;
  // workspace: inv_kf[nkf] | gpos[nkf] | tpos[nkf] (all set to all ones per call) | vscan[nkf] | vsums[nb + 1] | escan[nkf] | esums[nb + 1] |
  // wB[nkf][7] | wW[nkf][7]
  int32_t *inv_kf, *gpos, *tpos; mt_u64 *vscan, *vsums, *escan, *esums; double *wB, *wW;
};

__device__ __forceinline__ bool eg_kf_bad(const EgArgs& a, int k) { return a.kf_bad && a.kf_bad[k]; }
__device__ __forceinline__ bool eg_in(const EgArgs& a, int k) { return k >= 0 && k < a.nkf; }
__device__ __forceinline__ long long eg_rank(const EgArgs& a, int k) { return a.kf_rank ? (long long)a.kf_rank[k] : (long long)k; }
__device__ __forceinline__ int eg_kf_of_rank(const EgArgs& a, int r) { return a.kf_rank ? a.inv_kf[r] : r; }
// (a CSR row whose offsets are out of range is empty wherever the walk meets it - mt_range - and k_eg_stamp flags it)
__device__ __forceinline__ bool eg_sim3_ok(const double* S) {
  bool fin = true;
  for (int q = 0; q < 7; q++) fin = fin && isfinite(S[q]);
  return fin && ((S[0] * S[0] + S[1] * S[1]) + (S[2] * S[2] + S[3] * S[3])) > 0.0;
}

__global__ __launch_bounds__(EG_WG) void k_eg_stamp(EgArgs a) {
  const int i = blockIdx.x * EG_WG + threadIdx.x;
  if (i < a.nkf) {
    int lo, hi;
    if (!mt_range(a.child_off, i, a.n_child, &lo, &hi) || !mt_range(a.loop_off, i, a.n_loop, &lo, &hi) || !mt_range(a.conn_off, i, a.n_cw, &lo, &hi) ||
        !mt_range(a.ord_off, i, a.n_ord, &lo, &hi))
      mt_flag(a.status, EG_ST_OFFSETS);
    const int par = a.kf_parent[i];
    if (par < -1 || par >= a.nkf) mt_flag(a.status, EG_ST_KF);
    if (a.kf_rank) {
      const int r = a.kf_rank[i];
      if (r < 0 || r >= a.nkf) mt_flag(a.status, EG_ST_RANK);
      else if (atomicMax(&a.inv_kf[r], i) != -1) mt_flag(a.status, EG_ST_RANK);  // (not a permutation: the highest index holds the place)
    }
  }
  if (i < a.nconn) {
    const int k = a.group_kf[i];
    if (!eg_in(a, k)) mt_flag(a.status, EG_ST_KF);
    else if (!eg_sim3_ok(a.corrected + 7 * (size_t)i) || !eg_sim3_ok(a.non_corrected + 7 * (size_t)i)) mt_flag(a.status, EG_ST_SIM3);
    else if (atomicMax(&a.gpos[k], i) != -1) mt_flag(a.status, EG_ST_KF);        // (a keyframe listed twice: its last instance counts)
  }
  if (i < a.ntgt) {
    int lo, hi;
    if (!mt_range(a.link_off, i, a.n_link, &lo, &hi)) mt_flag(a.status, EG_ST_OFFSETS);
    const int k = a.tgt_kf[i];
    if (!eg_in(a, k)) mt_flag(a.status, EG_ST_KF);
    else if (atomicMax(&a.tpos[k], i) != -1) mt_flag(a.status, EG_ST_KF);
  }
  // every entry of the five tables: one out of range is skipped wherever the walk meets it
  if ((i < a.n_child && !eg_in(a, a.child_kf[i])) || (i < a.n_loop && !eg_in(a, a.loop_edge[i])) || (i < a.n_cw && !eg_in(a, a.conn_kf[i])) ||
      (i < a.n_ord && !eg_in(a, a.ord_kf[i])) || (i < a.n_link && !eg_in(a, a.link_kf[i])))
    mt_flag(a.status, EG_ST_KF);
}

__global__ __launch_bounds__(EG_WG) void k_eg_vscan(EgArgs a) {
  __shared__ mt_u64 sw[EG_WG / 64];
  const int r = blockIdx.x * EG_WG + threadIdx.x;
  const int k = r < a.nkf ? eg_kf_of_rank(a, r) : -1;
  mt_u64 tot;
  const mt_u64 ex = mt_block_excl<EG_WG>(k >= 0 && !eg_kf_bad(a, k) ? 1ull : 0ull, sw, &tot);
  if (r < a.nkf) a.vscan[r] = ex;
  if (threadIdx.x == 0) a.vsums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(EG_WG) void k_eg_vertices(EgArgs a) {
  const int r = blockIdx.x * EG_WG + threadIdx.x;
  if (r >= a.nkf) return;
  if (r == 0) {
    const int n = (int)a.vsums[a.nb];
    a.counts[0] = n;
    if (n > a.cap_vtx) mt_flag(a.status, EG_ST_CAP_VTX);
  }
  const int k = eg_kf_of_rank(a, r);
  if (k < 0 || eg_kf_bad(a, k)) return;                                        // (kf_vtx was set to -1)
  const int v = (int)(a.vscan[r] + a.vsums[blockIdx.x]);
  a.kf_vtx[k] = v;
  const int g = a.gpos[k];
  double S[7], x[7], B[7];
  if (g >= 0) { for (int q = 0; q < 7; q++) S[q] = a.corrected[7 * (size_t)g + q]; }     // (:775-782)
  else {                                                                       // (:783-788) Sim3d(RxSO3d(1.0, Rcw), tcw)
    double T[12];
    for (int q = 0; q < 12; q++) T[q] = a.kf_Tcw[12 * (size_t)k + q];
    mc_se3_as_sim3(T, S);
  }
  s3_log(S, x);
  s3_exp(x, B);
  for (int q = 0; q < 7; q++) {
    a.wB[7 * (size_t)k + q] = B[q];
    a.wW[7 * (size_t)k + q] = g >= 0 ? a.non_corrected[7 * (size_t)g + q] : B[q];          // (:826-833, :842-847)
  }
  if (v >= a.cap_vtx) return;
  a.vtx_kf[v] = k;
  for (int q = 0; q < 7; q++) a.lie7[7 * (size_t)v + q] = x[q];
  a.vtx_fixed[v] = k == a.loop_kf ? 1 : 0;                                     // (:790-792)
}

// the entry of arr[lo, hi) of the least kf_rank above *prev (*prev becomes that rank), or -1; entries out of range are skipped, a
// keyframe named twice is met once
__device__ __forceinline__ int eg_next(const EgArgs& a, const int32_t* arr, int lo, int hi, long long* prev) {
  int best = -1;
  long long br = 0x7FFFFFFFFFFFFFFFll;
  for (int e = lo; e < hi; e++) {
    const int k = arr[e];
    if (!eg_in(a, k)) continue;
    const long long rk = eg_rank(a, k);
    if (rk > *prev && rk < br) { br = rk; best = k; }
  }
  if (best >= 0) *prev = br;
  return best;
}
__device__ __forceinline__ bool eg_holds(const int32_t* arr, int lo, int hi, int k) {
  for (int e = lo; e < hi; e++) if (arr[e] == k) return true;
  return false;
}
// KeyFrame::GetWeight (src/KeyFrame.cc:312-319): 0 when j is not connected
__device__ __forceinline__ int eg_weight(const EgArgs& a, int i, int j) {
  int lo, hi;
  mt_range(a.conn_off, i, a.n_cw, &lo, &hi);
  for (int e = lo; e < hi; e++) if (a.conn_kf[e] == j) return a.conn_w[e];
  return 0;
}
// the weight rule of a loop connection (:803-806): the (current, loop) pair is exempt
__device__ __forceinline__ bool eg_lc_pass(const EgArgs& a, int i, int j) {
  return !((a.kf_id[i] != a.kf_id[a.cur_kf] || a.kf_id[j] != a.kf_id[a.loop_kf]) && eg_weight(a, i, j) < a.min_weight);
}
// whether target t_kf's row gave the edge to `other` (its pair is in inserted_edges, :819)
__device__ __forceinline__ bool eg_linked(const EgArgs& a, int t_kf, int other) {
  const int t = a.tpos[t_kf];
  if (t < 0) return false;
  int lo, hi;
  mt_range(a.link_off, t, a.n_link, &lo, &hi);
  return eg_holds(a.link_kf, lo, hi, other) && a.kf_vtx[t_kf] >= 0 && a.kf_vtx[other] >= 0 && eg_lc_pass(a, t_kf, other);
}

__device__ __forceinline__ void eg_edge(const EgArgs& a, int at, int j, int i, int kind, const double* Sjw, const double* Swi) {
  if (at >= a.cap_edges) return;
  double S[7];
  s3_mul(Sjw, Swi, S);
  a.edge_j[at] = a.kf_vtx[j]; a.edge_i[at] = a.kf_vtx[i]; a.edge_kind[at] = (uint8_t)kind;
  for (int q = 0; q < 7; q++) a.edge_S[7 * (size_t)at + q] = S[q];
}

// The edges of keyframe i in the reference's order: its loop-connection row (:797-821) from place atA, then its parent, its loop edges and
// its covisibility edges (:824-905) from place atB.  *nA, *nB = how many; *ndrop = edges that every other rule admits of which an end has
// no vertex.  EMIT = false only counts.
template <bool EMIT>
__device__ __forceinline__ void eg_walk(const EgArgs& a, int i, int atA, int atB, int* nA, int* nB, int* ndrop) {
  int cA = 0, cB = 0, drop = 0, lo, hi;
  const bool has_vtx = a.kf_vtx[i] >= 0;
  const int t = a.tpos[i];
  if (t >= 0) {
    mt_range(a.link_off, t, a.n_link, &lo, &hi);
    double Swi[7];
    if (EMIT && has_vtx && lo < hi) s3_inverse(a.wB + 7 * (size_t)i, Swi);     // (exp of the block, not the non-corrected Sim3: :799-800)
    long long prev = -1;
    for (;;) {
      const int j = eg_next(a, a.link_kf, lo, hi, &prev);
      if (j < 0) break;
      if (!eg_lc_pass(a, i, j)) continue;
      if (!has_vtx || a.kf_vtx[j] < 0) { drop++; continue; }
      if (EMIT) eg_edge(a, atA + cA, j, i, 0, a.wB + 7 * (size_t)j, Swi);
      cA++;
    }
  }
  if (has_vtx) {
    double Swi[7];
    if (EMIT) s3_inverse(a.wW + 7 * (size_t)i, Swi);
    int par = a.kf_parent[i];
    if (par < 0 || par >= a.nkf) par = -1;
    if (par >= 0) {                                                            // (:836-854)
      if (a.kf_vtx[par] < 0) drop++;
      else { if (EMIT) eg_edge(a, atB + cB, par, i, 1, a.wW + 7 * (size_t)par, Swi); cB++; }
    }
    int llo, lhi;
    mt_range(a.loop_off, i, a.n_loop, &llo, &lhi);
    long long prev = -1;
    for (;;) {                                                                 // (:857-876) std::set<KeyFrame*>: ascending kf_rank
      const int l = eg_next(a, a.loop_edge, llo, lhi, &prev);
      if (l < 0) break;
      if (!(a.kf_id[l] < a.kf_id[i])) continue;
      if (a.kf_vtx[l] < 0) { drop++; continue; }
      if (EMIT) eg_edge(a, atB + cB, l, i, 2, a.wW + 7 * (size_t)l, Swi);
      cB++;
    }
    int clo, chi;
    mt_range(a.child_off, i, a.n_child, &clo, &chi);
    mt_range(a.ord_off, i, a.n_ord, &lo, &hi);
    int nw = 0;
    while (lo + nw < hi && a.ord_w[lo + nw] >= a.min_weight) nw++;
    if (lo + nw == hi) nw = 0;                                                 // (src/KeyFrame.cc:218-235: upper_bound gave end())
    for (int e = lo; e < lo + nw; e++) {                                       // (:879-905)
      const int n = a.ord_kf[e];
      if (!eg_in(a, n) || n == par || eg_holds(a.child_kf, clo, chi, n) || eg_holds(a.loop_edge, llo, lhi, n)) continue;
      if (eg_kf_bad(a, n) || !(a.kf_id[n] < a.kf_id[i])) continue;
      if (eg_linked(a, i, n) || eg_linked(a, n, i)) continue;
      if (a.kf_vtx[n] < 0) { drop++; continue; }
      if (EMIT) eg_edge(a, atB + cB, n, i, 3, a.wW + 7 * (size_t)n, Swi);
      cB++;
    }
  }
  *nA = cA; *nB = cB; *ndrop = drop;
}

__global__ __launch_bounds__(EG_WG) void k_eg_escan(EgArgs a) {
  __shared__ mt_u64 sw[EG_WG / 64];
  const int r = blockIdx.x * EG_WG + threadIdx.x;
  const int i = r < a.nkf ? eg_kf_of_rank(a, r) : -1;
  int nA = 0, nB = 0, drop = 0;
  if (i >= 0) eg_walk<false>(a, i, 0, 0, &nA, &nB, &drop);
  mt_u64 tot;
  const mt_u64 ex = mt_block_excl<EG_WG>(((mt_u64)(uint32_t)nB << 32) | (mt_u64)(uint32_t)nA, sw, &tot);   // (neither sum reaches 2^31)
  if (r < a.nkf) a.escan[r] = ex;
  if (threadIdx.x == 0) a.esums[blockIdx.x] = tot;
  drop = mt_wave_sum(drop);
  if ((threadIdx.x & 63) == 0 && drop) atomicAdd(&a.counts[3], drop);
}

__global__ __launch_bounds__(EG_WG) void k_eg_emit(EgArgs a) {
  const int r = blockIdx.x * EG_WG + threadIdx.x;
  if (r >= a.nkf) return;
  const mt_u64 t = a.esums[a.nb];
  const int totA = (int)(uint32_t)t, totB = (int)(t >> 32);
  if (r == 0) {
    a.counts[1] = totA + totB; a.counts[2] = totA;
    if (totA + totB > a.cap_edges) mt_flag(a.status, EG_ST_CAP_EDGES);
  }
  const int i = eg_kf_of_rank(a, r);
  if (i < 0) return;
  const mt_u64 at = a.escan[r] + a.esums[blockIdx.x];
  int nA, nB, drop;
  eg_walk<true>(a, i, (int)(uint32_t)at, totA + (int)(at >> 32), &nA, &nB, &drop);
}

// workspace sections, each rounded up to 256 bytes; [0, ones) is set to all ones by every call
struct EgWs { size_t inv_kf, gpos, tpos, ones, vscan, vsums, escan, esums, wB, wW, total; int nb; };
static EgWs eg_workspace(int nkf) {
  EgWs w; Carve ws;
  w.nb = (nkf + EG_WG - 1) / EG_WG;
  w.inv_kf = ws.take(4 * (size_t)nkf); w.gpos = ws.take(4 * (size_t)nkf); w.tpos = ws.take(4 * (size_t)nkf);
  w.ones = ws.total;
  w.vscan = ws.take(8 * (size_t)nkf); w.vsums = ws.take(8 * ((size_t)w.nb + 1)); w.escan = ws.take(8 * (size_t)nkf); w.esums = ws.take(8 * ((size_t)w.nb + 1));
  w.wB = ws.take(56 * (size_t)nkf); w.wW = ws.take(56 * (size_t)nkf);
  w.total = ws.total;
  return w;
}

// ---------------------------------------------------------------------------------------------------------- write-back
struct EaArgs {
  int n_vtx, nkf, npts, nobs, n_levels;
  const int32_t* vtx_kf; const double *lie_orig, *lie_opt; double *kf_Tcw, *kf_center, *X; const uint8_t *pt_bad, *pt_done; const int32_t *pt_corr_ref, *pt_ref_kf;
  const int32_t *obs_off, *obs_kf, *ref_level; const float* scale_factors; double* normal; float* min_max; uint8_t* nd_written; uint8_t* pt_moved;
  int32_t* counts; uint32_t* status;
  // workspace: vtx_of[nkf] (set to all ones per call) | Sorig[n_vtx][7] | Sinv[n_vtx][7]
  int32_t* vtx_of; double *Sorig, *Sinv;
};

__global__ __launch_bounds__(EG_WG) void k_ea_stamp(EaArgs a) {
  const int v = blockIdx.x * EG_WG + threadIdx.x;
  if (v >= a.n_vtx) return;
  const int k = a.vtx_kf[v];
  bool fin = true;
  for (int q = 0; q < 7; q++) fin = fin && isfinite(a.lie_orig[7 * (size_t)v + q]) && isfinite(a.lie_opt[7 * (size_t)v + q]);
  if (k < 0 || k >= a.nkf) mt_flag(a.status, EG_ST_KF);
  else if (!fin) mt_flag(a.status, EG_ST_SIM3);                                // (the vertex is absent: its keyframe and its points stay)
  else if (atomicMax(&a.vtx_of[k], v) != -1) mt_flag(a.status, EG_ST_KF);      // (a keyframe listed twice: its last vertex counts)
}

__global__ __launch_bounds__(EG_WG) void k_ea_pose(EaArgs a) {
  const int v = blockIdx.x * EG_WG + threadIdx.x;
  const int k = v < a.n_vtx ? a.vtx_kf[v] : -1;
  const bool own = k >= 0 && k < a.nkf && a.vtx_of[k] == v;
  const uint64_t m = __ballot(own);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts[0], (int)__popcll(m));
  if (!own) return;
  double So[7], Sn[7], Si[7], T[12];
  s3_exp(a.lie_orig + 7 * (size_t)v, So);
  s3_exp(a.lie_opt + 7 * (size_t)v, Sn);                                       // (:918-929) Tiw = [R | t / s]
  s3_inverse(Sn, Si);
  for (int q = 0; q < 7; q++) { a.Sorig[7 * (size_t)v + q] = So[q]; a.Sinv[7 * (size_t)v + q] = Si[q]; }
  s3_to_pose34(Sn, T);
  mt_set_pose(a.kf_Tcw, a.kf_center, k, T);
}

__global__ __launch_bounds__(EG_WG) void k_ea_points(EaArgs a) {
  const int p = blockIdx.x * EG_WG + threadIdx.x;
  int v = -1;
  if (p < a.npts && !(a.pt_bad && a.pt_bad[p])) {                              // (:935-949)
    // both candidates are loaded and one is picked by value (no pointer is selected across the condition: DESIGN.md section 2 says why)
    const int done = a.pt_done ? (int)a.pt_done[p] : 0;
    const int rc = a.pt_done ? a.pt_corr_ref[p] : -1, rr = a.pt_ref_kf[p];
    const int r = done != 0 ? rc : rr;
    if (r < -1 || r >= a.nkf) mt_flag(a.status, EG_ST_KF);
    else if (r >= 0) v = a.vtx_of[r];
  }
  const uint64_t m = __ballot(v >= 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts[1], (int)__popcll(m));
  if (p >= a.npts) return;
  a.pt_moved[p] = v >= 0 ? 1 : 0;
  if (a.nd_written) a.nd_written[p] = 0;
  if (v < 0) return;
  const double P[3] = {a.X[3 * (size_t)p], a.X[3 * (size_t)p + 1], a.X[3 * (size_t)p + 2]};
  double Pc[3], Pw[3];
  s3_act(a.Sorig + 7 * (size_t)v, P, Pc);                                      // (:951-953)
  s3_act(a.Sinv + 7 * (size_t)v, Pc, Pw);
  a.X[3 * (size_t)p] = Pw[0]; a.X[3 * (size_t)p + 1] = Pw[1]; a.X[3 * (size_t)p + 2] = Pw[2];
  if (!a.nd_written) return;
  // UpdateNormalAndDepth (:955): every SetPose precedes the point loop, so every centre is the new one
  int lo, hi;
  if (!mt_range(a.obs_off, p, a.nobs, &lo, &hi)) { mt_flag(a.status, EG_ST_OFFSETS); return; }
  if (lo == hi) return;
  const int r = a.pt_ref_kf[p], lvl = a.ref_level[p];
  if (r < 0 || r >= a.nkf) { if (r != -1) mt_flag(a.status, EG_ST_KF); return; }      // (-1: a point without a reference keyframe gets no normal)
  if (lvl < 0 || lvl >= a.n_levels) { mt_flag(a.status, EG_ST_LEVEL); return; }
  const int res = mt_normal_depth(a.obs_kf, lo, hi, a.nkf, a.kf_center, Pw[0], Pw[1], Pw[2], r, lvl, a.scale_factors, a.n_levels, a.normal + 3 * (size_t)p,
                                  a.min_max + 2 * (size_t)p);
  if (res == MT_ND_KF) mt_flag(a.status, EG_ST_KF);
  if (res == MT_ND_OK) a.nd_written[p] = 1;
}

struct EaWs { size_t vtx_of, Sorig, Sinv, total; };
static EaWs ea_workspace(int nkf, int n_vtx) {
  EaWs w; Carve ws;
  w.vtx_of = ws.take(4 * (size_t)nkf); w.Sorig = ws.take(56 * (size_t)n_vtx); w.Sinv = ws.take(56 * (size_t)n_vtx);
  w.total = ws.total > 0 ? ws.total : 256;
  return w;
}

// kf_id is distinct among the keyframes that are not bad (inserted_edges is keyed by id pairs)
static std::string eg_check_ids(const char* entry, const int32_t* kf_id, const uint8_t* kf_bad, int nkf) {
  std::vector<std::pair<int32_t, int32_t> > ids;
  for (int k = 0; k < nkf; k++) if (!(kf_bad && kf_bad[k])) ids.push_back(std::make_pair(kf_id[k], k));
  std::sort(ids.begin(), ids.end());
  for (size_t q = 1; q < ids.size(); q++)
    if (ids[q].first == ids[q - 1].first) return arg_fail(entry, "kf_id %d is held by keyframes %d and %d, neither bad", ids[q].first, ids[q - 1].second, ids[q].second);
  return {};
}

}  // namespace orbhip

extern "C" {

int orbl_essential_graph_assemble_workspace(int nkf, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && bytes, ORBHIP_EINVAL, "orbl_essential_graph_assemble_workspace: bad argument");
  *bytes = orbhip::eg_workspace(nkf).total;
  return 0;
}

int orbl_essential_graph_assemble_device(int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const int32_t* kf_rank, const double* kf_Tcw, const int32_t* kf_parent,
                                         int n_child, const int32_t* child_off, const int32_t* child_kf, int n_loop, const int32_t* loop_off, const int32_t* loop_kf,
                                         int n_connw, const int32_t* conn_off, const int32_t* conn_kf, const int32_t* conn_w, int n_ord, const int32_t* ord_off,
                                         const int32_t* ord_kf, const int32_t* ord_w, int nconn, const int32_t* conn_group_kf, const double* corrected,
                                         const double* non_corrected, int ntgt, const int32_t* tgt_kf, int n_link, const int32_t* link_off, const int32_t* link_kf,
                                         int loop_keyframe, int cur_keyframe, int min_weight, int cap_vtx, int cap_edges, int32_t* counts, int32_t* vtx_kf, int32_t* kf_vtx,
                                         double* lie7, uint8_t* vtx_fixed, int32_t* edge_j, int32_t* edge_i, double* edge_Sji, uint8_t* edge_kind, uint32_t* status,
                                         void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(nkf >= 1 && n_child >= 0 && n_loop >= 0 && n_connw >= 0 && n_ord >= 0 && nconn >= 0 && ntgt >= 0 && n_link >= 0, ORBHIP_EINVAL,
                 "orbl_essential_graph_assemble: bad count (nkf is >= 1)");
  ORBHIP_REQUIRE(loop_keyframe >= 0 && loop_keyframe < nkf && cur_keyframe >= 0 && cur_keyframe < nkf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: loop_kf or cur_kf out of range");
  ORBHIP_REQUIRE(min_weight >= 1, ORBHIP_EINVAL, "orbl_essential_graph_assemble: min_weight is >= 1");
  ORBHIP_REQUIRE(cap_vtx >= 0 && cap_edges >= 0, ORBHIP_EINVAL, "orbl_essential_graph_assemble: negative capacity");
  ORBHIP_REQUIRE(kf_id && kf_Tcw && kf_parent && child_off && loop_off && conn_off && ord_off && counts && kf_vtx && workspace, ORBHIP_EINVAL,
                 "orbl_essential_graph_assemble: NULL argument");
  ORBHIP_REQUIRE(n_child == 0 || child_kf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL child_kf");
  ORBHIP_REQUIRE(n_loop == 0 || loop_kf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL loop_kf");
  ORBHIP_REQUIRE(n_connw == 0 || (conn_kf && conn_w), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL conn_kf or conn_w");
  ORBHIP_REQUIRE(n_ord == 0 || (ord_kf && ord_w), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL ord_kf or ord_w");
  ORBHIP_REQUIRE(nconn == 0 || (conn_group_kf && corrected && non_corrected), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL group argument");
  ORBHIP_REQUIRE(ntgt == 0 || (tgt_kf && link_off), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL tgt_kf or link_off");
  ORBHIP_REQUIRE(n_link == 0 || link_kf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL link_kf");
  ORBHIP_REQUIRE(cap_vtx == 0 || (vtx_kf && lie7 && vtx_fixed), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL vertex output");
  ORBHIP_REQUIRE(cap_edges == 0 || (edge_j && edge_i && edge_Sji && edge_kind), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL edge output");
  const void* q8[] = {kf_Tcw, corrected, non_corrected, lie7, edge_Sji, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_essential_graph_assemble: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {kf_id, kf_rank, kf_parent, child_off, child_kf, loop_off, loop_kf, conn_off, conn_kf, conn_w, ord_off, ord_kf, ord_w, conn_group_kf, tgt_kf, link_off, link_kf,
                      counts, vtx_kf, kf_vtx, edge_j, edge_i, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_essential_graph_assemble: 32-bit arrays must be 4-byte aligned");
  const EgWs ws = eg_workspace(nkf);
  uint8_t* wb = (uint8_t*)workspace;
  EgArgs A; std::memset(&A, 0, sizeof(A));
  A.nkf = nkf; A.nconn = nconn; A.ntgt = ntgt; A.n_child = n_child; A.n_loop = n_loop; A.n_cw = n_connw; A.n_ord = n_ord; A.n_link = n_link;
  A.loop_kf = loop_keyframe; A.cur_kf = cur_keyframe; A.min_weight = min_weight; A.cap_vtx = cap_vtx; A.cap_edges = cap_edges; A.nb = ws.nb;
  A.kf_id = kf_id; A.kf_bad = kf_bad; A.kf_rank = kf_rank; A.kf_Tcw = kf_Tcw; A.kf_parent = kf_parent; A.child_off = child_off; A.child_kf = child_kf;
  A.loop_off = loop_off; A.loop_edge = loop_kf; A.conn_off = conn_off; A.conn_kf = conn_kf; A.conn_w = conn_w; A.ord_off = ord_off; A.ord_kf = ord_kf; A.ord_w = ord_w;
  A.group_kf = conn_group_kf; A.corrected = corrected; A.non_corrected = non_corrected; A.tgt_kf = tgt_kf; A.link_off = link_off; A.link_kf = link_kf;
  A.counts = counts; A.vtx_kf = vtx_kf; A.kf_vtx = kf_vtx; A.lie7 = lie7; A.vtx_fixed = vtx_fixed; A.edge_j = edge_j; A.edge_i = edge_i; A.edge_S = edge_Sji;
  A.edge_kind = edge_kind; A.status = status;
  A.inv_kf = (int32_t*)(wb + ws.inv_kf); A.gpos = (int32_t*)(wb + ws.gpos); A.tpos = (int32_t*)(wb + ws.tpos);
  A.vscan = (mt_u64*)(wb + ws.vscan); A.vsums = (mt_u64*)(wb + ws.vsums); A.escan = (mt_u64*)(wb + ws.escan); A.esums = (mt_u64*)(wb + ws.esums);
  A.wB = (double*)(wb + ws.wB); A.wW = (double*)(wb + ws.wW);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 16, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0xFF, ws.ones, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(kf_vtx, 0xFF, 4 * (size_t)nkf, st));
  auto grid = [](int n) { return dim3((unsigned)((n + EG_WG - 1) / EG_WG)); };
  const int n_stamp = std::max(std::max(std::max(nkf, nconn), std::max(ntgt, n_child)), std::max(std::max(n_loop, n_connw), std::max(n_ord, n_link)));
  hipLaunchKernelGGL(k_eg_stamp, grid(n_stamp), dim3(EG_WG), 0, st, A);
  hipLaunchKernelGGL(k_eg_vscan, grid(nkf), dim3(EG_WG), 0, st, A);
  hipLaunchKernelGGL(k_mt_scan_sums<mt_u64>, dim3(1), dim3(MT_SUM_WG), 0, st, A.vsums, A.nb);
  hipLaunchKernelGGL(k_eg_vertices, grid(nkf), dim3(EG_WG), 0, st, A);
  hipLaunchKernelGGL(k_eg_escan, grid(nkf), dim3(EG_WG), 0, st, A);
  hipLaunchKernelGGL(k_mt_scan_sums<mt_u64>, dim3(1), dim3(MT_SUM_WG), 0, st, A.esums, A.nb);
  hipLaunchKernelGGL(k_eg_emit, grid(nkf), dim3(EG_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_essential_graph_assemble(int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const int32_t* kf_rank, const double* kf_Tcw, const int32_t* kf_parent,
                                  const int32_t* child_off, const int32_t* child_kf, const int32_t* loop_off, const int32_t* loop_kf, const int32_t* conn_off,
                                  const int32_t* conn_kf, const int32_t* conn_w, const int32_t* ord_off, const int32_t* ord_kf, const int32_t* ord_w, int nconn,
                                  const int32_t* conn_group_kf, const double* corrected, const double* non_corrected, int ntgt, const int32_t* tgt_kf,
                                  const int32_t* link_off, const int32_t* link_kf, int loop_keyframe, int cur_keyframe, int min_weight, int cap_vtx, int cap_edges,
                                  int32_t* counts, int32_t* vtx_kf, int32_t* kf_vtx, double* lie7, uint8_t* vtx_fixed, int32_t* edge_j, int32_t* edge_i,
                                  double* edge_Sji, uint8_t* edge_kind) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(nkf >= 1 && nconn >= 0 && ntgt >= 0, ORBHIP_EINVAL, "orbl_essential_graph_assemble: bad count (nkf is >= 1)");
  ORBHIP_REQUIRE(loop_keyframe >= 0 && loop_keyframe < nkf && cur_keyframe >= 0 && cur_keyframe < nkf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: loop_kf or cur_kf out of range");
  ORBHIP_REQUIRE(min_weight >= 1, ORBHIP_EINVAL, "orbl_essential_graph_assemble: min_weight is >= 1");
  ORBHIP_REQUIRE(cap_vtx >= 0 && cap_edges >= 0, ORBHIP_EINVAL, "orbl_essential_graph_assemble: negative capacity");
  ORBHIP_REQUIRE(kf_id && kf_Tcw && kf_parent && child_off && loop_off && conn_off && ord_off && counts && kf_vtx, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL argument");
  ORBHIP_REQUIRE(nconn == 0 || (conn_group_kf && corrected && non_corrected), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL group argument");
  ORBHIP_REQUIRE(ntgt == 0 || (tgt_kf && link_off), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL tgt_kf or link_off");
  ORBHIP_REQUIRE(cap_vtx == 0 || (vtx_kf && lie7 && vtx_fixed), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL vertex output");
  ORBHIP_REQUIRE(cap_edges == 0 || (edge_j && edge_i && edge_Sji && edge_kind), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL edge output");
  static const char E[] = "orbl_essential_graph_assemble";
  int n_child = 0, n_loop = 0, n_connw = 0, n_ord = 0, n_link = 0;
  ORBHIP_ARG(check_csr(E, "child_off", child_off, nkf, &n_child));
  ORBHIP_ARG(check_csr(E, "loop_off", loop_off, nkf, &n_loop));
  ORBHIP_ARG(check_csr(E, "conn_off", conn_off, nkf, &n_connw));
  ORBHIP_ARG(check_csr(E, "ord_off", ord_off, nkf, &n_ord));
  ORBHIP_ARG(check_csr(E, "link_off", link_off, ntgt, &n_link));
  ORBHIP_REQUIRE(n_child == 0 || child_kf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL child_kf");
  ORBHIP_REQUIRE(n_loop == 0 || loop_kf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL loop_kf");
  ORBHIP_REQUIRE(n_connw == 0 || (conn_kf && conn_w), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL conn_kf or conn_w");
  ORBHIP_REQUIRE(n_ord == 0 || (ord_kf && ord_w), ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL ord_kf or ord_w");
  ORBHIP_REQUIRE(n_link == 0 || link_kf, ORBHIP_EINVAL, "orbl_essential_graph_assemble: NULL link_kf");
  ORBHIP_ARG(check_index(E, "kf_parent", kf_parent, nkf, nkf, true));
  ORBHIP_ARG(check_index(E, "child_kf", child_kf, n_child, nkf));
  ORBHIP_ARG(check_index(E, "loop_kf", loop_kf, n_loop, nkf));
  ORBHIP_ARG(check_index(E, "conn_kf", conn_kf, n_connw, nkf));
  ORBHIP_ARG(check_index(E, "ord_kf", ord_kf, n_ord, nkf));
  ORBHIP_ARG(check_index(E, "link_kf", link_kf, n_link, nkf));
  ORBHIP_ARG(check_listed_once(E, "conn_group_kf", conn_group_kf, nconn, nkf));
  ORBHIP_ARG(check_listed_once(E, "tgt_kf", tgt_kf, ntgt, nkf));
  if (kf_rank) ORBHIP_ARG(check_permutation(E, "kf_rank", kf_rank, nkf));
  ORBHIP_ARG(eg_check_ids(E, kf_id, kf_bad, nkf));
  for (int c = 0; c < nconn; c++)
    for (const double* s : {corrected + 7 * (size_t)c, non_corrected + 7 * (size_t)c})
      ORBHIP_REQUIRE(mc_finite(s, 7) && (s[0] * s[0] + s[1] * s[1]) + (s[2] * s[2] + s[3] * s[3]) > 0.0, ORBHIP_EINVAL,
                     "orbl_essential_graph_assemble: a corrected / non_corrected Sim3 is not finite or its quaternion is zero");
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, nc = (size_t)nconn, nt = (size_t)ntgt, cv = (size_t)cap_vtx, ce = (size_t)cap_edges;
  RoundTrip R(W);
  const HostIn<int32_t> d_id = R.in(kf_id, nk), d_rank = R.in(kf_rank, nk), d_par = R.in(kf_parent, nk), d_coff = R.csr(child_off, nk), d_ckf = R.in(child_kf, (size_t)n_child),
                        d_loff = R.csr(loop_off, nk), d_lkf = R.in(loop_kf, (size_t)n_loop), d_woff = R.csr(conn_off, nk), d_wkf = R.in(conn_kf, (size_t)n_connw),
                        d_ww = R.in(conn_w, (size_t)n_connw), d_ooff = R.csr(ord_off, nk), d_okf = R.in(ord_kf, (size_t)n_ord), d_ow = R.in(ord_w, (size_t)n_ord),
                        d_grp = R.in(conn_group_kf, nc), d_tgt = R.in(tgt_kf, nt), d_koff = R.csr(ntgt ? link_off : nullptr, nt), d_kkf = R.in(link_kf, (size_t)n_link);
  const HostIn<uint8_t> d_bad = R.in(kf_bad, nk);
  const HostIn<double> d_T = R.in(kf_Tcw, 12 * nk), d_cor = R.in(corrected, 7 * nc), d_non = R.in(non_corrected, 7 * nc);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4), o_vkf = R.out<int32_t>(cv), o_kfv = R.out<int32_t>(nk), o_ej = R.out<int32_t>(ce), o_ei = R.out<int32_t>(ce);
  const HostOut<double> o_lie = R.out<double>(7 * cv), o_S = R.out<double>(7 * ce);
  const HostOut<uint8_t> o_fixed = R.out<uint8_t>(cv), o_kind = R.out<uint8_t>(ce);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(eg_workspace(nkf).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_essential_graph_assemble_device(nkf, d_id.dev(), d_bad.dev(), d_rank.dev(), d_T.dev(), d_par.dev(), n_child, d_coff.dev(), d_ckf.dev(), n_loop, d_loff.dev(),
                                                 d_lkf.dev(), n_connw, d_woff.dev(), d_wkf.dev(), d_ww.dev(), n_ord, d_ooff.dev(), d_okf.dev(), d_ow.dev(), nconn, d_grp.dev(),
                                                 d_cor.dev(), d_non.dev(), ntgt, d_tgt.dev(), n_link, d_koff.dev(), d_kkf.dev(), loop_keyframe, cur_keyframe, min_weight, cap_vtx,
                                                 cap_edges, o_counts.dev(), o_vkf.dev(), o_kfv.dev(), o_lie.dev(), o_fixed.dev(), o_ej.dev(), o_ei.dev(), o_S.dev(), o_kind.dev(),
                                                 o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 4);
  const size_t nv = (size_t)o_counts[0], ne = (size_t)o_counts[1];
  if (nv > cv || ne > ce) {
    set_error("orbl_essential_graph_assemble: wanted %d vertices, %d edges; capacities %d, %d", o_counts[0], o_counts[1], cap_vtx, cap_edges);
    return ORBHIP_ECAP;
  }
  // the lists up to their counts: what lies behind them in the caller's arrays is not touched
  R.copy_out(o_vkf, vtx_kf, nv); R.copy_out(o_lie, lie7, 7 * nv); R.copy_out(o_fixed, vtx_fixed, nv); R.copy_out(o_kfv, kf_vtx, nk);
  R.copy_out(o_ej, edge_j, ne); R.copy_out(o_ei, edge_i, ne); R.copy_out(o_S, edge_Sji, 7 * ne); R.copy_out(o_kind, edge_kind, ne);
  return 0;
}

int orbl_essential_graph_apply_workspace(int nkf, int n_vtx, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && n_vtx >= 0 && bytes, ORBHIP_EINVAL, "orbl_essential_graph_apply_workspace: bad argument");
  *bytes = orbhip::ea_workspace(nkf, n_vtx).total;
  return 0;
}

int orbl_essential_graph_apply_device(int n_vtx, const int32_t* vtx_kf, const double* lie_orig, const double* lie_opt, int nkf, double* kf_Tcw, double* kf_center, int npts,
                                      double* X, const uint8_t* pt_bad, const uint8_t* pt_done, const int32_t* pt_corr_ref, const int32_t* pt_ref_kf, int nobs,
                                      const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, double* normal,
                                      float* min_max, uint8_t* nd_written, uint8_t* pt_moved, int32_t* counts, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(n_vtx >= 0 && nkf >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_essential_graph_apply: negative count");
  ORBHIP_REQUIRE(counts && workspace, ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL counts or workspace");
  ORBHIP_REQUIRE(n_vtx == 0 || (vtx_kf && lie_orig && lie_opt && kf_Tcw), ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL vertex argument");
  ORBHIP_REQUIRE(npts == 0 || (X && pt_ref_kf && pt_moved), ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL point argument");
  ORBHIP_REQUIRE(!pt_done || pt_corr_ref, ORBHIP_EINVAL, "orbl_essential_graph_apply: pt_done needs pt_corr_ref");
  const bool any_nd = obs_off || obs_kf || ref_level || scale_factors || normal || min_max || nd_written;
  const bool nd = obs_off && ref_level && scale_factors && normal && min_max && nd_written && (nobs == 0 || obs_kf);
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_essential_graph_apply: the normal / depth arguments are given as a set");
  ORBHIP_REQUIRE(!nd || nkf == 0 || kf_center, ORBHIP_EINVAL, "orbl_essential_graph_apply: the normals need kf_center");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_essential_graph_apply: n_levels out of range");
  const void* q8[] = {lie_orig, lie_opt, kf_Tcw, kf_center, X, normal, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_essential_graph_apply: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {vtx_kf, pt_corr_ref, pt_ref_kf, obs_off, obs_kf, ref_level, scale_factors, min_max, counts, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_essential_graph_apply: 32-bit arrays must be 4-byte aligned");
  const EaWs ws = ea_workspace(nkf, n_vtx);
  uint8_t* wb = (uint8_t*)workspace;
  EaArgs A; std::memset(&A, 0, sizeof(A));
  A.n_vtx = n_vtx; A.nkf = nkf; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels;
  A.vtx_kf = vtx_kf; A.lie_orig = lie_orig; A.lie_opt = lie_opt; A.kf_Tcw = kf_Tcw; A.kf_center = kf_center; A.X = X; A.pt_bad = pt_bad; A.pt_done = pt_done;
  A.pt_corr_ref = pt_corr_ref; A.pt_ref_kf = pt_ref_kf; A.pt_moved = pt_moved; A.counts = counts; A.status = status;
  if (nd) { A.obs_off = obs_off; A.obs_kf = obs_kf; A.ref_level = ref_level; A.scale_factors = scale_factors; A.normal = normal; A.min_max = min_max; A.nd_written = nd_written; }
  A.vtx_of = (int32_t*)(wb + ws.vtx_of); A.Sorig = (double*)(wb + ws.Sorig); A.Sinv = (double*)(wb + ws.Sinv);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 8, st));
  if (nkf > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.vtx_of, 0xFF, 4 * (size_t)nkf, st));
  auto grid = [](int n) { return dim3((unsigned)((n + EG_WG - 1) / EG_WG)); };
  if (n_vtx > 0 && nkf > 0) {
    hipLaunchKernelGGL(k_ea_stamp, grid(n_vtx), dim3(EG_WG), 0, st, A);
    hipLaunchKernelGGL(k_ea_pose, grid(n_vtx), dim3(EG_WG), 0, st, A);
  }
  if (npts > 0) hipLaunchKernelGGL(k_ea_points, grid(npts), dim3(EG_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_essential_graph_apply(int n_vtx, const int32_t* vtx_kf, const double* lie_orig, const double* lie_opt, int nkf, double* kf_Tcw, double* kf_center, int npts, double* X,
                               const uint8_t* pt_bad, const uint8_t* pt_done, const int32_t* pt_corr_ref, const int32_t* pt_ref_kf, const int32_t* obs_off,
                               const int32_t* obs_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, double* normal, float* min_max,
                               uint8_t* nd_written, uint8_t* pt_moved, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(n_vtx >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_essential_graph_apply: negative count");
  ORBHIP_REQUIRE(counts, ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL counts");
  ORBHIP_REQUIRE(n_vtx == 0 || (vtx_kf && lie_orig && lie_opt && kf_Tcw), ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL vertex argument");
  ORBHIP_REQUIRE(npts == 0 || (X && pt_ref_kf && pt_moved), ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL point argument");
  ORBHIP_REQUIRE(!pt_done || pt_corr_ref, ORBHIP_EINVAL, "orbl_essential_graph_apply: pt_done needs pt_corr_ref");
  const bool any_nd = obs_off || obs_kf || ref_level || scale_factors || normal || min_max || nd_written;
  const bool nd = obs_off && ref_level && scale_factors && normal && min_max && nd_written;
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_essential_graph_apply: the normal / depth arguments are given as a set");
  ORBHIP_REQUIRE(!nd || nkf == 0 || kf_center, ORBHIP_EINVAL, "orbl_essential_graph_apply: the normals need kf_center");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_essential_graph_apply: n_levels out of range");
  static const char E[] = "orbl_essential_graph_apply";
  ORBHIP_ARG(check_listed_once(E, "vtx_kf", vtx_kf, n_vtx, nkf));
  ORBHIP_REQUIRE(n_vtx == 0 || (mc_finite(lie_orig, 7 * (size_t)n_vtx) && mc_finite(lie_opt, 7 * (size_t)n_vtx)), ORBHIP_EINVAL, "orbl_essential_graph_apply: a tangent is not finite");
  const auto alive = [&](int p) { return !(pt_bad && pt_bad[p]); };
  ORBHIP_ARG(check_index_if(E, "pt_ref_kf", pt_ref_kf, npts, nkf, [&](int p) { return alive(p) && !(pt_done && pt_done[p]) && pt_ref_kf[p] != -1; }));
  if (pt_done)                                                        // (check_index_if reads the entry before it asks: pt_corr_ref may be NULL without pt_done)
    ORBHIP_ARG(check_index_if(E, "pt_corr_ref", pt_corr_ref, npts, nkf, [&](int p) { return alive(p) && pt_done[p] && pt_corr_ref[p] != -1; }));
  int nobs = 0;
  if (nd) {
    ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
    ORBHIP_REQUIRE(nobs == 0 || obs_kf, ORBHIP_EINVAL, "orbl_essential_graph_apply: NULL obs_kf");
    ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
    const auto read = [&](int p) { return obs_off[p] != obs_off[p + 1] && alive(p); };          // (no normal: neither is read)
    ORBHIP_ARG(check_index_if(E, "pt_ref_kf", pt_ref_kf, npts, nkf, [&](int p) { return read(p) && pt_ref_kf[p] != -1; }));
    ORBHIP_ARG(check_index_if(E, "ref_level", ref_level, npts, n_levels, read));
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts, nv = (size_t)n_vtx;
  const bool run_nd = nd && npts > 0;                               // (without points the device entry takes the normal / depth set as absent)
  RoundTrip R(W);
  const HostOut<double> t_Tcw = R.inout(kf_Tcw, 12 * nk), t_center = R.inout(kf_center, 3 * nk), t_X = R.inout(X, 3 * np);
  const HostIn<int32_t> d_vkf = R.in(vtx_kf, nv), d_cref = R.in(pt_corr_ref, np), d_ref = R.in(pt_ref_kf, np), d_ooff = R.csr(run_nd ? obs_off : nullptr, np),
                        d_okf = R.in(run_nd ? obs_kf : nullptr, (size_t)nobs), d_lvl = R.in(run_nd ? ref_level : nullptr, np);
  const HostIn<double> d_lo = R.in(lie_orig, 7 * nv), d_ln = R.in(lie_opt, 7 * nv);
  const HostIn<uint8_t> d_bad = R.in(pt_bad, np), d_done = R.in(pt_done, np);
  const HostIn<float> d_sf = R.in(run_nd ? scale_factors : nullptr, (size_t)n_levels);
  const HostOut<int32_t> o_counts = R.out<int32_t>(2);
  const HostOut<uint8_t> o_moved = R.out<uint8_t>(np), o_wrote = R.out<uint8_t>(np, run_nd);
  const HostOut<double> o_normal = R.out<double>(3 * np, run_nd);
  const HostOut<float> o_mm = R.out<float>(2 * np, run_nd);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(ea_workspace(nkf, n_vtx).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_essential_graph_apply_device(n_vtx, d_vkf.dev(), d_lo.dev(), d_ln.dev(), nkf, t_Tcw.dev(), t_center.dev(), npts, t_X.dev(), d_bad.dev(), d_done.dev(),
                                              d_done.dev() ? d_cref.dev() : nullptr, d_ref.dev(), nobs, d_ooff.dev(), d_okf.dev(), d_lvl.dev(), d_sf.dev(), n_levels,
                                              o_normal.dev(), o_mm.dev(), o_wrote.dev(), o_moved.dev(), o_counts.dev(), o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 2);
  R.copy_out(t_Tcw, kf_Tcw, 12 * nk); R.copy_out(t_center, kf_center, 3 * nk); R.copy_out(t_X, X, 3 * np);
  R.copy_out(o_moved, pt_moved, np);
  if (run_nd) {
    R.copy_out(o_wrote, nd_written, np);
    for (size_t p = 0; p < np; p++)
      if (o_wrote[p]) { std::copy_n(&o_normal[3 * p], 3, normal + 3 * p); std::copy_n(&o_mm[2 * p], 2, min_max + 2 * p); }      // (rows of other points are not touched)
  }
  return 0;
}

}  // extern "C"
