// orb_mapcorrect.inc -- the two steps of a loop closure that move the map: LoopClosing::CorrectLoop's pose / point correction
// (src/LoopClosing.cc:437-523, orbl_correct_loop*) and the write-back of the global bundle adjustment (:681-739,
// orbl_propagate_global_ba*).  Textually included by orb_localmap.hip.  FP64 throughout, no fused multiply-add (-ffp-contract=off);
// every sum is taken in the order written here (DESIGN.md section 2, "CorrectLoop and the global-BA write-back").
//
// Both loops are sequential in the reference; the kernels use their closed forms, in which no workgroup waits for another:
//   correct_loop   the keyframe that moves a point is the one of lowest conn_rank among those that list it (a 64-bit atomicMin of
//                  (rank << 32 | list position) per slot: order-free); a point's normal sees the NEW centre of exactly the group keyframes
//                  of lower rank than its owner, because SetPose follows a keyframe's own points.
//     k_ml_init    one lane per connected keyframe / point: the checks of the device form, kpos[k] = where the list names keyframe k
//     k_ml_pose    one lane per connected keyframe: both Sim3, the inverse of the corrected one, the new pose and centre (to the workspace:
//                  the tables still hold the values at entry, which the other lanes and the point kernel read)
//     k_ml_slots   one lane per slot, twice: the owner; then whether a second keyframe lists the point
//     k_ml_points  one lane per point: the new position, the normal / depth walk (mt_normal_depth) with the centre rule above
//                  (both centres are loaded and one is picked by value: DESIGN.md section 2 says why)
//     k_ml_store   one lane per connected keyframe: the new pose and centre into the tables
//   propagate_global_ba   a keyframe's matrix needs its parent's, so k_gb_walk is ONE workgroup that advances one tree level per round
//                  (two __syncthreads: look at the parents, then write) until a round changes nothing; what is left is a cycle.
//     k_gb_origins one lane per origin: state[k] = done;  k_gb_init  one lane per keyframe: dead (no usable parent) or left open
//     k_gb_walk    the rounds; gba[k] = (Tcw[k] o Twc[parent]) o gba[parent] for a reached keyframe outside the BA, operands at entry values
//     k_gb_apply   one lane per keyframe: bef = Tcw, Tcw = gba, the centre, the flags
//     k_gb_points  one lane per point
// Outputs are written with vector stores only, each element by the one lane that owns it.
#include "orb_maptable.h"
#include "sim3_math.h"

namespace orbhip {

#define MC_WG 256
#define MC_CHAIN_WG 1024          /* k_gb_walk: one workgroup */
#define ML_ST_OFFSETS 1u          /* *status bits of orbl_correct_loop_device */
#define ML_ST_KF 2u
#define ML_ST_PT 4u
#define ML_ST_RANK 8u
#define ML_ST_LEVEL 16u
#define ML_ST_SCW 32u
#define GB_ST_KF 1u               /* *status bits of orbl_propagate_global_ba_device */
#define GB_ST_CYCLE 2u
#define GB_ST_STALE 4u
#define MC_NONE 0xFFFFFFFFFFFFFFFFull

// ---------------------------------------------------------------------------------------------------------- CorrectLoop
struct MlArgs {
  int nkf, nconn, nslots, npts, nobs, n_levels;
  double* kf_Tcw; double* kf_center; const int32_t* conn_kf; const int32_t* conn_rank; const double* Scw; const int32_t* slot_off; const int32_t* slot_pt;
  double* X; const uint8_t* pt_bad; const uint8_t* pt_done; const int32_t* obs_off; const int32_t* obs_kf; const int32_t* ref_kf; const int32_t* ref_level;
  const float* scale_factors;
  double *corrected, *non_corrected; int32_t* pt_owner; double* normal; float* min_max; uint8_t* nd_written; int32_t* counts; uint32_t* status;
  // workspace: kpos[nkf] (set to -1 per call) | rhit[nconn] (cleared per call) | cval[nconn] | own[npts] (set to all ones per call) |
  // contested[npts] (cleared per call) | cinv[nconn][7] | newT[nconn][12] | newC[nconn][3]
  int32_t *kpos, *rhit, *cval; unsigned long long* own; uint8_t* contested; double *cinv, *newT, *newC;
};

__device__ __forceinline__ uint32_t ml_rank(const MlArgs& a, int c) { return (uint32_t)(a.conn_rank ? a.conn_rank[c] : c); }
__device__ __forceinline__ bool ml_takes_part(const MlArgs& a, int p) { return !(a.pt_bad && a.pt_bad[p]) && !(a.pt_done && a.pt_done[p]); }

__global__ __launch_bounds__(MC_WG) void k_ml_init(MlArgs a) {
  const int i = blockIdx.x * MC_WG + threadIdx.x;
  int lo, hi;
  if (i < a.nconn) {
    if (!mt_range(a.slot_off, i, a.nslots, &lo, &hi)) mt_flag(a.status, ML_ST_OFFSETS);
    const int k = a.conn_kf[i];
    if (k < 0 || k >= a.nkf) mt_flag(a.status, ML_ST_KF);
    else if (atomicMax(&a.kpos[k], i) != -1) mt_flag(a.status, ML_ST_KF);            // (a keyframe listed twice: its last instance counts)
    if (a.conn_rank) {
      const int r = a.conn_rank[i];
      if (r < 0 || r >= a.nconn) mt_flag(a.status, ML_ST_RANK);
      else if (atomicAdd(&a.rhit[r], 1) != 0) mt_flag(a.status, ML_ST_RANK);          // (not a permutation)
    }
  }
  if (i < a.npts && a.obs_off && !mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, ML_ST_OFFSETS);
  if (i == 0) {
    bool fin = true;
    for (int q = 0; q < 7; q++) fin = fin && isfinite(a.Scw[q]);
    if (!fin || !((a.Scw[0] * a.Scw[0] + a.Scw[1] * a.Scw[1]) + (a.Scw[2] * a.Scw[2] + a.Scw[3] * a.Scw[3]) > 0.0)) mt_flag(a.status, ML_ST_SCW);
  }
}

__global__ __launch_bounds__(MC_WG) void k_ml_pose(MlArgs a) {
  const int c = blockIdx.x * MC_WG + threadIdx.x;
  if (c >= a.nconn) return;
  const int last = a.nconn - 1, cur = a.conn_kf[last], k = a.conn_kf[c];
  const bool cur_ok = cur >= 0 && cur < a.nkf;                                 // (the current keyframe is the last entry, so it is its own last instance)
  const bool ok = cur_ok && k >= 0 && k < a.nkf && a.kpos[k] == c;
  a.cval[c] = ok;
  double* Sn = a.non_corrected + 7 * (size_t)c;
  double* Sc = a.corrected + 7 * (size_t)c;
  if (!ok) { for (int q = 0; q < 7; q++) { Sn[q] = 0.0; Sc[q] = 0.0; } return; }
  double Tiw[12], S[7];
  for (int q = 0; q < 12; q++) Tiw[q] = a.kf_Tcw[12 * (size_t)k + q];
  mc_se3_as_sim3(Tiw, S);                                                     // (:464-468)
  for (int q = 0; q < 7; q++) Sn[q] = S[q];
  double C[7];
  if (c == last) { for (int q = 0; q < 7; q++) C[q] = a.Scw[q]; }              // (:438)
  else {                                                                       // (:454-461)
    double Tcw[12], Twc[12], Tic[12], Sic[7];
    for (int q = 0; q < 12; q++) Tcw[q] = a.kf_Tcw[12 * (size_t)cur + q];
    mc_pose_inverse(Tcw, Twc);
    mc_affine_mul(Tiw, Twc, Tic);
    mc_se3_as_sim3(Tic, Sic);
    s3_mul(Sic, a.Scw, C);
  }
  for (int q = 0; q < 7; q++) Sc[q] = C[q];
  double Ci[7], T[12];
  s3_inverse(C, Ci);                                                          // (:479)
  for (int q = 0; q < 7; q++) a.cinv[7 * (size_t)c + q] = Ci[q];
  s3_to_pose34(C, T);                                                         // (:508-516)
  mt_set_pose(a.newT, a.newC, c, T);
}

// the connected keyframe that holds slot s, or -1
__device__ __forceinline__ int ml_row_of(const MlArgs& a, int s) {
  int b = 0, t = a.nconn;
  while (b < t) { const int m = (b + t) >> 1; if (a.slot_off[m] <= s) b = m + 1; else t = m; }
  const int c = b - 1;
  int l, h;
  if (c < 0 || !mt_range(a.slot_off, c, a.nslots, &l, &h) || s < l || s >= h) return -1;
  return c;
}

template <int PASS>
__global__ __launch_bounds__(MC_WG) void k_ml_slots(MlArgs a) {
  const int s = blockIdx.x * MC_WG + threadIdx.x;
  if (s >= a.nslots) return;
  const int c = ml_row_of(a, s);
  if (c < 0 || !a.cval[c]) return;
  const int p = a.slot_pt[s];
  if (p < -1 || p >= a.npts) { if (PASS == 0) mt_flag(a.status, ML_ST_PT); return; }
  if (p < 0 || !ml_takes_part(a, p)) return;                                   // (:485-493)
  if (PASS == 0) atomicMin(&a.own[p], ((unsigned long long)ml_rank(a, c) << 32) | (uint32_t)c);
  else if ((uint32_t)a.own[p] != (uint32_t)c) a.contested[p] = 1;              // (every writer stores the same byte)
}

__global__ __launch_bounds__(MC_WG) void k_ml_points(MlArgs a) {
  const int p = blockIdx.x * MC_WG + threadIdx.x;
  const unsigned long long key = p < a.npts ? a.own[p] : MC_NONE;
  const bool moved = key != MC_NONE;
  const uint64_t m_moved = __ballot(moved), m_cont = __ballot(moved && a.contested[p]);
  if ((threadIdx.x & 63) == 0) {
    if (m_moved) atomicAdd(&a.counts[0], (int)__popcll(m_moved));
    if (m_cont) atomicAdd(&a.counts[1], (int)__popcll(m_cont));
  }
  if (p >= a.npts) return;
  if (!moved) { a.pt_owner[p] = -1; if (a.nd_written) a.nd_written[p] = 0; return; }
  const int c = (int)(uint32_t)key;
  const uint32_t orank = (uint32_t)(key >> 32);
  a.pt_owner[p] = a.conn_kf[c];
  double P[3] = {a.X[3 * (size_t)p], a.X[3 * (size_t)p + 1], a.X[3 * (size_t)p + 2]}, Pc[3], Pw[3];
  s3_act(a.non_corrected + 7 * (size_t)c, P, Pc);                              // (:498)
  s3_act(a.cinv + 7 * (size_t)c, Pc, Pw);
  a.X[3 * (size_t)p] = Pw[0]; a.X[3 * (size_t)p + 1] = Pw[1]; a.X[3 * (size_t)p + 2] = Pw[2];
  if (!a.nd_written) return;
  // UpdateNormalAndDepth (:503); a group keyframe of lower rank than the owner has had its SetPose (:519)
  uint8_t wrote = 0;
  int lo, hi;
  const bool live = mt_range(a.obs_off, p, a.nobs, &lo, &hi) && lo < hi;
  const int r = live ? a.ref_kf[p] : -1, lvl = live ? a.ref_level[p] : -1;
  if (live && (r < 0 || r >= a.nkf)) mt_flag(a.status, ML_ST_KF);
  if (live && (lvl < 0 || lvl >= a.n_levels)) mt_flag(a.status, ML_ST_LEVEL);
  if (r >= 0 && r < a.nkf && lvl >= 0 && lvl < a.n_levels) {
    const auto centre = [&](int k) {
      const int kc = a.kpos[k];
      // both centres are loaded and one is picked by value (no pointer is selected across the three-part condition)
      const int kcs = kc >= 0 ? kc : 0;
      const bool use_new = kc >= 0 && a.cval[kcs] != 0 && ml_rank(a, kcs) < orank;
      const double* cn = a.newC + 3 * (size_t)kcs;
      const double* co = a.kf_center + 3 * (size_t)k;
      const double n0 = cn[0], n1 = cn[1], n2 = cn[2], o0 = co[0], o1 = co[1], o2 = co[2];
      return make_double3(use_new ? n0 : o0, use_new ? n1 : o1, use_new ? n2 : o2);
    };
    const int res = mt_normal_depth(a.obs_kf, lo, hi, a.nkf, Pw[0], Pw[1], Pw[2], r, a.scale_factors, a.n_levels, a.normal + 3 * (size_t)p, a.min_max + 2 * (size_t)p,
                                    [](int) { return true; }, centre, [&](int) { return lvl; });
    if (res == MT_ND_KF) mt_flag(a.status, ML_ST_KF);
    wrote = res == MT_ND_OK;
  }
  a.nd_written[p] = wrote;
}

__global__ __launch_bounds__(MC_WG) void k_ml_store(MlArgs a) {
  const int c = blockIdx.x * MC_WG + threadIdx.x;
  if (c >= a.nconn || !a.cval[c]) return;
  const int k = a.conn_kf[c];
  for (int q = 0; q < 12; q++) a.kf_Tcw[12 * (size_t)k + q] = a.newT[12 * (size_t)c + q];
  if (a.kf_center) for (int q = 0; q < 3; q++) a.kf_center[3 * (size_t)k + q] = a.newC[3 * (size_t)c + q];
}

// workspace sections, each rounded up to 256 bytes; [0, cleared) is zeroed, kpos and own are set to all ones by every call
struct MlWs { size_t rhit, contested, cleared, kpos, own, cval, cinv, newT, newC, total; };
static MlWs ml_workspace(int nkf, int nconn, int npts) {
  MlWs w; Carve ws;
  w.rhit = ws.take(4 * (size_t)nconn); w.contested = ws.take((size_t)npts);
  w.cleared = ws.total;
  w.kpos = ws.take(4 * (size_t)nkf); w.own = ws.take(8 * (size_t)npts);
  w.cval = ws.take(4 * (size_t)nconn); w.cinv = ws.take(56 * (size_t)nconn); w.newT = ws.take(96 * (size_t)nconn); w.newC = ws.take(24 * (size_t)nconn);
  w.total = ws.total;
  return w;
}

// ---------------------------------------------------------------------------------------------------------- global BA write-back
struct GbArgs {
  int nkf, n_origin, npts;
  double* kf_Tcw; double* kf_gba; uint8_t* kf_in_gba; const int32_t* kf_parent; const int32_t* origin_kf; double* kf_center;
  double* X; const uint8_t* pt_bad; const uint8_t* pt_in_gba; const double* pt_gba_X; const int32_t* pt_ref_kf;
  double* kf_bef; uint8_t* kf_reached; uint8_t* pt_moved; int32_t* counts; uint32_t* status;
  uint8_t* state;                 // workspace: state[nkf] (cleared per call)
};
#define GB_OPEN 0                 /* not settled yet */
#define GB_DONE 1                 /* reached, its global_BA_Tcw_ is final */
#define GB_DEAD 2                 /* its parent chain does not end in an origin */
#define GB_READY_DONE 3           /* open, the parent was settled before this round: finished after the barrier */
#define GB_READY_DEAD 4

__global__ __launch_bounds__(MC_WG) void k_gb_origins(GbArgs a) {
  const int i = blockIdx.x * MC_WG + threadIdx.x;
  if (i >= a.n_origin) return;
  const int k = a.origin_kf[i];
  if (k < 0 || k >= a.nkf) mt_flag(a.status, GB_ST_KF);
  else a.state[k] = GB_DONE;                                                   // (every writer stores the same byte)
}

__global__ __launch_bounds__(MC_WG) void k_gb_init(GbArgs a) {
  const int k = blockIdx.x * MC_WG + threadIdx.x;
  if (k >= a.nkf || a.state[k] == GB_DONE) return;
  const int par = a.kf_parent[k];
  if (par < -1 || par >= a.nkf) mt_flag(a.status, GB_ST_KF);
  if (par == k) mt_flag(a.status, GB_ST_CYCLE);
  if (par < 0 || par >= a.nkf || par == k) a.state[k] = GB_DEAD;
}

// ONE workgroup.  A round settles every open keyframe whose parent was settled in an earlier round, so a round is one tree level and
// the parent's matrix is always a value stored before the last barrier.  The rounds end when one marks nothing: what is still open
// then hangs on a cycle.
__global__ __launch_bounds__(MC_CHAIN_WG) void k_gb_walk(GbArgs a) {
  const int tid = threadIdx.x;
  for (;;) {
    int marked = 0;
    for (int k = tid; k < a.nkf; k += MC_CHAIN_WG) {
      if (a.state[k] != GB_OPEN) continue;
      const uint8_t ps = a.state[a.kf_parent[k]];                              // (another lane may mark the parent READY meanwhile: as good as open)
      if (ps == GB_DONE) { a.state[k] = GB_READY_DONE; marked = 1; }
      else if (ps == GB_DEAD) { a.state[k] = GB_READY_DEAD; marked = 1; }
    }
    if (!__syncthreads_or(marked)) break;                                      // (workgroup-uniform)
    for (int k = tid; k < a.nkf; k += MC_CHAIN_WG) {
      const uint8_t s = a.state[k];
      if (s == GB_READY_DEAD) a.state[k] = GB_DEAD;
      if (s != GB_READY_DONE) continue;
      if (!a.kf_in_gba[k]) {                                                   // (:691-696, operands at their values at entry)
        const int par = a.kf_parent[k];
        double Tc[12], Tp[12], Twc[12], Tcp[12], G[12], Gp[12];
        for (int q = 0; q < 12; q++) { Tc[q] = a.kf_Tcw[12 * (size_t)k + q]; Tp[q] = a.kf_Tcw[12 * (size_t)par + q]; Gp[q] = a.kf_gba[12 * (size_t)par + q]; }
        mc_pose_inverse(Tp, Twc);
        mc_affine_mul(Tc, Twc, Tcp);
        mc_affine_mul(Tcp, Gp, G);
        for (int q = 0; q < 12; q++) a.kf_gba[12 * (size_t)k + q] = G[q];
      }
      a.state[k] = GB_DONE;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(MC_WG) void k_gb_apply(GbArgs a) {
  const int k = blockIdx.x * MC_WG + threadIdx.x;
  const uint8_t st = k < a.nkf ? a.state[k] : GB_DEAD;
  const bool reached = st == GB_DONE, prop = reached && !a.kf_in_gba[k];
  const uint64_t m_r = __ballot(reached), m_p = __ballot(prop);
  if ((threadIdx.x & 63) == 0) {
    if (m_r) atomicAdd(&a.counts[0], (int)__popcll(m_r));
    if (m_p) atomicAdd(&a.counts[1], (int)__popcll(m_p));
  }
  if (k >= a.nkf) return;
  if (st == GB_OPEN) mt_flag(a.status, GB_ST_CYCLE);
  a.kf_reached[k] = reached;
  if (!reached) return;
  double T[12];
  for (int q = 0; q < 12; q++) { a.kf_bef[12 * (size_t)k + q] = a.kf_Tcw[12 * (size_t)k + q]; T[q] = a.kf_gba[12 * (size_t)k + q]; }      // (:700-701)
  mt_set_pose(a.kf_Tcw, a.kf_center, k, T);
  if (prop) a.kf_in_gba[k] = 1;
}

__global__ __launch_bounds__(MC_WG) void k_gb_points(GbArgs a) {
  const int p = blockIdx.x * MC_WG + threadIdx.x;
  int kind = 0; bool stale = false;
  int r = -1;
  if (p < a.npts && !(a.pt_bad && a.pt_bad[p])) {                              // (:711)
    if (a.pt_in_gba && a.pt_in_gba[p]) kind = 1;                               // (:713-715)
    else {
      r = a.pt_ref_kf[p];
      if (r < 0 || r >= a.nkf) mt_flag(a.status, GB_ST_KF);
      else if (a.kf_reached[r]) kind = 2;
      else stale = a.kf_in_gba[r] != 0;      // (flagged but not walked: the reference would read a stale global_BA_Bef_Tcw_; here the point stays)
    }
  }
  const uint64_t m_m = __ballot(kind != 0), m_s = __ballot(stale);
  if ((threadIdx.x & 63) == 0) {
    if (m_m) atomicAdd(&a.counts[2], (int)__popcll(m_m));
    if (m_s) { atomicAdd(&a.counts[3], (int)__popcll(m_s)); mt_flag(a.status, GB_ST_STALE); }
  }
  if (p >= a.npts) return;
  a.pt_moved[p] = (uint8_t)kind;
  double* x = a.X + 3 * (size_t)p;
  if (kind == 1) { for (int q = 0; q < 3; q++) x[q] = a.pt_gba_X[3 * (size_t)p + q]; }
  else if (kind == 2) {                                                        // (:725-737)
    double Tb[12], Tn[12], Twc[12], P[3] = {x[0], x[1], x[2]}, Xc[3], Xw[3];
    for (int q = 0; q < 12; q++) { Tb[q] = a.kf_bef[12 * (size_t)r + q]; Tn[q] = a.kf_Tcw[12 * (size_t)r + q]; }
    mc_apply34(Tb, P, Xc);
    mc_pose_inverse(Tn, Twc);
    mc_apply34(Twc, Xc, Xw);
    x[0] = Xw[0]; x[1] = Xw[1]; x[2] = Xw[2];
  }
}

static size_t gb_workspace_bytes(int nkf) { Carve ws; ws.take((size_t)nkf); return ws.total > 0 ? ws.total : 256; }

static bool mc_finite(const double* v, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

}  // namespace orbhip

extern "C" {

int orbl_correct_loop_workspace(int nkf, int nconn, int npts, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && nconn >= 0 && npts >= 0 && bytes, ORBHIP_EINVAL, "orbl_correct_loop_workspace: bad argument");
  *bytes = orbhip::ml_workspace(nkf, nconn, npts).total;
  return 0;
}

int orbl_correct_loop_device(int nkf, double* kf_Tcw, double* kf_center, int nconn, const int32_t* conn_kf, const int32_t* conn_rank, const double* Scw, int nslots,
                             const int32_t* slot_off, const int32_t* slot_pt, int npts, double* X, const uint8_t* pt_bad, const uint8_t* pt_done, int nobs,
                             const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels,
                             double* corrected, double* non_corrected, int32_t* pt_owner, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts,
                             uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(nkf >= 1 && nconn >= 1 && nslots >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_correct_loop: bad count (nkf and nconn are >= 1)");
  ORBHIP_REQUIRE(kf_Tcw && conn_kf && Scw && slot_off && corrected && non_corrected && counts && workspace, ORBHIP_EINVAL, "orbl_correct_loop: NULL argument");
  ORBHIP_REQUIRE(nslots == 0 || slot_pt, ORBHIP_EINVAL, "orbl_correct_loop: NULL slot_pt");
  ORBHIP_REQUIRE(npts == 0 || (X && pt_owner), ORBHIP_EINVAL, "orbl_correct_loop: NULL X or pt_owner");
  const bool any_nd = obs_off || obs_kf || ref_kf || ref_level || scale_factors || normal || min_max || nd_written;
  const bool nd = obs_off && ref_kf && ref_level && scale_factors && normal && min_max && nd_written && (nobs == 0 || obs_kf);
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_correct_loop: the normal / depth arguments are given as a set");
  ORBHIP_REQUIRE(!nd || kf_center, ORBHIP_EINVAL, "orbl_correct_loop: the normals need kf_center");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_correct_loop: n_levels out of range");
  const void* q8[] = {kf_Tcw, kf_center, Scw, X, corrected, non_corrected, normal, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_correct_loop: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {conn_kf, conn_rank, slot_off, slot_pt, obs_off, obs_kf, ref_kf, ref_level, scale_factors, pt_owner, min_max, counts, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_correct_loop: 32-bit arrays must be 4-byte aligned");
  const MlWs ws = ml_workspace(nkf, nconn, npts);
  uint8_t* wb = (uint8_t*)workspace;
  MlArgs A; std::memset(&A, 0, sizeof(A));
  A.nkf = nkf; A.nconn = nconn; A.nslots = nslots; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels;
  A.kf_Tcw = kf_Tcw; A.kf_center = kf_center; A.conn_kf = conn_kf; A.conn_rank = conn_rank; A.Scw = Scw; A.slot_off = slot_off; A.slot_pt = slot_pt;
  A.X = X; A.pt_bad = pt_bad; A.pt_done = pt_done;
  if (nd) { A.obs_off = obs_off; A.obs_kf = obs_kf; A.ref_kf = ref_kf; A.ref_level = ref_level; A.scale_factors = scale_factors; A.normal = normal; A.min_max = min_max; A.nd_written = nd_written; }
  A.corrected = corrected; A.non_corrected = non_corrected; A.pt_owner = pt_owner; A.counts = counts; A.status = status;
  A.rhit = (int32_t*)(wb + ws.rhit); A.contested = wb + ws.contested; A.kpos = (int32_t*)(wb + ws.kpos); A.own = (unsigned long long*)(wb + ws.own);
  A.cval = (int32_t*)(wb + ws.cval); A.cinv = (double*)(wb + ws.cinv); A.newT = (double*)(wb + ws.newT); A.newC = (double*)(wb + ws.newC);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 8, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0, ws.cleared, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.kpos, 0xFF, ws.cval - ws.kpos, st));           // (kpos and own are adjacent)
  auto grid = [](int n) { return dim3((unsigned)((n + MC_WG - 1) / MC_WG)); };
  hipLaunchKernelGGL(k_ml_init, grid(std::max(nconn, nd ? npts : 0)), dim3(MC_WG), 0, st, A);
  hipLaunchKernelGGL(k_ml_pose, grid(nconn), dim3(MC_WG), 0, st, A);
  if (nslots > 0 && npts > 0) {
    hipLaunchKernelGGL(k_ml_slots<0>, grid(nslots), dim3(MC_WG), 0, st, A);
    hipLaunchKernelGGL(k_ml_slots<1>, grid(nslots), dim3(MC_WG), 0, st, A);
  }
  if (npts > 0) hipLaunchKernelGGL(k_ml_points, grid(npts), dim3(MC_WG), 0, st, A);
  hipLaunchKernelGGL(k_ml_store, grid(nconn), dim3(MC_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_correct_loop(int nkf, double* kf_Tcw, double* kf_center, int nconn, const int32_t* conn_kf, const int32_t* conn_rank, const double* Scw,
                      const int32_t* slot_off, const int32_t* slot_pt, int npts, double* X, const uint8_t* pt_bad, const uint8_t* pt_done, const int32_t* obs_off,
                      const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, double* corrected,
                      double* non_corrected, int32_t* pt_owner, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(nkf >= 1 && nconn >= 1 && npts >= 0, ORBHIP_EINVAL, "orbl_correct_loop: bad count (nkf and nconn are >= 1)");
  ORBHIP_REQUIRE(kf_Tcw && conn_kf && Scw && slot_off && corrected && non_corrected && counts, ORBHIP_EINVAL, "orbl_correct_loop: NULL argument");
  ORBHIP_REQUIRE(npts == 0 || (X && pt_owner), ORBHIP_EINVAL, "orbl_correct_loop: NULL X or pt_owner");
  const bool any_nd = obs_off || obs_kf || ref_kf || ref_level || scale_factors || normal || min_max || nd_written;
  const bool nd = obs_off && ref_kf && ref_level && scale_factors && normal && min_max && nd_written;
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_correct_loop: the normal / depth arguments are given as a set");
  ORBHIP_REQUIRE(!nd || kf_center, ORBHIP_EINVAL, "orbl_correct_loop: the normals need kf_center");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_correct_loop: n_levels out of range");
  ORBHIP_REQUIRE(mc_finite(Scw, 7) && (Scw[0] * Scw[0] + Scw[1] * Scw[1]) + (Scw[2] * Scw[2] + Scw[3] * Scw[3]) > 0.0, ORBHIP_EINVAL,
                 "orbl_correct_loop: Scw is not finite or its quaternion is zero");
  static const char E[] = "orbl_correct_loop";
  int nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "slot_off", slot_off, nconn, &nslots));
  ORBHIP_REQUIRE(nslots == 0 || slot_pt, ORBHIP_EINVAL, "orbl_correct_loop: NULL slot_pt");
  if (nd) {
    ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
    ORBHIP_REQUIRE(nobs == 0 || obs_kf, ORBHIP_EINVAL, "orbl_correct_loop: NULL obs_kf");
  }
  ORBHIP_ARG(check_listed_once(E, "conn_kf", conn_kf, nconn, nkf));
  if (conn_rank) ORBHIP_ARG(check_permutation(E, "conn_rank", conn_rank, nconn));
  ORBHIP_ARG(check_index(E, "slot_pt", slot_pt, nslots, npts, true));
  if (nd) {
    ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
    const auto read = [&](int p) { return obs_off[p] != obs_off[p + 1] && !(pt_bad && pt_bad[p]); };          // (no normal: its reference keyframe is not read)
    ORBHIP_ARG(check_index_if(E, "ref_kf", ref_kf, npts, nkf, read));
    ORBHIP_ARG(check_index_if(E, "ref_level", ref_level, npts, n_levels, read));
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, nc = (size_t)nconn, np = (size_t)npts;
  const bool run_nd = nd && npts > 0;                               // (without points the device entry takes the normal / depth set as absent)
  RoundTrip R(W);
  const HostOut<double> t_Tcw = R.inout(kf_Tcw, 12 * nk), t_center = R.inout(kf_center, 3 * nk), t_X = R.inout(X, 3 * np);
  const HostIn<int32_t> d_conn = R.in(conn_kf, nc), d_rank = R.in(conn_rank, nc), d_slot_off = R.csr(slot_off, nc), d_slot_pt = R.in(slot_pt, (size_t)nslots);
  const HostIn<int32_t> d_obs_off = R.csr(run_nd ? obs_off : nullptr, np), d_obs_kf = R.in(run_nd ? obs_kf : nullptr, (size_t)nobs);
  const HostIn<int32_t> d_ref = R.in(run_nd ? ref_kf : nullptr, np), d_lvl = R.in(run_nd ? ref_level : nullptr, np);
  const HostIn<uint8_t> d_bad = R.in(pt_bad, np), d_done = R.in(pt_done, np);
  const HostIn<double> d_Scw = R.in(Scw, 7);
  const HostIn<float> d_sf = R.in(run_nd ? scale_factors : nullptr, (size_t)n_levels);
  const HostOut<int32_t> o_counts = R.out<int32_t>(2), o_owner = R.out<int32_t>(np);
  const HostOut<double> o_corr = R.out<double>(7 * nc), o_non = R.out<double>(7 * nc), o_normal = R.out<double>(3 * np, run_nd);
  const HostOut<float> o_mm = R.out<float>(2 * np, run_nd);
  const HostOut<uint8_t> o_wrote = R.out<uint8_t>(np, run_nd);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(ml_workspace(nkf, nconn, npts).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_correct_loop_device(nkf, t_Tcw.dev(), t_center.dev(), nconn, d_conn.dev(), d_rank.dev(), d_Scw.dev(), nslots, d_slot_off.dev(), d_slot_pt.dev(), npts,
                                     t_X.dev(), d_bad.dev(), d_done.dev(), nobs, d_obs_off.dev(), d_obs_kf.dev(), d_ref.dev(), d_lvl.dev(), d_sf.dev(), n_levels,
                                     o_corr.dev(), o_non.dev(), o_owner.dev(), o_normal.dev(), o_mm.dev(), o_wrote.dev(), o_counts.dev(), o_status.dev(),
                                     R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 2);
  R.copy_out(o_corr, corrected, 7 * nc); R.copy_out(o_non, non_corrected, 7 * nc);
  R.copy_out(t_Tcw, kf_Tcw, 12 * nk); R.copy_out(t_center, kf_center, 3 * nk); R.copy_out(t_X, X, 3 * np);
  R.copy_out(o_owner, pt_owner, np);
  for (size_t p = 0; run_nd && p < np; p++) {
    if (o_owner[p] < 0) continue;                                   // (rows of points that did not move are not touched)
    nd_written[p] = o_wrote[p];
    if (o_wrote[p]) { std::copy_n(&o_normal[3 * p], 3, normal + 3 * p); std::copy_n(&o_mm[2 * p], 2, min_max + 2 * p); }
  }
  return 0;
}

int orbl_propagate_global_ba_workspace(int nkf, int npts, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && npts >= 0 && bytes, ORBHIP_EINVAL, "orbl_propagate_global_ba_workspace: bad argument");
  *bytes = orbhip::gb_workspace_bytes(nkf);
  return 0;
}

int orbl_propagate_global_ba_device(int nkf, double* kf_Tcw, double* kf_gba_Tcw, uint8_t* kf_in_gba, const int32_t* kf_parent, int n_origin, const int32_t* origin_kf,
                                    double* kf_center, int npts, double* X, const uint8_t* pt_bad, const uint8_t* pt_in_gba, const double* pt_gba_X,
                                    const int32_t* pt_ref_kf, double* kf_bef_Tcw, uint8_t* kf_reached, uint8_t* pt_moved, int32_t* counts, uint32_t* status,
                                    void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(nkf >= 0 && n_origin >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_propagate_global_ba: negative count");
  ORBHIP_REQUIRE(counts && workspace, ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL counts or workspace");
  ORBHIP_REQUIRE(nkf == 0 || (kf_Tcw && kf_gba_Tcw && kf_in_gba && kf_parent && kf_bef_Tcw && kf_reached), ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL keyframe argument");
  ORBHIP_REQUIRE(n_origin == 0 || origin_kf, ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL origin_kf");
  ORBHIP_REQUIRE(npts == 0 || (X && pt_ref_kf && pt_moved), ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL point argument");
  ORBHIP_REQUIRE((pt_in_gba != nullptr) == (pt_gba_X != nullptr), ORBHIP_EINVAL, "orbl_propagate_global_ba: pt_in_gba and pt_gba_X are given together");
  const void* q8[] = {kf_Tcw, kf_gba_Tcw, kf_center, X, pt_gba_X, kf_bef_Tcw};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_propagate_global_ba: 64-bit arrays must be 8-byte aligned");
  const void* q4[] = {kf_parent, origin_kf, pt_ref_kf, counts, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_propagate_global_ba: 32-bit arrays must be 4-byte aligned");
  GbArgs A; std::memset(&A, 0, sizeof(A));
  A.nkf = nkf; A.n_origin = n_origin; A.npts = npts;
  A.kf_Tcw = kf_Tcw; A.kf_gba = kf_gba_Tcw; A.kf_in_gba = kf_in_gba; A.kf_parent = kf_parent; A.origin_kf = origin_kf; A.kf_center = kf_center;
  A.X = X; A.pt_bad = pt_bad; A.pt_in_gba = pt_in_gba; A.pt_gba_X = pt_gba_X; A.pt_ref_kf = pt_ref_kf;
  A.kf_bef = kf_bef_Tcw; A.kf_reached = kf_reached; A.pt_moved = pt_moved; A.counts = counts; A.status = status; A.state = (uint8_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 16, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(workspace, 0, gb_workspace_bytes(nkf), st));
  auto grid = [](int n) { return dim3((unsigned)((n + MC_WG - 1) / MC_WG)); };
  if (nkf > 0) {
    if (n_origin > 0) hipLaunchKernelGGL(k_gb_origins, grid(n_origin), dim3(MC_WG), 0, st, A);
    hipLaunchKernelGGL(k_gb_init, grid(nkf), dim3(MC_WG), 0, st, A);
    hipLaunchKernelGGL(k_gb_walk, dim3(1), dim3(MC_CHAIN_WG), 0, st, A);
    hipLaunchKernelGGL(k_gb_apply, grid(nkf), dim3(MC_WG), 0, st, A);
  }
  if (npts > 0) hipLaunchKernelGGL(k_gb_points, grid(npts), dim3(MC_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_propagate_global_ba(int nkf, double* kf_Tcw, double* kf_gba_Tcw, uint8_t* kf_in_gba, const int32_t* kf_parent, int n_origin, const int32_t* origin_kf,
                             double* kf_center, int npts, double* X, const uint8_t* pt_bad, const uint8_t* pt_in_gba, const double* pt_gba_X,
                             const int32_t* pt_ref_kf, double* kf_bef_Tcw, uint8_t* kf_reached, uint8_t* pt_moved, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(nkf >= 0 && n_origin >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_propagate_global_ba: negative count");
  ORBHIP_REQUIRE(counts, ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL counts");
  ORBHIP_REQUIRE(nkf == 0 || (kf_Tcw && kf_gba_Tcw && kf_in_gba && kf_parent && kf_bef_Tcw && kf_reached), ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL keyframe argument");
  ORBHIP_REQUIRE(n_origin == 0 || origin_kf, ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL origin_kf");
  ORBHIP_REQUIRE(npts == 0 || (X && pt_ref_kf && pt_moved), ORBHIP_EINVAL, "orbl_propagate_global_ba: NULL point argument");
  ORBHIP_REQUIRE((pt_in_gba != nullptr) == (pt_gba_X != nullptr), ORBHIP_EINVAL, "orbl_propagate_global_ba: pt_in_gba and pt_gba_X are given together");
  static const char E[] = "orbl_propagate_global_ba";
  ORBHIP_ARG(check_index(E, "origin_kf", origin_kf, n_origin, nkf));
  ORBHIP_ARG(check_index(E, "kf_parent", kf_parent, nkf, nkf, true));
  for (int k = 0; k < nkf; k++) ORBHIP_REQUIRE(kf_parent[k] != k, ORBHIP_EINVAL, "orbl_propagate_global_ba: a keyframe is its own kf_parent");
  const auto read = [&](int p) { return !(pt_bad && pt_bad[p]) && !(pt_in_gba && pt_in_gba[p]); };           // (else its reference keyframe is not read)
  ORBHIP_ARG(check_index_if(E, "pt_ref_kf", pt_ref_kf, npts, nkf, read));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts;
  RoundTrip R(W);
  const HostOut<double> t_Tcw = R.inout(kf_Tcw, 12 * nk), t_gba = R.inout(kf_gba_Tcw, 12 * nk), t_center = R.inout(kf_center, 3 * nk), t_X = R.inout(X, 3 * np);
  const HostOut<uint8_t> t_in_gba = R.inout(kf_in_gba, nk);
  const HostIn<int32_t> d_parent = R.in(kf_parent, nk), d_origin = R.in(origin_kf, (size_t)n_origin), d_ref = R.in(pt_ref_kf, np);
  const HostIn<uint8_t> d_bad = R.in(pt_bad, np), d_pt_in = R.in(pt_in_gba, np);
  const HostIn<double> d_gba_X = R.in(pt_gba_X, 3 * np);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4);
  const HostOut<double> o_bef = R.out<double>(12 * nk);
  const HostOut<uint8_t> o_reached = R.out<uint8_t>(nk), o_moved = R.out<uint8_t>(np);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(gb_workspace_bytes(nkf));
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_propagate_global_ba_device(nkf, t_Tcw.dev(), t_gba.dev(), t_in_gba.dev(), d_parent.dev(), n_origin, d_origin.dev(), t_center.dev(), npts, t_X.dev(),
                                            d_bad.dev(), d_pt_in.dev(), d_gba_X.dev(), d_ref.dev(), o_bef.dev(), o_reached.dev(), o_moved.dev(), o_counts.dev(),
                                            o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 4);
  R.copy_out(t_Tcw, kf_Tcw, 12 * nk); R.copy_out(t_gba, kf_gba_Tcw, 12 * nk); R.copy_out(t_in_gba, kf_in_gba, nk); R.copy_out(t_center, kf_center, 3 * nk);
  R.copy_out(o_reached, kf_reached, nk);
  for (size_t k = 0; k < nk; k++)
    if (o_reached[k]) std::copy_n(&o_bef[12 * k], 12, kf_bef_Tcw + 12 * k);          // (rows of unreached keyframes are not touched)
  R.copy_out(t_X, X, 3 * np); R.copy_out(o_moved, pt_moved, np);
  return 0;
}

}  // extern "C"
