// orb_localba.inc -- the two halves of CeresOptimizer::LocalBundleAdjustment around the optimisation, on the flat map tables:
// orbl_local_ba_assemble* collects the local keyframes, the local map points and the fixed keyframes and flattens one row per
// (point, observing keyframe) (src/CeresOptimizer.cc:346-406, :423-506, in the order csrc/compat/orbslam_dropin.h fixed), and
// orbl_local_ba_apply* writes the result back (:573-598): the outlier erases with their SetBadFlag cascade, SetPose, SetWorldPos and
// UpdateNormalAndDepth.  Textually included by orb_localmap.hip.  FP64 throughout, no fused multiply-add (-ffp-contract=off); every
// sum is taken in the order written here (DESIGN.md section 2, "LocalBundleAdjustment on the tables").
//
// assemble: every list is an ORDERED compaction.  A flag per element is laid out in the order of the list (keyframe id, kf_rank,
// pt_rank), an exclusive scan gives each flagged element its place (k_la_*scan: mt_block_excl per workgroup, then the workgroup sums by
// k_mt_scan_sums), and the element's own lane writes it there.  Atomics only take order-free minima, maxima and ors.
//   k_la_stamp       one lane per list position / keyframe / point: first[k] = the least position of (cur_kf, nbr_kf...) that names
//                    keyframe k (atomicMin), the inverses of the two ranks (atomicMax: a repeat is flagged), the offset checks
//   k_la_local       one lane per list position: kf_role 1 / 3, the place among the local cameras by counting the (kf_id, position)
//                    pairs below its own, the camera's row
//   k_la_slots       one workgroup per local keyframe: pt_local (every writer stores the same byte)
//   k_la_fixed       one lane per point: the observers of a local point that are neither stamped nor bad (the same byte again)
//   k_la_kscan       one lane per kf_rank position: the fixed flags;   k_la_fixed_cams: their rows, kf_role 2, counts[0..1]
//   k_la_pscan       one lane per pt_rank position: (local, rows of the point) as one 64-bit pair;   k_la_emit: the points and rows
// apply: the erases of one point are sequential, points are independent of each other.
//   k_ap_mark        one lane per row: want[e] = the first row that erases observation e (atomicMin)
//   k_ap_erase       one lane per point: its marked observations in row order, the reference keyframe, the bad flag and its cascade
//   k_ap_write       one lane per camera / local point: SetPose with the centre, SetWorldPos
//   k_ap_normals     one lane per local point: UpdateNormalAndDepth (mt_normal_depth) over the alive observations, the new centres
// Outputs are written with vector stores only.
#include "orb_maptable.h"        /* LA_WG, the LA_ST_* bits of *status (orbl_local_ba_assemble_device, orbl_local_ba_apply_device), LA_NONE */

namespace orbhip {

struct LaArgs {
  int cur_kf, n_nbr, nkf, nslots, npts, nobs, n_levels, cap_cam, cap_pts, cap_obs, nbk, nbp;
  const int32_t* nbr_kf; const int32_t* kf_id; const uint8_t* kf_bad; const int32_t* kf_rank; const double* kf_Tcw; const double* kf_K4;
  const int32_t* slot_off; const int32_t* slot_pt; const double* X; const uint8_t* pt_bad; const int32_t* pt_rank;
  const int32_t* obs_off; const int32_t* obs_kf; const float* obs_uv; const int32_t* obs_level; const float* inv_level_sigma2;
  int32_t* counts; int32_t* cam_kf; double* K4; double* poses7; uint8_t* cam_fixed; uint8_t* cam_local; int32_t* lpt_pt; double* pts3;
  int32_t* lobs_cam; int32_t* lobs_pt; double* lobs_uv; float* lobs_isg; int32_t* lobs_src; uint8_t* kf_role; uint8_t* pt_local; uint32_t* status;
  // workspace: first[nkf] | inv_kf[nkf] | inv_pt[npts] | cam_of[nkf] (all set to all ones per call) | fixed[nkf] (cleared per call) |
  // kscan[nkf] | ksums[nbk + 1] | pscan[npts] | psums[nbp + 1] | meta[4]
  uint32_t* first; int32_t* inv_kf; int32_t* inv_pt; int32_t* cam_of; uint8_t* fixed; mt_u64 *kscan, *ksums, *pscan, *psums; int32_t* meta;
};

__device__ __forceinline__ bool la_kf_bad(const LaArgs& a, int k) { return a.kf_bad && a.kf_bad[k]; }
__device__ __forceinline__ int la_kf_at(const LaArgs& a, int pos) { return pos == 0 ? a.cur_kf : a.nbr_kf[pos - 1]; }
// the keyframe of list position q when that position is where the list first names it and it becomes a local camera, else -1
__device__ __forceinline__ int la_local_at(const LaArgs& a, int q) {
  const int k = la_kf_at(a, q);
  if (k < 0 || k >= a.nkf || a.first[k] != (uint32_t)q) return -1;
  return (q == 0 || !la_kf_bad(a, k)) ? k : -1;                                // (:359: a bad neighbour is stamped, not collected)
}

__global__ __launch_bounds__(LA_WG) void k_la_stamp(LaArgs a) {
  const int i = blockIdx.x * LA_WG + threadIdx.x;
  if (i <= a.n_nbr) {
    const int k = la_kf_at(a, i);
    if (k < 0 || k >= a.nkf) mt_flag(a.status, LA_ST_KF);
    else atomicMin(&a.first[k], (uint32_t)i);
  }
  if (i < a.nkf) {
    int lo, hi;
    if (!mt_range(a.slot_off, i, a.nslots, &lo, &hi)) mt_flag(a.status, LA_ST_OFFSETS);
    if (a.kf_rank) {
      const int r = a.kf_rank[i];
      if (r < 0 || r >= a.nkf) mt_flag(a.status, LA_ST_RANK);
      else if (atomicMax(&a.inv_kf[r], i) != -1) mt_flag(a.status, LA_ST_RANK);  // (not a permutation: the highest index holds the place)
    }
  }
  if (i < a.npts) {
    int lo, hi;
    if (!mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, LA_ST_OFFSETS);
    if (a.pt_rank) {
      const int r = a.pt_rank[i];
      if (r < 0 || r >= a.npts) mt_flag(a.status, LA_ST_RANK);
      else if (atomicMax(&a.inv_pt[r], i) != -1) mt_flag(a.status, LA_ST_RANK);
    }
  }
}

// one camera row: the keyframe, its intrinsics, Matrix4dToMatrix_7_1 of its pose (ba_matrix4d_to_pose7), the two flags
__device__ __forceinline__ void la_write_cam(const LaArgs& a, int c, int k, bool local) {
  a.cam_of[k] = c;
  if (c >= a.cap_cam) return;
  mt_pose34_to_pose7(a.kf_Tcw + 12 * (size_t)k, a.poses7 + 7 * (size_t)c);
  for (int j = 0; j < 4; j++) a.K4[4 * (size_t)c + j] = a.kf_K4[4 * (size_t)k + j];
  a.cam_kf[c] = k;
  a.cam_local[c] = local ? 1 : 0;
  a.cam_fixed[c] = (!local || a.kf_id[k] == 0) ? 1 : 0;                        // (:476-481, :499-502)
}

__global__ __launch_bounds__(LA_WG) void k_la_local(LaArgs a) {
  const int pos = blockIdx.x * LA_WG + threadIdx.x;
  if (pos > a.n_nbr) return;
  const int k0 = la_kf_at(a, pos);
  if (k0 < 0 || k0 >= a.nkf || a.first[k0] != (uint32_t)pos) return;           // (out of range, or named earlier in the list)
  const int k = la_local_at(a, pos);
  a.kf_role[k0] = k >= 0 ? 1 : 3;
  if (k < 0) return;
  const int id = a.kf_id[k];
  int below = 0, n_local = 0;
  for (int q = 0; q <= a.n_nbr; q++) {                                         // by keyframe id; ties: the current keyframe, then list order
    const int kq = la_local_at(a, q);
    if (kq < 0) continue;
    n_local++;
    const int idq = a.kf_id[kq];
    below += (idq < id || (idq == id && q < pos)) ? 1 : 0;
  }
  la_write_cam(a, below, k, true);
  if (pos == 0) a.meta[0] = n_local;
}

__global__ __launch_bounds__(LA_WG) void k_la_slots(LaArgs a) {
  const int k = la_local_at(a, (int)blockIdx.x);                               // (workgroup-uniform)
  if (k < 0) return;
  int lo, hi;
  if (!mt_range(a.slot_off, k, a.nslots, &lo, &hi)) return;
  for (int s = lo + (int)threadIdx.x; s < hi; s += LA_WG) {
    const int p = a.slot_pt[s];
    if (p < -1 || p >= a.npts) { mt_flag(a.status, LA_ST_PT); continue; }
    if (p >= 0 && !(a.pt_bad && a.pt_bad[p])) a.pt_local[p] = 1;               // (:375-380)
  }
}

__global__ __launch_bounds__(LA_WG) void k_la_fixed(LaArgs a) {
  const int p = blockIdx.x * LA_WG + threadIdx.x;
  if (p >= a.npts || !a.pt_local[p]) return;
  int lo, hi;
  if (!mt_range(a.obs_off, p, a.nobs, &lo, &hi)) return;
  for (int e = lo; e < hi; e++) {                                              // (:389-405)
    const int k = a.obs_kf[e];
    if (k < 0 || k >= a.nkf) { mt_flag(a.status, LA_ST_KF); continue; }
    if (a.kf_role[k] == 0 && !la_kf_bad(a, k)) a.fixed[k] = 1;
  }
}

__device__ __forceinline__ int la_kf_of_rank(const LaArgs& a, int r) { return a.kf_rank ? a.inv_kf[r] : r; }
__device__ __forceinline__ int la_pt_of_rank(const LaArgs& a, int r) { return a.pt_rank ? a.inv_pt[r] : r; }

__global__ __launch_bounds__(LA_WG) void k_la_kscan(LaArgs a) {
  __shared__ mt_u64 sw[LA_WG / 64];
  const int r = blockIdx.x * LA_WG + threadIdx.x;
  const int k = r < a.nkf ? la_kf_of_rank(a, r) : -1;
  mt_u64 tot;
  const mt_u64 ex = mt_block_excl<LA_WG>(k >= 0 && a.fixed[k] ? 1ull : 0ull, sw, &tot);
  if (r < a.nkf) a.kscan[r] = ex;
  if (threadIdx.x == 0) a.ksums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(LA_WG) void k_la_fixed_cams(LaArgs a) {
  const int r = blockIdx.x * LA_WG + threadIdx.x;
  if (r >= a.nkf) return;
  const int n_local = a.meta[0];
  if (r == 0) {
    const int ncam = n_local + (int)a.ksums[a.nbk];
    a.counts[0] = ncam; a.counts[1] = n_local;
    if (ncam > a.cap_cam) mt_flag(a.status, LA_ST_CAP_CAM);
  }
  const int k = la_kf_of_rank(a, r);
  if (k < 0 || !a.fixed[k]) return;
  a.kf_role[k] = 2;
  la_write_cam(a, n_local + (int)(a.kscan[r] + a.ksums[blockIdx.x]), k, false);
}

// whether observation e of a local point becomes a row: its keyframe is not bad and has a camera (:432, :458, :483)
__device__ __forceinline__ bool la_row_ok(const LaArgs& a, int e) {
  return mt_row_ok(a.obs_kf, a.obs_level, e, a.nkf, a.n_levels, a.kf_bad, a.cam_of, a.status, LA_ST_KF, LA_ST_LEVEL);
}

__global__ __launch_bounds__(LA_WG) void k_la_pscan(LaArgs a) {
  __shared__ mt_u64 sw[LA_WG / 64];
  const int r = blockIdx.x * LA_WG + threadIdx.x;
  const int p = r < a.npts ? la_pt_of_rank(a, r) : -1;
  mt_u64 v = 0;
  if (p >= 0 && a.pt_local[p]) {
    int lo, hi, rows = 0;
    if (mt_range(a.obs_off, p, a.nobs, &lo, &hi))
      for (int e = lo; e < hi; e++) rows += la_row_ok(a, e) ? 1 : 0;
    v = ((mt_u64)(uint32_t)rows << 32) | 1ull;                                  // (rows, points): neither sum reaches 2^31
  }
  mt_u64 tot;
  const mt_u64 ex = mt_block_excl<LA_WG>(v, sw, &tot);
  if (r < a.npts) a.pscan[r] = ex;
  if (threadIdx.x == 0) a.psums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(LA_WG) void k_la_emit(LaArgs a) {
  const int r = blockIdx.x * LA_WG + threadIdx.x;
  if (r >= a.npts) return;
  if (r == 0) {
    const mt_u64 t = a.psums[a.nbp];
    const int np = (int)(uint32_t)t, no = (int)(t >> 32);
    a.counts[2] = np; a.counts[3] = no;
    if (np > a.cap_pts) mt_flag(a.status, LA_ST_CAP_PTS);
    if (no > a.cap_obs) mt_flag(a.status, LA_ST_CAP_OBS);
  }
  const int p = la_pt_of_rank(a, r);
  if (p < 0 || !a.pt_local[p]) return;
  const mt_u64 at = a.pscan[r] + a.psums[blockIdx.x];
  const int j = (int)(uint32_t)at;
  int row = (int)(at >> 32);
  if (j < a.cap_pts) {
    a.lpt_pt[j] = p;
    for (int q = 0; q < 3; q++) a.pts3[3 * (size_t)j + q] = a.X[3 * (size_t)p + q];
  }
  int lo, hi;
  if (!mt_range(a.obs_off, p, a.nobs, &lo, &hi)) return;
  for (int e = lo; e < hi; e++) {
    if (!la_row_ok(a, e)) continue;
    if (row < a.cap_obs) {
      a.lobs_cam[row] = a.cam_of[a.obs_kf[e]]; a.lobs_pt[row] = j;
      a.lobs_uv[2 * (size_t)row] = (double)a.obs_uv[2 * (size_t)e]; a.lobs_uv[2 * (size_t)row + 1] = (double)a.obs_uv[2 * (size_t)e + 1];
      a.lobs_isg[row] = a.inv_level_sigma2[a.obs_level[e]];
      a.lobs_src[row] = e;
    }
    row++;
  }
}

// workspace sections, each rounded up to 256 bytes; [0, ones) is set to all ones and `fixed` is cleared by every call
struct LaWs { size_t first, inv_kf, inv_pt, cam_of, ones, fixed, kscan, ksums, pscan, psums, meta, total; int nbk, nbp; };
static LaWs la_workspace(int nkf, int npts) {
  LaWs w; Carve ws;
  w.nbk = (nkf + LA_WG - 1) / LA_WG; w.nbp = (npts + LA_WG - 1) / LA_WG;
  w.first = ws.take(4 * (size_t)nkf); w.inv_kf = ws.take(4 * (size_t)nkf); w.inv_pt = ws.take(4 * (size_t)npts); w.cam_of = ws.take(4 * (size_t)nkf);
  w.ones = ws.total;
  w.fixed = ws.take((size_t)nkf);
  w.kscan = ws.take(8 * (size_t)nkf); w.ksums = ws.take(8 * ((size_t)w.nbk + 1)); w.pscan = ws.take(8 * (size_t)npts); w.psums = ws.take(8 * ((size_t)w.nbp + 1));
  w.meta = ws.take(16);
  w.total = ws.total;
  return w;
}

// ---------------------------------------------------------------------------------------------------------- write-back
struct ApArgs {
  int ncam, npts_local, nobs_local, nkf, nslots, npts, nobs, n_levels;
  const int32_t* cam_kf; const uint8_t* cam_local; const double* poses7; const int32_t* lpt_pt; const double* pts3; const int32_t* lobs_src; const uint8_t* obs_erase;
  double* kf_Tcw; double* kf_center; const int32_t* slot_off; int32_t* slot_pt; double* X; uint8_t* pt_bad; int32_t* pt_nobs; int32_t* pt_ref_kf;
  const int32_t* obs_off; const int32_t* obs_kf; const int32_t* obs_slot; const int32_t* obs_level; const int32_t* kf_level0; const float* scale_factors;
  uint8_t* obs_erased; double* normal; float* min_max; uint8_t* nd_written; int32_t* counts; uint32_t* status;
  uint32_t* want;                 // workspace: want[nobs] (set to all ones per call)
};

__global__ __launch_bounds__(LA_WG) void k_ap_mark(ApArgs a) {
  const int i = blockIdx.x * LA_WG + threadIdx.x;
  if (i >= a.nobs_local || !a.obs_erase[i]) return;
  const int e = a.lobs_src[i];
  if (e < 0 || e >= a.nobs) { mt_flag(a.status, LA_ST_OBS); return; }
  atomicMin(&a.want[e], (uint32_t)i);                                          // (a later row on the same observation finds it dead)
}

// the observation dies: KeyFrame::EraseMapPointMatch on its slot, whatever it holds
__device__ __forceinline__ void ap_kill(const ApArgs& a, int e) {
  a.obs_erased[e] = 1;
  const int k = a.obs_kf[e];
  if (k < 0 || k >= a.nkf) { mt_flag(a.status, LA_ST_KF); return; }
  int lo, hi;
  if (!mt_range(a.slot_off, k, a.nslots, &lo, &hi)) { mt_flag(a.status, LA_ST_OFFSETS); return; }
  const int s = a.obs_slot[e];
  if (s < 0 || s >= hi - lo) { mt_flag(a.status, LA_ST_OBS); return; }
  a.slot_pt[lo + s] = -1;
}

__global__ __launch_bounds__(LA_WG) void k_ap_erase(ApArgs a) {
  const int p = blockIdx.x * LA_WG + threadIdx.x;
  int n_erased = 0, n_dead = 0, n_bad = 0;
  int lo = 0, hi = 0;
  if (p < a.npts && !mt_range(a.obs_off, p, a.nobs, &lo, &hi)) mt_flag(a.status, LA_ST_OFFSETS);
  if (lo < hi) {
    int nobs = a.pt_nobs[p], ref = a.pt_ref_kf[p];
    long long prev = -1;
    for (;;) {                                                                 // the marked observations of the point in row order
      uint32_t best = LA_NONE; int be = -1;
      for (int e = lo; e < hi; e++) { const uint32_t w = a.want[e]; if (w != LA_NONE && (long long)w > prev && w < best) { best = w; be = e; } }
      if (be < 0) break;
      prev = (long long)best;
      const int k = a.obs_kf[be];
      ap_kill(a, be);                                                          // (:578, src/MapPoint.cc:144-151)
      n_erased++; n_dead++; nobs--;
      if (ref == k)                                                            // (:153-154; it stays when no observation is left)
        for (int e = lo; e < hi; e++) if (!a.obs_erased[e]) { ref = a.obs_kf[e]; break; }
      if (nobs <= 2) {                                                         // SetBadFlag (:157-161, :174-188): the rows behind find nothing alive
        for (int e = lo; e < hi; e++) if (!a.obs_erased[e]) { ap_kill(a, e); n_dead++; }
        a.pt_bad[p] = 1; n_bad = 1;
        break;
      }
    }
    if (n_erased) { a.pt_nobs[p] = nobs; a.pt_ref_kf[p] = ref; }
  }
  n_erased = mt_wave_sum(n_erased); n_dead = mt_wave_sum(n_dead); n_bad = mt_wave_sum(n_bad);
  if ((threadIdx.x & 63) == 0) {
    if (n_erased) atomicAdd(&a.counts[0], n_erased);
    if (n_bad) atomicAdd(&a.counts[1], n_bad);
    if (n_dead) atomicAdd(&a.counts[2], n_dead);
  }
}

__global__ __launch_bounds__(LA_WG) void k_ap_write(ApArgs a) {
  const int i = blockIdx.x * LA_WG + threadIdx.x;
  if (i < a.ncam && a.cam_local[i]) {                                          // (:585-591) Matrix_7_1_ToMatrix4d (ba_pose7_to_matrix4d), KeyFrame::SetPose
    const int k = a.cam_kf[i];
    if (k < 0 || k >= a.nkf) mt_flag(a.status, LA_ST_KF);
    else {
      double T[12];
      mt_pose7_to_pose34(a.poses7 + 7 * (size_t)i, T);
      mt_set_pose(a.kf_Tcw, a.kf_center, k, T);
    }
  }
  if (i < a.npts_local) {                                                      // (:596) SetWorldPos, bad points included
    const int p = a.lpt_pt[i];
    if (p < 0 || p >= a.npts) mt_flag(a.status, LA_ST_PT);
    else for (int j = 0; j < 3; j++) a.X[3 * (size_t)p + j] = a.pts3[3 * (size_t)i + j];
  }
}

__global__ __launch_bounds__(LA_WG) void k_ap_normals(ApArgs a) {
  const int j = blockIdx.x * LA_WG + threadIdx.x;
  int wrote = 0;
  const int p = j < a.npts_local ? a.lpt_pt[j] : -1;
  int lo = 0, hi = 0;
  if (p >= 0 && p < a.npts && !a.pt_bad[p] && mt_range(a.obs_off, p, a.nobs, &lo, &hi)) {       // (src/MapPoint.cc:342)
    const int ref = a.pt_ref_kf[p];
    // over what is alive (:352-360); the level is that of the reference keyframe's own observation, and without one operator[] on the
    // copy of the observations inserts index 0 (:366)
    const int res = mt_normal_depth(a.obs_kf, lo, hi, a.nkf, a.X[3 * (size_t)p], a.X[3 * (size_t)p + 1], a.X[3 * (size_t)p + 2], ref, a.scale_factors, a.n_levels,
                                    a.normal + 3 * (size_t)p, a.min_max + 2 * (size_t)p, [&](int e) { return !a.obs_erased[e]; },
                                    [&](int k) { return make_double3(a.kf_center[3 * (size_t)k], a.kf_center[3 * (size_t)k + 1], a.kf_center[3 * (size_t)k + 2]); },
                                    [&](int e) { const int l = e >= 0 ? a.obs_level[e] : -1; return l != -1 ? l : a.kf_level0 ? a.kf_level0[ref] : 0; });
    if (res == MT_ND_KF || res == MT_ND_REF) mt_flag(a.status, LA_ST_KF);
    if (res == MT_ND_LEVEL) mt_flag(a.status, LA_ST_LEVEL);
    if (res == MT_ND_OK) { a.nd_written[p] = 1; wrote = 1; }
  }
  const uint64_t m = __ballot(wrote != 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts[3], (int)__popcll(m));
}

static size_t ap_workspace_bytes(int nobs) { Carve ws; ws.take(4 * (size_t)nobs); return ws.total > 0 ? ws.total : 256; }

}  // namespace orbhip

extern "C" {

int orbl_local_ba_assemble_workspace(int nkf, int npts, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && npts >= 0 && bytes, ORBHIP_EINVAL, "orbl_local_ba_assemble_workspace: bad argument");
  *bytes = orbhip::la_workspace(nkf, npts).total;
  return 0;
}

int orbl_local_ba_assemble_device(int cur_kf, int n_nbr, const int32_t* nbr_kf, int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const int32_t* kf_rank,
                                  const double* kf_Tcw, const double* kf_K4, int nslots, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const double* X,
                                  const uint8_t* pt_bad, const int32_t* pt_rank, int nobs, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv,
                                  const int32_t* obs_level, const float* inv_level_sigma2, int n_levels, int cap_cam, int cap_pts, int cap_obs, int32_t* counts,
                                  int32_t* cam_kf, double* K4, double* poses7, uint8_t* cam_fixed, uint8_t* cam_local, int32_t* lpt_pt, double* pts3, int32_t* lobs_cam,
                                  int32_t* lobs_pt, double* lobs_uv, float* lobs_inv_sigma2, int32_t* lobs_src, uint8_t* kf_role, uint8_t* pt_local, uint32_t* status,
                                  void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(nkf >= 1 && n_nbr >= 0 && nslots >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_local_ba_assemble: bad count (nkf is >= 1)");
  ORBHIP_REQUIRE(cur_kf >= 0 && cur_kf < nkf, ORBHIP_EINVAL, "orbl_local_ba_assemble: cur_kf out of range");
  ORBHIP_REQUIRE(cap_cam >= 0 && cap_pts >= 0 && cap_obs >= 0, ORBHIP_EINVAL, "orbl_local_ba_assemble: negative capacity");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_local_ba_assemble: n_levels out of range");
  ORBHIP_REQUIRE(kf_id && kf_Tcw && kf_K4 && kf_slot_off && inv_level_sigma2 && counts && kf_role && workspace, ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL argument");
  ORBHIP_REQUIRE(n_nbr == 0 || nbr_kf, ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL nbr_kf");
  ORBHIP_REQUIRE(nslots == 0 || kf_slot_pt, ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL kf_slot_pt");
  ORBHIP_REQUIRE(npts == 0 || (X && obs_off && pt_local), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL point argument");
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_uv && obs_level), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL observation argument");
  ORBHIP_REQUIRE(cap_cam == 0 || (cam_kf && K4 && poses7 && cam_fixed && cam_local), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL camera output");
  ORBHIP_REQUIRE(cap_pts == 0 || (lpt_pt && pts3), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL point output");
  ORBHIP_REQUIRE(cap_obs == 0 || (lobs_cam && lobs_pt && lobs_uv && lobs_inv_sigma2 && lobs_src), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL row output");
  const void* q8[] = {kf_Tcw, kf_K4, X, K4, poses7, pts3, lobs_uv, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_local_ba_assemble: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {nbr_kf, kf_id, kf_rank, kf_slot_off, kf_slot_pt, pt_rank, obs_off, obs_kf, obs_uv, obs_level, inv_level_sigma2, counts, cam_kf, lpt_pt, lobs_cam, lobs_pt,
                      lobs_inv_sigma2, lobs_src, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_local_ba_assemble: 32-bit arrays must be 4-byte aligned");
  const LaWs ws = la_workspace(nkf, npts);
  uint8_t* wb = (uint8_t*)workspace;
  LaArgs A; std::memset(&A, 0, sizeof(A));
  A.cur_kf = cur_kf; A.n_nbr = n_nbr; A.nkf = nkf; A.nslots = nslots; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels;
  A.cap_cam = cap_cam; A.cap_pts = cap_pts; A.cap_obs = cap_obs; A.nbk = ws.nbk; A.nbp = ws.nbp;
  A.nbr_kf = nbr_kf; A.kf_id = kf_id; A.kf_bad = kf_bad; A.kf_rank = kf_rank; A.kf_Tcw = kf_Tcw; A.kf_K4 = kf_K4; A.slot_off = kf_slot_off; A.slot_pt = kf_slot_pt;
  A.X = X; A.pt_bad = pt_bad; A.pt_rank = pt_rank; A.obs_off = obs_off; A.obs_kf = obs_kf; A.obs_uv = obs_uv; A.obs_level = obs_level; A.inv_level_sigma2 = inv_level_sigma2;
  A.counts = counts; A.cam_kf = cam_kf; A.K4 = K4; A.poses7 = poses7; A.cam_fixed = cam_fixed; A.cam_local = cam_local; A.lpt_pt = lpt_pt; A.pts3 = pts3;
  A.lobs_cam = lobs_cam; A.lobs_pt = lobs_pt; A.lobs_uv = lobs_uv; A.lobs_isg = lobs_inv_sigma2; A.lobs_src = lobs_src; A.kf_role = kf_role; A.pt_local = pt_local;
  A.status = status;
  A.first = (uint32_t*)(wb + ws.first); A.inv_kf = (int32_t*)(wb + ws.inv_kf); A.inv_pt = (int32_t*)(wb + ws.inv_pt); A.cam_of = (int32_t*)(wb + ws.cam_of);
  A.fixed = wb + ws.fixed; A.kscan = (mt_u64*)(wb + ws.kscan); A.ksums = (mt_u64*)(wb + ws.ksums); A.pscan = (mt_u64*)(wb + ws.pscan); A.psums = (mt_u64*)(wb + ws.psums);
  A.meta = (int32_t*)(wb + ws.meta);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 16, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0xFF, ws.ones, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.fixed, 0, (size_t)nkf, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(kf_role, 0, (size_t)nkf, st));
  if (npts > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(pt_local, 0, (size_t)npts, st));
  auto grid = [](int n) { return dim3((unsigned)((n + LA_WG - 1) / LA_WG)); };
  hipLaunchKernelGGL(k_la_stamp, grid(std::max(std::max(n_nbr + 1, nkf), npts)), dim3(LA_WG), 0, st, A);
  hipLaunchKernelGGL(k_la_local, grid(n_nbr + 1), dim3(LA_WG), 0, st, A);
  if (nslots > 0 && npts > 0) hipLaunchKernelGGL(k_la_slots, dim3((unsigned)(n_nbr + 1)), dim3(LA_WG), 0, st, A);
  if (npts > 0) hipLaunchKernelGGL(k_la_fixed, grid(npts), dim3(LA_WG), 0, st, A);
  hipLaunchKernelGGL(k_la_kscan, grid(nkf), dim3(LA_WG), 0, st, A);
  hipLaunchKernelGGL(k_mt_scan_sums<mt_u64>, dim3(1), dim3(MT_SUM_WG), 0, st, A.ksums, A.nbk);
  hipLaunchKernelGGL(k_la_fixed_cams, grid(nkf), dim3(LA_WG), 0, st, A);
  if (npts > 0) {
    hipLaunchKernelGGL(k_la_pscan, grid(npts), dim3(LA_WG), 0, st, A);
    hipLaunchKernelGGL(k_mt_scan_sums<mt_u64>, dim3(1), dim3(MT_SUM_WG), 0, st, A.psums, A.nbp);
    hipLaunchKernelGGL(k_la_emit, grid(npts), dim3(LA_WG), 0, st, A);
  }
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_local_ba_assemble(int cur_kf, int n_nbr, const int32_t* nbr_kf, int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const int32_t* kf_rank, const double* kf_Tcw,
                           const double* kf_K4, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const double* X, const uint8_t* pt_bad,
                           const int32_t* pt_rank, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv, const int32_t* obs_level,
                           const float* inv_level_sigma2, int n_levels, int cap_cam, int cap_pts, int cap_obs, int32_t* counts, int32_t* cam_kf, double* K4,
                           double* poses7, uint8_t* cam_fixed, uint8_t* cam_local, int32_t* lpt_pt, double* pts3, int32_t* lobs_cam, int32_t* lobs_pt, double* lobs_uv,
                           float* lobs_inv_sigma2, int32_t* lobs_src, uint8_t* kf_role, uint8_t* pt_local) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(nkf >= 1 && n_nbr >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_local_ba_assemble: bad count (nkf is >= 1)");
  ORBHIP_REQUIRE(cur_kf >= 0 && cur_kf < nkf, ORBHIP_EINVAL, "orbl_local_ba_assemble: cur_kf out of range");
  ORBHIP_REQUIRE(cap_cam >= 0 && cap_pts >= 0 && cap_obs >= 0, ORBHIP_EINVAL, "orbl_local_ba_assemble: negative capacity");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_local_ba_assemble: n_levels out of range");
  ORBHIP_REQUIRE(kf_id && kf_Tcw && kf_K4 && kf_slot_off && inv_level_sigma2 && counts && kf_role, ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL argument");
  ORBHIP_REQUIRE(n_nbr == 0 || nbr_kf, ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL nbr_kf");
  ORBHIP_REQUIRE(npts == 0 || (X && obs_off && pt_local), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL point argument");
  ORBHIP_REQUIRE(cap_cam == 0 || (cam_kf && K4 && poses7 && cam_fixed && cam_local), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL camera output");
  ORBHIP_REQUIRE(cap_pts == 0 || (lpt_pt && pts3), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL point output");
  ORBHIP_REQUIRE(cap_obs == 0 || (lobs_cam && lobs_pt && lobs_uv && lobs_inv_sigma2 && lobs_src), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL row output");
  static const char E[] = "orbl_local_ba_assemble";
  int nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_REQUIRE(nslots == 0 || kf_slot_pt, ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL kf_slot_pt");
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_uv && obs_level), ORBHIP_EINVAL, "orbl_local_ba_assemble: NULL observation argument");
  ORBHIP_ARG(check_index(E, "nbr_kf", nbr_kf, n_nbr, nkf));
  ORBHIP_ARG(check_index(E, "kf_slot_pt", kf_slot_pt, nslots, npts, true));
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  ORBHIP_ARG(check_index(E, "obs_level", obs_level, nobs, n_levels));
  if (kf_rank) ORBHIP_ARG(check_permutation(E, "kf_rank", kf_rank, nkf));
  if (pt_rank) ORBHIP_ARG(check_permutation(E, "pt_rank", pt_rank, npts));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts, no = (size_t)nobs, cc = (size_t)cap_cam, cp = (size_t)cap_pts, co = (size_t)cap_obs;
  RoundTrip R(W);
  const HostIn<int32_t> d_nbr = R.in(nbr_kf, (size_t)n_nbr), d_id = R.in(kf_id, nk), d_krank = R.in(kf_rank, nk), d_soff = R.csr(kf_slot_off, nk),
                        d_spt = R.in(kf_slot_pt, (size_t)nslots), d_prank = R.in(pt_rank, np), d_ooff = R.csr(obs_off, np), d_okf = R.in(obs_kf, no), d_olvl = R.in(obs_level, no);
  const HostIn<uint8_t> d_kbad = R.in(kf_bad, nk), d_pbad = R.in(pt_bad, np);
  const HostIn<double> d_T = R.in(kf_Tcw, 12 * nk), d_K = R.in(kf_K4, 4 * nk), d_X = R.in(X, 3 * np);
  const HostIn<float> d_uv = R.in(obs_uv, 2 * no), d_isg = R.in(inv_level_sigma2, (size_t)n_levels);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4), o_cam_kf = R.out<int32_t>(cc), o_lpt = R.out<int32_t>(cp), o_ocam = R.out<int32_t>(co), o_opt = R.out<int32_t>(co),
                         o_osrc = R.out<int32_t>(co);
  const HostOut<double> o_K4 = R.out<double>(4 * cc), o_p7 = R.out<double>(7 * cc), o_pts3 = R.out<double>(3 * cp), o_ouv = R.out<double>(2 * co);
  const HostOut<float> o_oisg = R.out<float>(co);
  const HostOut<uint8_t> o_fixed = R.out<uint8_t>(cc), o_local = R.out<uint8_t>(cc), o_role = R.out<uint8_t>(nk), o_ptl = R.out<uint8_t>(np);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(la_workspace(nkf, npts).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_local_ba_assemble_device(cur_kf, n_nbr, d_nbr.dev(), nkf, d_id.dev(), d_kbad.dev(), d_krank.dev(), d_T.dev(), d_K.dev(), nslots, d_soff.dev(), d_spt.dev(), npts,
                                          d_X.dev(), d_pbad.dev(), d_prank.dev(), nobs, d_ooff.dev(), d_okf.dev(), d_uv.dev(), d_olvl.dev(), d_isg.dev(), n_levels, cap_cam,
                                          cap_pts, cap_obs, o_counts.dev(), o_cam_kf.dev(), o_K4.dev(), o_p7.dev(), o_fixed.dev(), o_local.dev(), o_lpt.dev(), o_pts3.dev(),
                                          o_ocam.dev(), o_opt.dev(), o_ouv.dev(), o_oisg.dev(), o_osrc.dev(), o_role.dev(), o_ptl.dev(), o_status.dev(), R.scratch_dev(),
                                          R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 4);
  const size_t ncam = (size_t)o_counts[0], npl = (size_t)o_counts[2], nol = (size_t)o_counts[3];
  if (ncam > cc || npl > cp || nol > co) {
    set_error("orbl_local_ba_assemble: wanted %d cameras, %d points, %d rows; capacities %d, %d, %d", o_counts[0], o_counts[2], o_counts[3], cap_cam, cap_pts, cap_obs);
    return ORBHIP_ECAP;
  }
  // the lists up to their counts: what lies behind them in the caller's arrays is not touched
  R.copy_out(o_cam_kf, cam_kf, ncam); R.copy_out(o_K4, K4, 4 * ncam); R.copy_out(o_p7, poses7, 7 * ncam); R.copy_out(o_fixed, cam_fixed, ncam); R.copy_out(o_local, cam_local, ncam);
  R.copy_out(o_lpt, lpt_pt, npl); R.copy_out(o_pts3, pts3, 3 * npl);
  R.copy_out(o_ocam, lobs_cam, nol); R.copy_out(o_opt, lobs_pt, nol); R.copy_out(o_ouv, lobs_uv, 2 * nol); R.copy_out(o_oisg, lobs_inv_sigma2, nol); R.copy_out(o_osrc, lobs_src, nol);
  R.copy_out(o_role, kf_role, nk); R.copy_out(o_ptl, pt_local, np);
  return 0;
}

int orbl_local_ba_apply_workspace(int nobs, size_t* bytes) {
  ORBHIP_REQUIRE(nobs >= 0 && bytes, ORBHIP_EINVAL, "orbl_local_ba_apply_workspace: bad argument");
  *bytes = orbhip::ap_workspace_bytes(nobs);
  return 0;
}

int orbl_local_ba_apply_device(int ncam, const int32_t* cam_kf, const uint8_t* cam_local, const double* poses7, int npts_local, const int32_t* lpt_pt, const double* pts3,
                               int nobs_local, const int32_t* lobs_src, const uint8_t* obs_erase, int nkf, double* kf_Tcw, double* kf_center, int nslots,
                               const int32_t* kf_slot_off, int32_t* kf_slot_pt, int npts, double* X, uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_ref_kf, int nobs,
                               const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot, const int32_t* obs_level, const int32_t* kf_level0,
                               const float* scale_factors, int n_levels, uint8_t* obs_erased, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts,
                               uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(ncam >= 0 && npts_local >= 0 && nobs_local >= 0 && nkf >= 0 && nslots >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_local_ba_apply: negative count");
  ORBHIP_REQUIRE(counts && workspace, ORBHIP_EINVAL, "orbl_local_ba_apply: NULL counts or workspace");
  ORBHIP_REQUIRE(ncam == 0 || (cam_kf && cam_local && poses7 && kf_Tcw), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL camera argument");
  ORBHIP_REQUIRE(npts_local == 0 || (lpt_pt && pts3 && X), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL local point argument");
  ORBHIP_REQUIRE(nobs_local == 0 || (lobs_src && obs_erase), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL row argument");
  ORBHIP_REQUIRE(nkf == 0 || kf_slot_off, ORBHIP_EINVAL, "orbl_local_ba_apply: NULL kf_slot_off");
  ORBHIP_REQUIRE(nslots == 0 || kf_slot_pt, ORBHIP_EINVAL, "orbl_local_ba_apply: NULL kf_slot_pt");
  ORBHIP_REQUIRE(npts == 0 || (pt_bad && pt_nobs && pt_ref_kf && obs_off), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL point argument");
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_slot && obs_erased), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL observation argument");
  const bool any_nd = normal || min_max || nd_written || scale_factors;
  const bool nd = scale_factors && (npts == 0 || (normal && min_max && nd_written)) && (nobs == 0 || obs_level);      // (no points: no rows to point at)
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_local_ba_apply: the normal / depth arguments are given as a set");
  ORBHIP_REQUIRE(!nd || nkf == 0 || kf_center, ORBHIP_EINVAL, "orbl_local_ba_apply: the normals need kf_center");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_local_ba_apply: n_levels out of range");
  const void* q8[] = {poses7, pts3, kf_Tcw, kf_center, X, normal, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_local_ba_apply: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {cam_kf, lpt_pt, lobs_src, kf_slot_off, kf_slot_pt, pt_nobs, pt_ref_kf, obs_off, obs_kf, obs_slot, obs_level, kf_level0, scale_factors, min_max, counts, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_local_ba_apply: 32-bit arrays must be 4-byte aligned");
  ApArgs A; std::memset(&A, 0, sizeof(A));
  A.ncam = ncam; A.npts_local = npts_local; A.nobs_local = nobs_local; A.nkf = nkf; A.nslots = nslots; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels;
  A.cam_kf = cam_kf; A.cam_local = cam_local; A.poses7 = poses7; A.lpt_pt = lpt_pt; A.pts3 = pts3; A.lobs_src = lobs_src; A.obs_erase = obs_erase;
  A.kf_Tcw = kf_Tcw; A.kf_center = kf_center; A.slot_off = kf_slot_off; A.slot_pt = kf_slot_pt; A.X = X; A.pt_bad = pt_bad; A.pt_nobs = pt_nobs; A.pt_ref_kf = pt_ref_kf;
  A.obs_off = obs_off; A.obs_kf = obs_kf; A.obs_slot = obs_slot; A.obs_level = obs_level; A.kf_level0 = kf_level0; A.scale_factors = scale_factors;
  A.obs_erased = obs_erased; A.counts = counts; A.status = status; A.want = (uint32_t*)workspace;
  if (nd) { A.normal = normal; A.min_max = min_max; A.nd_written = nd_written; }
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 16, st));
  if (nobs > 0) {
    ORBHIP_CHECK_HIP(hipMemsetAsync(workspace, 0xFF, 4 * (size_t)nobs, st));
    ORBHIP_CHECK_HIP(hipMemsetAsync(obs_erased, 0, (size_t)nobs, st));
  }
  if (nd && npts > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(nd_written, 0, (size_t)npts, st));
  auto grid = [](int n) { return dim3((unsigned)((n + LA_WG - 1) / LA_WG)); };
  if (nobs_local > 0 && nobs > 0) hipLaunchKernelGGL(k_ap_mark, grid(nobs_local), dim3(LA_WG), 0, st, A);
  if (npts > 0 && nobs > 0) hipLaunchKernelGGL(k_ap_erase, grid(npts), dim3(LA_WG), 0, st, A);
  if (std::max(ncam, npts_local) > 0) hipLaunchKernelGGL(k_ap_write, grid(std::max(ncam, npts_local)), dim3(LA_WG), 0, st, A);
  if (nd && npts_local > 0 && nobs > 0) hipLaunchKernelGGL(k_ap_normals, grid(npts_local), dim3(LA_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_local_ba_apply(int ncam, const int32_t* cam_kf, const uint8_t* cam_local, const double* poses7, int npts_local, const int32_t* lpt_pt, const double* pts3,
                        int nobs_local, const int32_t* lobs_src, const uint8_t* obs_erase, int nkf, double* kf_Tcw, double* kf_center, const int32_t* kf_slot_off,
                        int32_t* kf_slot_pt, int npts, double* X, uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_ref_kf, const int32_t* obs_off, const int32_t* obs_kf,
                        const int32_t* obs_slot, const int32_t* obs_level, const int32_t* kf_level0, const float* scale_factors, int n_levels, uint8_t* obs_erased,
                        double* normal, float* min_max, uint8_t* nd_written, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(ncam >= 0 && npts_local >= 0 && nobs_local >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_local_ba_apply: negative count");
  ORBHIP_REQUIRE(counts, ORBHIP_EINVAL, "orbl_local_ba_apply: NULL counts");
  ORBHIP_REQUIRE(ncam == 0 || (cam_kf && cam_local && poses7 && kf_Tcw), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL camera argument");
  ORBHIP_REQUIRE(npts_local == 0 || (lpt_pt && pts3 && X), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL local point argument");
  ORBHIP_REQUIRE(nobs_local == 0 || (lobs_src && obs_erase), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL row argument");
  ORBHIP_REQUIRE(nkf == 0 || kf_slot_off, ORBHIP_EINVAL, "orbl_local_ba_apply: NULL kf_slot_off");
  ORBHIP_REQUIRE(npts == 0 || (pt_bad && pt_nobs && pt_ref_kf && obs_off), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL point argument");
  const bool any_nd = normal || min_max || nd_written || scale_factors;
  const bool nd = scale_factors && (npts == 0 || (normal && min_max && nd_written));
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_local_ba_apply: the normal / depth arguments are given as a set");
  ORBHIP_REQUIRE(!nd || nkf == 0 || kf_center, ORBHIP_EINVAL, "orbl_local_ba_apply: the normals need kf_center");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_local_ba_apply: n_levels out of range");
  static const char E[] = "orbl_local_ba_apply";
  int nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_REQUIRE(nslots == 0 || kf_slot_pt, ORBHIP_EINVAL, "orbl_local_ba_apply: NULL kf_slot_pt");
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_slot && obs_erased && (!nd || obs_level)), ORBHIP_EINVAL, "orbl_local_ba_apply: NULL observation argument");
  ORBHIP_ARG(check_index(E, "cam_kf", cam_kf, ncam, nkf));
  ORBHIP_ARG(check_index(E, "lpt_pt", lpt_pt, npts_local, npts));
  ORBHIP_ARG(check_index(E, "lobs_src", lobs_src, nobs_local, nobs));
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  for (int e = 0; e < nobs; e++) {
    const int k = obs_kf[e];
    ORBHIP_REQUIRE(arg_in_range(obs_slot[e], 0, kf_slot_off[k + 1] - kf_slot_off[k]), ORBHIP_EINVAL, "orbl_local_ba_apply: obs_slot names a slot its keyframe does not have");
  }
  for (int c = 0; c < ncam; c++) {
    if (!cam_local[c]) continue;
    const double* s = poses7 + 7 * (size_t)c;
    ORBHIP_REQUIRE(mc_finite(s, 7) && ((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]) + s[6] * s[6] > 0.0, ORBHIP_EINVAL,
                   "orbl_local_ba_apply: a local camera's pose is not finite or its quaternion is zero");
  }
  if (nd) {
    ORBHIP_ARG(check_index(E, "obs_level", obs_level, nobs, n_levels));
    if (kf_level0) ORBHIP_ARG(check_index(E, "kf_level0", kf_level0, nkf, n_levels));
    std::vector<uint8_t> local((size_t)npts, 0);
    for (int j = 0; j < npts_local; j++) local[lpt_pt[j]] = 1;
    const auto read = [&](int p) { return local[p] && obs_off[p] != obs_off[p + 1]; };                  // (else its reference keyframe is not read)
    ORBHIP_ARG(check_index_if(E, "pt_ref_kf", pt_ref_kf, npts, nkf, read));
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts, no = (size_t)nobs, nc = (size_t)ncam, nl = (size_t)npts_local, nr = (size_t)nobs_local;
  RoundTrip R(W);
  const HostOut<double> t_Tcw = R.inout(kf_Tcw, 12 * nk), t_center = R.inout(kf_center, 3 * nk), t_X = R.inout(X, 3 * np);
  const HostOut<int32_t> t_spt = R.inout(kf_slot_pt, (size_t)nslots), t_nobs = R.inout(pt_nobs, np), t_ref = R.inout(pt_ref_kf, np);
  const HostOut<uint8_t> t_bad = R.inout(pt_bad, np);
  const HostIn<int32_t> d_cam = R.in(cam_kf, nc), d_lpt = R.in(lpt_pt, nl), d_src = R.in(lobs_src, nr), d_soff = R.csr(kf_slot_off, nk), d_ooff = R.csr(obs_off, np),
                        d_okf = R.in(obs_kf, no), d_oslot = R.in(obs_slot, no), d_olvl = R.in(nd ? obs_level : nullptr, no), d_l0 = R.in(nd ? kf_level0 : nullptr, nk);
  const HostIn<uint8_t> d_cloc = R.in(cam_local, nc), d_erase = R.in(obs_erase, nr);
  const HostIn<double> d_p7 = R.in(poses7, 7 * nc), d_pts3 = R.in(pts3, 3 * nl);
  const HostIn<float> d_sf = R.in(nd ? scale_factors : nullptr, (size_t)n_levels);
  const HostOut<int32_t> o_counts = R.out<int32_t>(4);
  const HostOut<uint8_t> o_erased = R.out<uint8_t>(no), o_wrote = R.out<uint8_t>(np, nd);
  const HostOut<double> o_normal = R.out<double>(3 * np, nd);
  const HostOut<float> o_mm = R.out<float>(2 * np, nd);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(ap_workspace_bytes(nobs));
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_local_ba_apply_device(ncam, d_cam.dev(), d_cloc.dev(), d_p7.dev(), npts_local, d_lpt.dev(), d_pts3.dev(), nobs_local, d_src.dev(), d_erase.dev(), nkf,
                                       t_Tcw.dev(), t_center.dev(), nslots, d_soff.dev(), t_spt.dev(), npts, t_X.dev(), t_bad.dev(), t_nobs.dev(), t_ref.dev(), nobs,
                                       d_ooff.dev(), d_okf.dev(), d_oslot.dev(), d_olvl.dev(), d_l0.dev(), d_sf.dev(), n_levels, o_erased.dev(), o_normal.dev(), o_mm.dev(),
                                       o_wrote.dev(), o_counts.dev(), o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 4);
  R.copy_out(t_Tcw, kf_Tcw, 12 * nk); R.copy_out(t_center, kf_center, 3 * nk); R.copy_out(t_X, X, 3 * np);
  R.copy_out(t_spt, kf_slot_pt, (size_t)nslots); R.copy_out(t_nobs, pt_nobs, np); R.copy_out(t_ref, pt_ref_kf, np); R.copy_out(t_bad, pt_bad, np);
  R.copy_out(o_erased, obs_erased, no);
  if (nd) {
    R.copy_out(o_wrote, nd_written, np);
    for (size_t p = 0; p < np; p++)
      if (o_wrote[p]) { std::copy_n(&o_normal[3 * p], 3, normal + 3 * p); std::copy_n(&o_mm[2 * p], 2, min_max + 2 * p); }      // (rows of other points are not touched)
  }
  return 0;
}

}  // extern "C"
