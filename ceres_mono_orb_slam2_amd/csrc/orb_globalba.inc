// orb_globalba.inc -- the two halves of CeresOptimizer::BundleAdjustment (GlobalBundleAdjustemnt) around the optimisation, on the flat
// map tables: orbl_global_ba_assemble* turns the keyframe list and the point list into the arguments of ba_solve
// (src/CeresOptimizer.cc:87-176, in the reading csrc/compat/orbslam_dropin.h fixed: cameras by keyframe id, an observer outside the list
// gives no row, a point without rows is left out), and orbl_global_ba_apply* writes the result back (:190-224): SetPose, SetWorldPos and
// UpdateNormalAndDepth (stage 0, Tracking.cc:502), or global_BA_Tcw_ / global_BA_pose_ with their stamps (stage 1, LoopClosing.cc:656).
// Textually included by orb_localmap.hip.  The scan, the row gate, LA_WG and the LA_ST_* status bits it shares with orb_localba.inc come
// from orb_maptable.h.  FP64 throughout, no fused multiply-add (-ffp-contract=off) (DESIGN.md section 2, "GlobalBundleAdjustment on the
// tables").
//
// assemble: every list is an ORDERED compaction; atomics only take order-free minima and integer sums.
//   k_ga_stamp     one lane per list position / point: firstk[k], firstp[p] = the least position that names it (atomicMin), the offset checks
//   k_ga_keys      one lane per ba_kf position: key = (kf_id, position) as one 64-bit word for a camera candidate, all ones otherwise
//   k_ga_rank      workgroup (x, y): the 256 positions of tile x against the key tiles y, y + gridDim.y, ... staged through LDS; the
//                  number of keys below its own is added to below[position] (n^2 compares over the whole device, no bound on the ids)
//   k_ga_cams      one lane per ba_kf position: the camera's row at place below[position], kf_cam, counts[0]
//   k_ga_pscan     one lane per ba_pt position: (rows of the point << 32 | 1) for a point with rows, scanned per workgroup;
//                  k_mt_scan_sums scans the workgroup sums;   k_ga_emit: the points and their rows, pt_idx, counts[1..2]
// apply:
//   k_gp_stamp     one lane per camera / problem point: cam_of[k], pt_of[p] = the last place that names it (atomicMax), the pose check
//   k_gp_write     one lane per keyframe / point: stage 0 the pose with its centre and the position, stage 1 the gba arrays and flags
//   k_gp_normals   one lane per point (stage 0): the normal / depth walk (mt_normal_depth) over the NEW centres
// Outputs are written with vector stores only.
#include "orb_maptable.h"

namespace orbhip {

#define GA_ST_REPEAT 1024u        /* assemble: a point twice in ba_pt (its first position counts) */
#define GA_ST_POSE 2048u          /* apply: a pose that is not finite or has |q| = 0 (the camera is not written) */
#define GA_RANK_Y 64              /* k_ga_rank: at most this many workgroups share the key tiles of one position tile */

struct GaArgs {
  int n_ba_kf, n_ba_pt, nkf, npts, nobs, n_levels, is_robust, cap_cam, cap_pts, cap_obs, nbp;
  const int32_t* ba_kf; const int32_t* ba_pt; const int32_t* kf_id; const uint8_t* kf_bad; const double* kf_Tcw; const double* kf_K4;
  const double* X; const uint8_t* pt_bad; const int32_t* obs_off; const int32_t* obs_kf; const float* obs_uv; const int32_t* obs_level; const float* inv_level_sigma2;
  int32_t* counts; int32_t* cam_kf; int32_t* kf_cam; double* K4; double* poses7; uint8_t* cam_fixed; int32_t* gpt_pt; int32_t* pt_idx; double* pts3;
  int32_t* gobs_cam; int32_t* gobs_pt; double* gobs_uv; double* gobs_weight; uint8_t* gobs_robust; int32_t* gobs_src; uint32_t* status;
  // workspace: firstk[nkf] | firstp[npts] (both set to all ones per call) | key[n_ba_kf] | below[n_ba_kf] | meta[4] (both cleared per call) |
  // pscan[n_ba_pt] | psums[nbp + 1]
  uint32_t* firstk; uint32_t* firstp; mt_u64* key; int32_t* below; int32_t* meta; mt_u64 *pscan, *psums;
};

__device__ __forceinline__ int ga_kf_at(const GaArgs& a, int q) { return a.ba_kf ? a.ba_kf[q] : q; }
__device__ __forceinline__ int ga_pt_at(const GaArgs& a, int r) { return a.ba_pt ? a.ba_pt[r] : r; }

__global__ __launch_bounds__(LA_WG) void k_ga_stamp(GaArgs a) {
  const int i = blockIdx.x * LA_WG + threadIdx.x;
  if (i < a.n_ba_kf) {
    const int k = ga_kf_at(a, i);
    if (k < 0 || k >= a.nkf) mt_flag(a.status, LA_ST_KF);
    else atomicMin(&a.firstk[k], (uint32_t)i);
  }
  if (i < a.n_ba_pt) {
    const int p = ga_pt_at(a, i);
    if (p < 0 || p >= a.npts) mt_flag(a.status, LA_ST_PT);
    else if (atomicMin(&a.firstp[p], (uint32_t)i) != LA_NONE) mt_flag(a.status, GA_ST_REPEAT);      // (whichever of the two arrives second sees the other)
  }
  if (i < a.npts) {
    int lo, hi;
    if (!mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, LA_ST_OFFSETS);
  }
}

// the keyframe of list position q when that position is where the list first names it and it is not bad, else -1 (:89, dropin :807-808)
__device__ __forceinline__ int ga_cand_at(const GaArgs& a, int q) {
  const int k = ga_kf_at(a, q);
  if (k < 0 || k >= a.nkf || a.firstk[k] != (uint32_t)q) return -1;
  return (a.kf_bad && a.kf_bad[k]) ? -1 : k;
}

__global__ __launch_bounds__(LA_WG) void k_ga_keys(GaArgs a) {
  const int q = blockIdx.x * LA_WG + threadIdx.x;
  const int k = q < a.n_ba_kf ? ga_cand_at(a, q) : -1;
  // (kf_id, position) in one word that compares as the pair does: the id with its sign bit turned (int32 order), then the position
  if (q < a.n_ba_kf) a.key[q] = k >= 0 ? (((mt_u64)((uint32_t)a.kf_id[k] ^ 0x80000000u) << 32) | (mt_u64)(uint32_t)q) : ~0ull;
  const uint64_t m = __ballot(k >= 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.meta[0], (int)__popcll(m));
}

__global__ __launch_bounds__(LA_WG) void k_ga_rank(GaArgs a) {
  __shared__ mt_u64 tile[LA_WG];
  const int q = blockIdx.x * LA_WG + threadIdx.x;
  const mt_u64 own = q < a.n_ba_kf ? a.key[q] : ~0ull;
  const int nt = (a.n_ba_kf + LA_WG - 1) / LA_WG;
  int below = 0;
  for (int t = blockIdx.y; t < nt; t += gridDim.y) {                           // (workgroup-uniform)
    const int s = t * LA_WG + (int)threadIdx.x;
    tile[threadIdx.x] = s < a.n_ba_kf ? a.key[s] : ~0ull;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < LA_WG; j++) below += tile[j] < own ? 1 : 0;             // (every lane reads the same word: an LDS broadcast)
    __syncthreads();
  }
  if (own != ~0ull && below) atomicAdd(&a.below[q], below);                     // (an integer sum: the same whatever the arrival order)
}

__global__ __launch_bounds__(LA_WG) void k_ga_cams(GaArgs a) {
  const int q = blockIdx.x * LA_WG + threadIdx.x;
  if (q == 0) {
    const int ncam = a.meta[0];
    a.counts[0] = ncam;
    if (ncam > a.cap_cam) mt_flag(a.status, LA_ST_CAP_CAM);
  }
  if (q >= a.n_ba_kf) return;
  const int k = ga_cand_at(a, q);
  if (k < 0) return;
  const int c = a.below[q];
  a.kf_cam[k] = c;
  if (c >= a.cap_cam) return;
  mt_pose34_to_pose7(a.kf_Tcw + 12 * (size_t)k, a.poses7 + 7 * (size_t)c);
  for (int j = 0; j < 4; j++) a.K4[4 * (size_t)c + j] = a.kf_K4[4 * (size_t)k + j];
  a.cam_kf[c] = k;
  a.cam_fixed[c] = a.kf_id[k] == 0 ? 1 : 0;                                    // (:115-120)
}

// whether observation e becomes a row: its keyframe is not bad and has a camera (:142 - the id gate is implied - and dropin :831)
__device__ __forceinline__ bool ga_row_ok(const GaArgs& a, int e) {
  return mt_row_ok(a.obs_kf, a.obs_level, e, a.nkf, a.n_levels, a.kf_bad, a.kf_cam, a.status, LA_ST_KF, LA_ST_LEVEL);
}

// the point of list position r when that position is where the list first names it, it is not bad and its list is in range, else -1;
// *rows = how many of its observations become rows
__device__ __forceinline__ int ga_point_at(const GaArgs& a, int r, int* lo, int* hi, int* rows) {
  *rows = 0;
  const int p = ga_pt_at(a, r);
  if (p < 0 || p >= a.npts || a.firstp[p] != (uint32_t)r || (a.pt_bad && a.pt_bad[p])) return -1;
  if (!mt_range(a.obs_off, p, a.nobs, lo, hi)) return -1;
  int n = 0;
  for (int e = *lo; e < *hi; e++) n += ga_row_ok(a, e) ? 1 : 0;
  *rows = n;
  return p;
}

__global__ __launch_bounds__(LA_WG) void k_ga_pscan(GaArgs a) {
  __shared__ mt_u64 sw[LA_WG / 64];
  const int r = blockIdx.x * LA_WG + threadIdx.x;
  int lo, hi, rows = 0;
  if (r < a.n_ba_pt) (void)ga_point_at(a, r, &lo, &hi, &rows);
  const mt_u64 v = rows > 0 ? (((mt_u64)(uint32_t)rows << 32) | 1ull) : 0ull;   // (rows, points): a point without rows is left out (:170-172)
  mt_u64 tot;
  const mt_u64 ex = mt_block_excl<LA_WG>(v, sw, &tot);
  if (r < a.n_ba_pt) a.pscan[r] = ex;
  if (threadIdx.x == 0) a.psums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(LA_WG) void k_ga_emit(GaArgs a) {
  const int r = blockIdx.x * LA_WG + threadIdx.x;
  if (r >= a.n_ba_pt) return;
  if (r == 0) {
    const mt_u64 t = a.psums[a.nbp];
    const int np = (int)(uint32_t)t, no = (int)(t >> 32);
    a.counts[1] = np; a.counts[2] = no;
    if (np > a.cap_pts) mt_flag(a.status, LA_ST_CAP_PTS);
    if (no > a.cap_obs) mt_flag(a.status, LA_ST_CAP_OBS);
  }
  int lo, hi, rows;
  const int p = ga_point_at(a, r, &lo, &hi, &rows);
  if (p < 0 || rows == 0) return;
  const mt_u64 at = a.pscan[r] + a.psums[blockIdx.x];
  const int j = (int)(uint32_t)at;
  int row = (int)(at >> 32);
  a.pt_idx[p] = j;
  if (j < a.cap_pts) {
    a.gpt_pt[j] = p;
    for (int q = 0; q < 3; q++) a.pts3[3 * (size_t)j + q] = a.X[3 * (size_t)p + q];
  }
  for (int e = lo; e < hi; e++) {
    if (!ga_row_ok(a, e)) continue;
    if (row < a.cap_obs) {
      a.gobs_cam[row] = a.kf_cam[a.obs_kf[e]]; a.gobs_pt[row] = j;
      a.gobs_uv[2 * (size_t)row] = (double)a.obs_uv[2 * (size_t)e]; a.gobs_uv[2 * (size_t)row + 1] = (double)a.obs_uv[2 * (size_t)e + 1];
      a.gobs_weight[row] = (double)a.inv_level_sigma2[a.obs_level[e]];
      a.gobs_robust[row] = a.is_robust ? 1 : 0;
      a.gobs_src[row] = e;
    }
    row++;
  }
}

// workspace sections, each rounded up to 256 bytes; [0, ones) is set to all ones and [zeros, zeros_end) is cleared by every call
struct GaWs { size_t firstk, firstp, ones, key, zeros, below, meta, zeros_end, pscan, psums, total; int nbp; };
static GaWs ga_workspace(int nkf, int npts, int n_ba_kf, int n_ba_pt) {
  GaWs w; Carve ws;
  w.nbp = (n_ba_pt + LA_WG - 1) / LA_WG;
  w.firstk = ws.take(4 * (size_t)nkf); w.firstp = ws.take(4 * (size_t)npts);
  w.ones = ws.total;
  w.key = ws.take(8 * (size_t)n_ba_kf);
  w.zeros = ws.total;
  w.below = ws.take(4 * (size_t)n_ba_kf); w.meta = ws.take(16);
  w.zeros_end = ws.total;
  w.pscan = ws.take(8 * (size_t)n_ba_pt); w.psums = ws.take(8 * ((size_t)w.nbp + 1));
  w.total = ws.total;
  return w;
}

// ---------------------------------------------------------------------------------------------------------- write-back
struct GpArgs {
  int ncam, npts_ba, stage, nkf, npts, nobs, n_levels;
  const int32_t* cam_kf; const double* poses7; const int32_t* gpt_pt; const double* pts3; const uint8_t* kf_bad; const uint8_t* pt_bad;
  double* kf_Tcw; double* kf_center; double* X; double* kf_gba_Tcw; uint8_t* kf_in_gba; double* pt_gba_X; uint8_t* pt_in_gba;
  const int32_t* pt_ref_kf; const int32_t* obs_off; const int32_t* obs_kf; const int32_t* ref_level; const float* scale_factors;
  double* normal; float* min_max; uint8_t* nd_written; int32_t* counts; uint32_t* status;
  int32_t* cam_of; int32_t* pt_of;        // workspace: cam_of[nkf] | pt_of[npts] (set to all ones per call)
};

__global__ __launch_bounds__(LA_WG) void k_gp_stamp(GpArgs a) {
  const int i = blockIdx.x * LA_WG + threadIdx.x;
  if (i < a.ncam) {
    const int k = a.cam_kf[i];
    const double* s = a.poses7 + 7 * (size_t)i;
    bool fin = true;
    for (int q = 0; q < 7; q++) fin = fin && isfinite(s[q]);
    if (k < 0 || k >= a.nkf) mt_flag(a.status, LA_ST_KF);
    else if (!fin || !(((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]) + s[6] * s[6] > 0.0)) mt_flag(a.status, GA_ST_POSE);
    else if (atomicMax(&a.cam_of[k], i) != -1) mt_flag(a.status, LA_ST_KF);    // (a keyframe listed twice: its last camera counts)
  }
  if (i < a.npts_ba) {
    const int p = a.gpt_pt[i];
    if (p < 0 || p >= a.npts) mt_flag(a.status, LA_ST_PT);
    else if (atomicMax(&a.pt_of[p], i) != -1) mt_flag(a.status, LA_ST_PT);      // (a point listed twice: its last place counts)
  }
}

__global__ __launch_bounds__(LA_WG) void k_gp_write(GpArgs a) {
  const int i = blockIdx.x * LA_WG + threadIdx.x;
  int c = -1, j = -1;
  if (i < a.nkf) {
    c = a.cam_of[i];
    if (c >= 0 && a.kf_bad && a.kf_bad[i]) c = -1;                              // (:193: the keyframe turned bad since)
    if (a.stage) a.kf_in_gba[i] = c >= 0 ? 1 : 0;
    if (c >= 0) {                                                              // (:199-204) stage 1 keeps the pose aside: no centre
      double T[12];
      mt_pose7_to_pose34(a.poses7 + 7 * (size_t)c, T);
      mt_set_pose(a.stage ? a.kf_gba_Tcw : a.kf_Tcw, a.stage ? nullptr : a.kf_center, i, T);
    }
  }
  if (i < a.npts) {
    j = a.pt_of[i];
    if (j >= 0 && a.pt_bad && a.pt_bad[i]) j = -1;                              // (:214)
    if (a.stage) a.pt_in_gba[i] = j >= 0 ? 1 : 0;
    else if (a.nd_written) a.nd_written[i] = 0;
    if (j >= 0) {                                                              // (:217-223)
      double* o = (a.stage ? a.pt_gba_X : a.X) + 3 * (size_t)i;
      for (int r = 0; r < 3; r++) o[r] = a.pts3[3 * (size_t)j + r];
    }
  }
  const uint64_t mc = __ballot(c >= 0), mp = __ballot(j >= 0);
  if ((threadIdx.x & 63) == 0) {
    if (mc) atomicAdd(&a.counts[0], (int)__popcll(mc));
    if (mp) atomicAdd(&a.counts[1], (int)__popcll(mp));
  }
}

__global__ __launch_bounds__(LA_WG) void k_gp_normals(GpArgs a) {
  const int p = blockIdx.x * LA_WG + threadIdx.x;
  int wrote = 0;
  int lo = 0, hi = 0;
  if (p < a.npts && a.pt_of[p] >= 0 && !(a.pt_bad && a.pt_bad[p])) {
    // UpdateNormalAndDepth (:219): every SetPose precedes the point loop, so every centre is the new one
    if (!mt_range(a.obs_off, p, a.nobs, &lo, &hi)) mt_flag(a.status, LA_ST_OFFSETS);
    if (lo < hi) {
      const int r = a.pt_ref_kf[p], lvl = a.ref_level[p];
      if (r < 0 || r >= a.nkf) { if (r != -1) mt_flag(a.status, LA_ST_KF); }      // (-1: a point without a reference keyframe gets no normal)
      else if (lvl < 0 || lvl >= a.n_levels) mt_flag(a.status, LA_ST_LEVEL);
      else {
        const int res = mt_normal_depth(a.obs_kf, lo, hi, a.nkf, a.kf_center, a.X[3 * (size_t)p], a.X[3 * (size_t)p + 1], a.X[3 * (size_t)p + 2], r, lvl, a.scale_factors,
                                        a.n_levels, a.normal + 3 * (size_t)p, a.min_max + 2 * (size_t)p);
        if (res == MT_ND_KF) mt_flag(a.status, LA_ST_KF);
        if (res == MT_ND_OK) { a.nd_written[p] = 1; wrote = 1; }
      }
    }
  }
  const uint64_t m = __ballot(wrote != 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts[2], (int)__popcll(m));
}

struct GpWs { size_t cam_of, pt_of, total; };
static GpWs gp_workspace(int nkf, int npts) {
  GpWs w; Carve ws;
  w.cam_of = ws.take(4 * (size_t)nkf); w.pt_of = ws.take(4 * (size_t)npts);
  w.total = ws.total > 0 ? ws.total : 256;
  return w;
}

}  // namespace orbhip

extern "C" {

int orbl_global_ba_assemble_workspace(int nkf, int npts, int n_ba_kf, int n_ba_pt, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && npts >= 0 && n_ba_kf >= 0 && n_ba_pt >= 0 && bytes, ORBHIP_EINVAL, "orbl_global_ba_assemble_workspace: bad argument");
  *bytes = orbhip::ga_workspace(nkf, npts, n_ba_kf, n_ba_pt).total;
  return 0;
}

int orbl_global_ba_assemble_device(int n_ba_kf, const int32_t* ba_kf, int n_ba_pt, const int32_t* ba_pt, int nkf, const int32_t* kf_id, const uint8_t* kf_bad,
                                   const double* kf_Tcw, const double* kf_K4, int npts, const double* X, const uint8_t* pt_bad, int nobs, const int32_t* obs_off,
                                   const int32_t* obs_kf, const float* obs_uv, const int32_t* obs_level, const float* inv_level_sigma2, int n_levels, int is_robust,
                                   int cap_cam, int cap_pts, int cap_obs, int32_t* counts, int32_t* cam_kf, int32_t* kf_cam, double* K4, double* poses7, uint8_t* cam_fixed,
                                   int32_t* gpt_pt, int32_t* pt_idx, double* pts3, int32_t* gobs_cam, int32_t* gobs_pt, double* gobs_uv, double* gobs_weight,
                                   uint8_t* gobs_robust, int32_t* gobs_src, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(n_ba_kf >= 0 && n_ba_pt >= 0 && nkf >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_global_ba_assemble: negative count");
  ORBHIP_REQUIRE(cap_cam >= 0 && cap_pts >= 0 && cap_obs >= 0, ORBHIP_EINVAL, "orbl_global_ba_assemble: negative capacity");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_global_ba_assemble: n_levels out of range");
  ORBHIP_REQUIRE(inv_level_sigma2 && counts && workspace, ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL argument");
  ORBHIP_REQUIRE(ba_kf || n_ba_kf == 0 || n_ba_kf == nkf, ORBHIP_EINVAL, "orbl_global_ba_assemble: a NULL ba_kf stands for all nkf keyframes (or an empty list)");
  ORBHIP_REQUIRE(ba_pt || n_ba_pt == 0 || n_ba_pt == npts, ORBHIP_EINVAL, "orbl_global_ba_assemble: a NULL ba_pt stands for all npts points (or an empty list)");
  ORBHIP_REQUIRE(nkf == 0 || (kf_id && kf_Tcw && kf_K4 && kf_cam), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL keyframe argument");
  ORBHIP_REQUIRE(npts == 0 || (X && obs_off && pt_idx), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL point argument");
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_uv && obs_level), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL observation argument");
  ORBHIP_REQUIRE(cap_cam == 0 || (cam_kf && K4 && poses7 && cam_fixed), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL camera output");
  ORBHIP_REQUIRE(cap_pts == 0 || (gpt_pt && pts3), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL point output");
  ORBHIP_REQUIRE(cap_obs == 0 || (gobs_cam && gobs_pt && gobs_uv && gobs_weight && gobs_robust && gobs_src), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL row output");
  const void* q8[] = {kf_Tcw, kf_K4, X, K4, poses7, pts3, gobs_uv, gobs_weight, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_global_ba_assemble: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {ba_kf, ba_pt, kf_id, obs_off, obs_kf, obs_uv, obs_level, inv_level_sigma2, counts, cam_kf, kf_cam, gpt_pt, pt_idx, gobs_cam, gobs_pt, gobs_src, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_global_ba_assemble: 32-bit arrays must be 4-byte aligned");
  const GaWs ws = ga_workspace(nkf, npts, n_ba_kf, n_ba_pt);
  uint8_t* wb = (uint8_t*)workspace;
  GaArgs A; std::memset(&A, 0, sizeof(A));
  A.n_ba_kf = n_ba_kf; A.n_ba_pt = n_ba_pt; A.nkf = nkf; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels; A.is_robust = is_robust ? 1 : 0;
  A.cap_cam = cap_cam; A.cap_pts = cap_pts; A.cap_obs = cap_obs; A.nbp = ws.nbp;
  A.ba_kf = ba_kf; A.ba_pt = ba_pt; A.kf_id = kf_id; A.kf_bad = kf_bad; A.kf_Tcw = kf_Tcw; A.kf_K4 = kf_K4; A.X = X; A.pt_bad = pt_bad;
  A.obs_off = obs_off; A.obs_kf = obs_kf; A.obs_uv = obs_uv; A.obs_level = obs_level; A.inv_level_sigma2 = inv_level_sigma2;
  A.counts = counts; A.cam_kf = cam_kf; A.kf_cam = kf_cam; A.K4 = K4; A.poses7 = poses7; A.cam_fixed = cam_fixed; A.gpt_pt = gpt_pt; A.pt_idx = pt_idx; A.pts3 = pts3;
  A.gobs_cam = gobs_cam; A.gobs_pt = gobs_pt; A.gobs_uv = gobs_uv; A.gobs_weight = gobs_weight; A.gobs_robust = gobs_robust; A.gobs_src = gobs_src; A.status = status;
  A.firstk = (uint32_t*)(wb + ws.firstk); A.firstp = (uint32_t*)(wb + ws.firstp); A.key = (mt_u64*)(wb + ws.key); A.below = (int32_t*)(wb + ws.below);
  A.meta = (int32_t*)(wb + ws.meta); A.pscan = (mt_u64*)(wb + ws.pscan); A.psums = (mt_u64*)(wb + ws.psums);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 12, st));
  if (ws.ones > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0xFF, ws.ones, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.zeros, 0, ws.zeros_end - ws.zeros, st));
  if (nkf > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(kf_cam, 0xFF, 4 * (size_t)nkf, st));
  if (npts > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(pt_idx, 0xFF, 4 * (size_t)npts, st));
  auto grid = [](int n) { return dim3((unsigned)((n + LA_WG - 1) / LA_WG)); };
  const int n_stamp = std::max(std::max(n_ba_kf, n_ba_pt), npts);
  if (n_stamp > 0) hipLaunchKernelGGL(k_ga_stamp, grid(n_stamp), dim3(LA_WG), 0, st, A);
  if (n_ba_kf > 0 && nkf > 0) {
    const unsigned nt = (unsigned)((n_ba_kf + LA_WG - 1) / LA_WG);
    hipLaunchKernelGGL(k_ga_keys, dim3(nt), dim3(LA_WG), 0, st, A);
    hipLaunchKernelGGL(k_ga_rank, dim3(nt, std::min(nt, (unsigned)GA_RANK_Y)), dim3(LA_WG), 0, st, A);
    hipLaunchKernelGGL(k_ga_cams, dim3(nt), dim3(LA_WG), 0, st, A);
  }
  if (n_ba_pt > 0 && npts > 0) {
    hipLaunchKernelGGL(k_ga_pscan, grid(n_ba_pt), dim3(LA_WG), 0, st, A);
    hipLaunchKernelGGL(k_mt_scan_sums<mt_u64>, dim3(1), dim3(MT_SUM_WG), 0, st, A.psums, A.nbp);
    hipLaunchKernelGGL(k_ga_emit, grid(n_ba_pt), dim3(LA_WG), 0, st, A);
  }
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_global_ba_assemble(int n_ba_kf, const int32_t* ba_kf, int n_ba_pt, const int32_t* ba_pt, int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const double* kf_Tcw,
                            const double* kf_K4, int npts, const double* X, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv,
                            const int32_t* obs_level, const float* inv_level_sigma2, int n_levels, int is_robust, int cap_cam, int cap_pts, int cap_obs, int32_t* counts,
                            int32_t* cam_kf, int32_t* kf_cam, double* K4, double* poses7, uint8_t* cam_fixed, int32_t* gpt_pt, int32_t* pt_idx, double* pts3,
                            int32_t* gobs_cam, int32_t* gobs_pt, double* gobs_uv, double* gobs_weight, uint8_t* gobs_robust, int32_t* gobs_src) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(n_ba_kf >= 0 && n_ba_pt >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_global_ba_assemble: negative count");
  ORBHIP_REQUIRE(cap_cam >= 0 && cap_pts >= 0 && cap_obs >= 0, ORBHIP_EINVAL, "orbl_global_ba_assemble: negative capacity");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_global_ba_assemble: n_levels out of range");
  ORBHIP_REQUIRE(inv_level_sigma2 && counts, ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL argument");
  ORBHIP_REQUIRE(ba_kf || n_ba_kf == 0 || n_ba_kf == nkf, ORBHIP_EINVAL, "orbl_global_ba_assemble: a NULL ba_kf stands for all nkf keyframes (or an empty list)");
  ORBHIP_REQUIRE(ba_pt || n_ba_pt == 0 || n_ba_pt == npts, ORBHIP_EINVAL, "orbl_global_ba_assemble: a NULL ba_pt stands for all npts points (or an empty list)");
  ORBHIP_REQUIRE(nkf == 0 || (kf_id && kf_Tcw && kf_K4 && kf_cam), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL keyframe argument");
  ORBHIP_REQUIRE(npts == 0 || (X && obs_off && pt_idx), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL point argument");
  ORBHIP_REQUIRE(cap_cam == 0 || (cam_kf && K4 && poses7 && cam_fixed), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL camera output");
  ORBHIP_REQUIRE(cap_pts == 0 || (gpt_pt && pts3), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL point output");
  ORBHIP_REQUIRE(cap_obs == 0 || (gobs_cam && gobs_pt && gobs_uv && gobs_weight && gobs_robust && gobs_src), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL row output");
  static const char E[] = "orbl_global_ba_assemble";
  int nobs = 0;
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_uv && obs_level), ORBHIP_EINVAL, "orbl_global_ba_assemble: NULL observation argument");
  if (ba_kf) ORBHIP_ARG(check_index(E, "ba_kf", ba_kf, n_ba_kf, nkf));
  if (ba_pt) ORBHIP_ARG(check_listed_once(E, "ba_pt", ba_pt, n_ba_pt, npts));      // (Map holds a std::set: a repeat is a caller's mistake)
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  ORBHIP_ARG(check_index(E, "obs_level", obs_level, nobs, n_levels));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts, no = (size_t)nobs, cc = (size_t)cap_cam, cp = (size_t)cap_pts, co = (size_t)cap_obs;
  RoundTrip R(W);
  const HostIn<int32_t> d_bkf = R.in(ba_kf, (size_t)n_ba_kf), d_bpt = R.in(ba_pt, (size_t)n_ba_pt), d_id = R.in(kf_id, nk), d_ooff = R.csr(obs_off, np),
                        d_okf = R.in(obs_kf, no), d_olvl = R.in(obs_level, no);
  const HostIn<uint8_t> d_kbad = R.in(kf_bad, nk), d_pbad = R.in(pt_bad, np);
  const HostIn<double> d_T = R.in(kf_Tcw, 12 * nk), d_K = R.in(kf_K4, 4 * nk), d_X = R.in(X, 3 * np);
  const HostIn<float> d_uv = R.in(obs_uv, 2 * no), d_isg = R.in(inv_level_sigma2, (size_t)n_levels);
  const HostOut<int32_t> o_counts = R.out<int32_t>(3), o_cam_kf = R.out<int32_t>(cc), o_kf_cam = R.out<int32_t>(nk, nkf > 0), o_gpt = R.out<int32_t>(cp),
                         o_pidx = R.out<int32_t>(np, npts > 0), o_ocam = R.out<int32_t>(co), o_opt = R.out<int32_t>(co), o_osrc = R.out<int32_t>(co);
  const HostOut<double> o_K4 = R.out<double>(4 * cc), o_p7 = R.out<double>(7 * cc), o_pts3 = R.out<double>(3 * cp), o_ouv = R.out<double>(2 * co), o_ow = R.out<double>(co);
  const HostOut<uint8_t> o_fixed = R.out<uint8_t>(cc), o_orob = R.out<uint8_t>(co);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(ga_workspace(nkf, npts, n_ba_kf, n_ba_pt).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_global_ba_assemble_device(n_ba_kf, d_bkf.dev(), n_ba_pt, d_bpt.dev(), nkf, d_id.dev(), d_kbad.dev(), d_T.dev(), d_K.dev(), npts, d_X.dev(), d_pbad.dev(), nobs,
                                           d_ooff.dev(), d_okf.dev(), d_uv.dev(), d_olvl.dev(), d_isg.dev(), n_levels, is_robust, cap_cam, cap_pts, cap_obs, o_counts.dev(),
                                           o_cam_kf.dev(), o_kf_cam.dev(), o_K4.dev(), o_p7.dev(), o_fixed.dev(), o_gpt.dev(), o_pidx.dev(), o_pts3.dev(), o_ocam.dev(),
                                           o_opt.dev(), o_ouv.dev(), o_ow.dev(), o_orob.dev(), o_osrc.dev(), o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 3);
  const size_t ncam = (size_t)o_counts[0], npb = (size_t)o_counts[1], nob = (size_t)o_counts[2];
  if (ncam > cc || npb > cp || nob > co) {
    set_error("orbl_global_ba_assemble: wanted %d cameras, %d points, %d rows; capacities %d, %d, %d", o_counts[0], o_counts[1], o_counts[2], cap_cam, cap_pts, cap_obs);
    return ORBHIP_ECAP;
  }
  // the lists up to their counts: what lies behind them in the caller's arrays is not touched
  R.copy_out(o_cam_kf, cam_kf, ncam); R.copy_out(o_K4, K4, 4 * ncam); R.copy_out(o_p7, poses7, 7 * ncam); R.copy_out(o_fixed, cam_fixed, ncam);
  R.copy_out(o_gpt, gpt_pt, npb); R.copy_out(o_pts3, pts3, 3 * npb);
  R.copy_out(o_ocam, gobs_cam, nob); R.copy_out(o_opt, gobs_pt, nob); R.copy_out(o_ouv, gobs_uv, 2 * nob); R.copy_out(o_ow, gobs_weight, nob);
  R.copy_out(o_orob, gobs_robust, nob); R.copy_out(o_osrc, gobs_src, nob);
  R.copy_out(o_kf_cam, kf_cam, nk); R.copy_out(o_pidx, pt_idx, np);
  return 0;
}

int orbl_global_ba_apply_workspace(int nkf, int npts, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && npts >= 0 && bytes, ORBHIP_EINVAL, "orbl_global_ba_apply_workspace: bad argument");
  *bytes = orbhip::gp_workspace(nkf, npts).total;
  return 0;
}

int orbl_global_ba_apply_device(int ncam, const int32_t* cam_kf, const double* poses7, int npts_ba, const int32_t* gpt_pt, const double* pts3, int stage, int nkf,
                                const uint8_t* kf_bad, double* kf_Tcw, double* kf_center, int npts, double* X, const uint8_t* pt_bad, double* kf_gba_Tcw, uint8_t* kf_in_gba,
                                double* pt_gba_X, uint8_t* pt_in_gba, const int32_t* pt_ref_kf, int nobs, const int32_t* obs_off, const int32_t* obs_kf,
                                const int32_t* ref_level, const float* scale_factors, int n_levels, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts,
                                uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(ncam >= 0 && npts_ba >= 0 && nkf >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_global_ba_apply: negative count");
  ORBHIP_REQUIRE(stage == 0 || stage == 1, ORBHIP_EINVAL, "orbl_global_ba_apply: stage is 0 or 1");
  ORBHIP_REQUIRE(counts && workspace, ORBHIP_EINVAL, "orbl_global_ba_apply: NULL counts or workspace");
  ORBHIP_REQUIRE(ncam == 0 || (cam_kf && poses7), ORBHIP_EINVAL, "orbl_global_ba_apply: NULL camera argument");
  ORBHIP_REQUIRE(npts_ba == 0 || (gpt_pt && pts3), ORBHIP_EINVAL, "orbl_global_ba_apply: NULL problem point argument");
  if (stage == 0) {
    ORBHIP_REQUIRE(nkf == 0 || kf_Tcw, ORBHIP_EINVAL, "orbl_global_ba_apply: stage 0 needs kf_Tcw");
    ORBHIP_REQUIRE(npts == 0 || X, ORBHIP_EINVAL, "orbl_global_ba_apply: stage 0 needs X");
  } else {
    ORBHIP_REQUIRE(nkf == 0 || (kf_gba_Tcw && kf_in_gba), ORBHIP_EINVAL, "orbl_global_ba_apply: stage 1 needs kf_gba_Tcw and kf_in_gba");
    ORBHIP_REQUIRE(npts == 0 || (pt_gba_X && pt_in_gba), ORBHIP_EINVAL, "orbl_global_ba_apply: stage 1 needs pt_gba_X and pt_in_gba");
  }
  const bool any_nd = pt_ref_kf || obs_off || obs_kf || ref_level || scale_factors || normal || min_max || nd_written;
  const bool nd = pt_ref_kf && obs_off && ref_level && scale_factors && normal && min_max && nd_written && (nobs == 0 || obs_kf);
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_global_ba_apply: the normal / depth arguments are given as a set");
  const bool run_nd = nd && stage == 0;
  ORBHIP_REQUIRE(!run_nd || nkf == 0 || kf_center, ORBHIP_EINVAL, "orbl_global_ba_apply: the normals need kf_center");
  ORBHIP_REQUIRE(!run_nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_global_ba_apply: n_levels out of range");
  const void* q8[] = {poses7, pts3, kf_Tcw, kf_center, X, kf_gba_Tcw, pt_gba_X, normal, workspace};
  for (const void* q : q8) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_global_ba_apply: 64-bit arrays and the workspace must be 8-byte aligned");
  const void* q4[] = {cam_kf, gpt_pt, pt_ref_kf, obs_off, obs_kf, ref_level, scale_factors, min_max, counts, status};
  for (const void* q : q4) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_global_ba_apply: 32-bit arrays must be 4-byte aligned");
  const GpWs ws = gp_workspace(nkf, npts);
  uint8_t* wb = (uint8_t*)workspace;
  GpArgs A; std::memset(&A, 0, sizeof(A));
  A.ncam = ncam; A.npts_ba = npts_ba; A.stage = stage; A.nkf = nkf; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels;
  A.cam_kf = cam_kf; A.poses7 = poses7; A.gpt_pt = gpt_pt; A.pts3 = pts3; A.kf_bad = kf_bad; A.pt_bad = pt_bad;
  if (stage == 0) { A.kf_Tcw = kf_Tcw; A.kf_center = kf_center; A.X = X; }
  else { A.kf_gba_Tcw = kf_gba_Tcw; A.kf_in_gba = kf_in_gba; A.pt_gba_X = pt_gba_X; A.pt_in_gba = pt_in_gba; }
  if (run_nd) {
    A.pt_ref_kf = pt_ref_kf; A.obs_off = obs_off; A.obs_kf = obs_kf; A.ref_level = ref_level; A.scale_factors = scale_factors;
    A.normal = normal; A.min_max = min_max; A.nd_written = nd_written;
  }
  A.counts = counts; A.status = status; A.cam_of = (int32_t*)(wb + ws.cam_of); A.pt_of = (int32_t*)(wb + ws.pt_of);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(counts, 0, 12, st));
  if (nkf + npts > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0xFF, ws.pt_of + 4 * (size_t)npts, st));
  auto grid = [](int n) { return dim3((unsigned)((n + LA_WG - 1) / LA_WG)); };
  if (std::max(ncam, npts_ba) > 0) hipLaunchKernelGGL(k_gp_stamp, grid(std::max(ncam, npts_ba)), dim3(LA_WG), 0, st, A);
  if (std::max(nkf, npts) > 0) hipLaunchKernelGGL(k_gp_write, grid(std::max(nkf, npts)), dim3(LA_WG), 0, st, A);
  if (run_nd && npts > 0 && nobs > 0) hipLaunchKernelGGL(k_gp_normals, grid(npts), dim3(LA_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_global_ba_apply(int ncam, const int32_t* cam_kf, const double* poses7, int npts_ba, const int32_t* gpt_pt, const double* pts3, int stage, int nkf,
                         const uint8_t* kf_bad, double* kf_Tcw, double* kf_center, int npts, double* X, const uint8_t* pt_bad, double* kf_gba_Tcw, uint8_t* kf_in_gba,
                         double* pt_gba_X, uint8_t* pt_in_gba, const int32_t* pt_ref_kf, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_level,
                         const float* scale_factors, int n_levels, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(ncam >= 0 && npts_ba >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_global_ba_apply: negative count");
  ORBHIP_REQUIRE(stage == 0 || stage == 1, ORBHIP_EINVAL, "orbl_global_ba_apply: stage is 0 or 1");
  ORBHIP_REQUIRE(counts, ORBHIP_EINVAL, "orbl_global_ba_apply: NULL counts");
  ORBHIP_REQUIRE(ncam == 0 || (cam_kf && poses7), ORBHIP_EINVAL, "orbl_global_ba_apply: NULL camera argument");
  ORBHIP_REQUIRE(npts_ba == 0 || (gpt_pt && pts3), ORBHIP_EINVAL, "orbl_global_ba_apply: NULL problem point argument");
  if (stage == 0) {
    ORBHIP_REQUIRE(nkf == 0 || kf_Tcw, ORBHIP_EINVAL, "orbl_global_ba_apply: stage 0 needs kf_Tcw");
    ORBHIP_REQUIRE(npts == 0 || X, ORBHIP_EINVAL, "orbl_global_ba_apply: stage 0 needs X");
  } else {
    ORBHIP_REQUIRE(nkf == 0 || (kf_gba_Tcw && kf_in_gba), ORBHIP_EINVAL, "orbl_global_ba_apply: stage 1 needs kf_gba_Tcw and kf_in_gba");
    ORBHIP_REQUIRE(npts == 0 || (pt_gba_X && pt_in_gba), ORBHIP_EINVAL, "orbl_global_ba_apply: stage 1 needs pt_gba_X and pt_in_gba");
  }
  const bool any_nd = pt_ref_kf || obs_off || obs_kf || ref_level || scale_factors || normal || min_max || nd_written;
  const bool nd = pt_ref_kf && obs_off && ref_level && scale_factors && normal && min_max && nd_written;
  ORBHIP_REQUIRE(!any_nd || nd, ORBHIP_EINVAL, "orbl_global_ba_apply: the normal / depth arguments are given as a set");
  const bool run_nd = nd && stage == 0 && npts > 0;
  ORBHIP_REQUIRE(!run_nd || nkf == 0 || kf_center, ORBHIP_EINVAL, "orbl_global_ba_apply: the normals need kf_center");
  ORBHIP_REQUIRE(!run_nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_global_ba_apply: n_levels out of range");
  static const char E[] = "orbl_global_ba_apply";
  ORBHIP_ARG(check_listed_once(E, "cam_kf", cam_kf, ncam, nkf));
  ORBHIP_ARG(check_listed_once(E, "gpt_pt", gpt_pt, npts_ba, npts));
  for (int c = 0; c < ncam; c++) {
    const double* s = poses7 + 7 * (size_t)c;
    ORBHIP_REQUIRE(mc_finite(s, 7) && ((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]) + s[6] * s[6] > 0.0, ORBHIP_EINVAL,
                   "orbl_global_ba_apply: a camera's pose is not finite or its quaternion is zero");
  }
  int nobs = 0;
  if (run_nd) {
    ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
    ORBHIP_REQUIRE(nobs == 0 || obs_kf, ORBHIP_EINVAL, "orbl_global_ba_apply: NULL obs_kf");
    ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
    std::vector<uint8_t> in((size_t)npts, 0);
    for (int j = 0; j < npts_ba; j++) in[gpt_pt[j]] = 1;
    const auto read = [&](int p) { return in[p] && obs_off[p] != obs_off[p + 1] && !(pt_bad && pt_bad[p]); };        // (no normal: neither is read)
    ORBHIP_ARG(check_index_if(E, "pt_ref_kf", pt_ref_kf, npts, nkf, [&](int p) { return read(p) && pt_ref_kf[p] != -1; }));
    ORBHIP_ARG(check_index_if(E, "ref_level", ref_level, npts, n_levels, read));
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, np = (size_t)npts, nc = (size_t)ncam, nb = (size_t)npts_ba;
  const bool s0 = stage == 0, s1 = stage == 1;
  RoundTrip R(W);
  const HostOut<double> t_Tcw = R.inout(s0 ? kf_Tcw : nullptr, 12 * nk), t_center = R.inout(s0 ? kf_center : nullptr, 3 * nk), t_X = R.inout(s0 ? X : nullptr, 3 * np),
                        t_gT = R.inout(s1 ? kf_gba_Tcw : nullptr, 12 * nk), t_gX = R.inout(s1 ? pt_gba_X : nullptr, 3 * np);
  const HostIn<int32_t> d_cam = R.in(cam_kf, nc), d_gpt = R.in(gpt_pt, nb), d_ref = R.in(run_nd ? pt_ref_kf : nullptr, np), d_ooff = R.csr(run_nd ? obs_off : nullptr, np),
                        d_okf = R.in(run_nd ? obs_kf : nullptr, (size_t)nobs), d_lvl = R.in(run_nd ? ref_level : nullptr, np);
  const HostIn<double> d_p7 = R.in(poses7, 7 * nc), d_pts3 = R.in(pts3, 3 * nb);
  const HostIn<uint8_t> d_kbad = R.in(kf_bad, nk), d_pbad = R.in(pt_bad, np);
  const HostIn<float> d_sf = R.in(run_nd ? scale_factors : nullptr, (size_t)n_levels);
  const HostOut<int32_t> o_counts = R.out<int32_t>(3);
  const HostOut<uint8_t> o_kin = R.out<uint8_t>(nk, s1 && nkf > 0), o_pin = R.out<uint8_t>(np, s1 && npts > 0), o_wrote = R.out<uint8_t>(np, run_nd);
  const HostOut<double> o_normal = R.out<double>(3 * np, run_nd);
  const HostOut<float> o_mm = R.out<float>(2 * np, run_nd);
  const HostOut<uint32_t> o_status = R.out<uint32_t>(1);
  R.scratch(gp_workspace(nkf, npts).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_global_ba_apply_device(ncam, d_cam.dev(), d_p7.dev(), npts_ba, d_gpt.dev(), d_pts3.dev(), stage, nkf, d_kbad.dev(), t_Tcw.dev(), t_center.dev(), npts, t_X.dev(),
                                        d_pbad.dev(), t_gT.dev(), o_kin.dev(), t_gX.dev(), o_pin.dev(), d_ref.dev(), nobs, d_ooff.dev(), d_okf.dev(), d_lvl.dev(), d_sf.dev(),
                                        n_levels, o_normal.dev(), o_mm.dev(), o_wrote.dev(), o_counts.dev(), o_status.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 3);
  if (s0) { R.copy_out(t_Tcw, kf_Tcw, 12 * nk); R.copy_out(t_center, kf_center, 3 * nk); R.copy_out(t_X, X, 3 * np); }
  else { R.copy_out(t_gT, kf_gba_Tcw, 12 * nk); R.copy_out(t_gX, pt_gba_X, 3 * np); R.copy_out(o_kin, kf_in_gba, nk); R.copy_out(o_pin, pt_in_gba, np); }
  if (run_nd) {
    R.copy_out(o_wrote, nd_written, np);
    for (size_t p = 0; p < np; p++)
      if (o_wrote[p]) { std::copy_n(&o_normal[3 * p], 3, normal + 3 * p); std::copy_n(&o_mm[2 * p], 2, min_max + 2 * p); }      // (rows of other points are not touched)
  }
  return 0;
}

}  // extern "C"
