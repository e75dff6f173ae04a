// orb_maptable.h -- what the kernels that walk the flat map tables share (orb_mappoint.inc, orb_kfculling.inc, orb_updateconn.inc,
// orb_mapcorrect.inc, orb_localba.inc, orb_essgraph.inc, orb_globalba.inc): the status word, the CSR row range, the workgroup scan, the
// 3x4 pose helpers and conversions, the row gate of the BA builders and MapPoint::UpdateNormalAndDepth.  Every .inc that uses one of
// them includes this header itself; it holds inline functions and templates only, so it may appear in more than one object of the
// library.  (orb_localupdate.inc, in orb_track.hip, keeps its own ulm_flag / ulm_range / ulm_block_scan: moved onto this header its
// device entry measured 1.2 % slower, profiles/maptable_refactor_time.json.)  FP64, no fused multiply-add (-ffp-contract=off); every sum
// is taken in the order written here - the tests hold these functions to the bit against the numpy restatements under tests/.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "ba_math.h"

namespace orbhip {

#define MT_SUM_WG 1024            /* k_mt_scan_sums: one workgroup */
#define MT_HD __host__ __device__ __forceinline__

// The three BA builders on the tables (orb_localba.inc, orb_essgraph.inc, orb_globalba.inc) share a workgroup size, and LocalBA and
// GlobalBA the *status bits of their device entries (GlobalBA adds GA_ST_*, the essential graph has EG_ST_* of its own).
#define LA_WG 256
#define LA_ST_OFFSETS 1u
#define LA_ST_KF 2u
#define LA_ST_PT 4u
#define LA_ST_RANK 8u
#define LA_ST_LEVEL 16u
#define LA_ST_CAP_CAM 32u
#define LA_ST_CAP_PTS 64u
#define LA_ST_CAP_OBS 128u
#define LA_ST_OBS 256u            /* apply: a row names an observation out of range, or an observation a slot its keyframe does not have */
#define LA_NONE 0xFFFFFFFFu

typedef unsigned long long mt_u64;

// ---------------------------------------------------------------------------------------------------------- table primitives
// raises `bits` in the status word of a device entry, when the caller gave one
__device__ __forceinline__ void mt_flag(uint32_t* status, uint32_t bits) { if (status) atomicOr(status, bits); }

// row i of a CSR table with `total` entries: [off[i], off[i + 1]) when it lies inside [0, total] and does not descend; false and an
// empty range when the offsets are not usable (the caller raises its own status bit)
__device__ __forceinline__ bool mt_range(const int32_t* off, int i, int total, int* lo, int* hi) {
  const int l = off[i], h = off[i + 1];
  const bool ok = l >= 0 && l <= h && h <= total;
  *lo = ok ? l : 0; *hi = ok ? h : 0;
  return ok;
}

__device__ __forceinline__ int mt_wave_sum(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// exclusive scan of one value per lane across a workgroup of WG lanes (a multiple of 64); *total = the workgroup's sum.
// sw: WG / 64 words of LDS, free again when the call returns
template <int WG, class T>
__device__ __forceinline__ T mt_block_excl(T v, T* sw, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(incl, o); if (lane >= o) incl += u; }
  if (lane == 63) sw[w] = incl;
  __syncthreads();
  T base = 0, tot = 0;
  for (int q = 0; q < WG / 64; q++) { const T s = sw[q]; if (q < w) base += s; tot += s; }
  __syncthreads();                                                              // (sw is free for the next call)
  *total = tot;
  return base + (incl - v);
}

// ONE workgroup: sums[0..nb) -> their exclusive scan, sums[nb] = the total
template <class T>
__global__ __launch_bounds__(MT_SUM_WG) void k_mt_scan_sums(T* sums, int nb) {
  __shared__ T sw[MT_SUM_WG / 64];
  T carry = 0;
  for (int b0 = 0; b0 < nb; b0 += MT_SUM_WG) {                                  // (workgroup-uniform)
    const int i = b0 + (int)threadIdx.x;
    T tot;
    const T ex = mt_block_excl<MT_SUM_WG>(i < nb ? sums[i] : T(0), sw, &tot);
    if (i < nb) sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) sums[nb] = carry;
}

// ---------------------------------------------------------------------------------------------------------- 3x4 poses
// C = A o B for row-major 3x4 matrices standing for 4x4 ones with the last row 0 0 0 1; every sum in index order k = 0..3
MT_HD void mc_affine_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      const double b3 = j == 3 ? 1.0 : 0.0;
      C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * b3;
    }
}

// Twc as KeyFrame::SetPose stores it (src/KeyFrame.cc:119-130): Rwc = Rcw^T, Ow = -(Rwc tcw); the centre is its last column
MT_HD void mc_pose_inverse(const double* T, double* Twc) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) Twc[4 * i + j] = T[4 * j + i];
    Twc[4 * i + 3] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
  }
}

// R x + t, each row (r0 x + r1 y) + r2 z, then + t
MT_HD void mc_apply34(const double* T, const double* x, double* out) {
  for (int i = 0; i < 3; i++) out[i] = ((T[4 * i] * x[0] + T[4 * i + 1] * x[1]) + T[4 * i + 2] * x[2]) + T[4 * i + 3];
}

// Sophus::Sim3d(Sophus::RxSO3d(1.0, R), t): the codec's matrix -> quaternion branches, un-normalised, scale 1
MT_HD void mc_se3_as_sim3(const double* T, double* S) {
  const double m[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
  rot_to_quat(m, S);
  S[4] = T[3]; S[5] = T[7]; S[6] = T[11];
}

// Matrix4dToMatrix_7_1 (ba_matrix4d_to_pose7): a 3x4 pose as (t, q), the quaternion un-normalised
MT_HD void mt_pose34_to_pose7(const double* T, double* o) {
  double S[7];
  mc_se3_as_sim3(T, S);
  o[0] = S[4]; o[1] = S[5]; o[2] = S[6]; o[3] = S[0]; o[4] = S[1]; o[5] = S[2]; o[6] = S[3];
}

// Matrix_7_1_ToMatrix4d (ba_pose7_to_matrix4d): (t, q) as a 3x4 pose; the quaternion is normalised first, the square root over the
// left-to-right sum of squares, then four divisions
MT_HD void mt_pose7_to_pose34(const double* s, double* T) {
  const double n = sqrt(((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]) + s[6] * s[6]);
  const double q[4] = {s[3] / n, s[4] / n, s[5] / n, s[6] / n};
  double R[9];
  quat_to_R(q, R);
  for (int r = 0; r < 3; r++) { T[4 * r] = R[3 * r]; T[4 * r + 1] = R[3 * r + 1]; T[4 * r + 2] = R[3 * r + 2]; T[4 * r + 3] = s[r]; }
}

// KeyFrame::SetPose: T becomes row k of the pose table and, when a centre table is given, its centre row k of that one
__device__ __forceinline__ void mt_set_pose(double* kf_Tcw, double* kf_center, int k, const double* T) {
  for (int q = 0; q < 12; q++) kf_Tcw[12 * (size_t)k + q] = T[q];
  if (kf_center) {
    double Twc[12];
    mc_pose_inverse(T, Twc);
    for (int q = 0; q < 3; q++) kf_center[3 * (size_t)k + q] = Twc[4 * q + 3];
  }
}

// ---------------------------------------------------------------------------------------------------------- the BA builders' row gate
// whether observation e becomes a row of the problem: its keyframe is not bad and has a camera (kf_cam[k] >= 0), its level is usable
// (src/CeresOptimizer.cc:142, :432, :458, :483).  A keyframe or a level out of range gives no row and raises st_kf / st_level.
__device__ __forceinline__ bool mt_row_ok(const int32_t* obs_kf, const int32_t* obs_level, int e, int nkf, int n_levels, const uint8_t* kf_bad,
                                          const int32_t* kf_cam, uint32_t* status, uint32_t st_kf, uint32_t st_level) {
  const int k = obs_kf[e];
  if (k < 0 || k >= nkf) { mt_flag(status, st_kf); return false; }
  if ((kf_bad && kf_bad[k]) || kf_cam[k] < 0) return false;
  const int lvl = obs_level[e];
  if (lvl < 0 || lvl >= n_levels) { mt_flag(status, st_level); return false; }
  return true;
}

// ---------------------------------------------------------------------------------------------------------- UpdateNormalAndDepth
#define MT_ND_OK 0                /* normal and min_max were written */
#define MT_ND_EMPTY 1             /* no observation is alive (src/MapPoint.cc:348): nothing written, as for every code below */
#define MT_ND_KF 2                /* an alive observation names a keyframe out of range */
#define MT_ND_REF 3               /* the reference keyframe is out of range */
#define MT_ND_LEVEL 4             /* the reference level is out of range */

// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:335-378) of the point at (x, y, z) over its observations [lo, hi), in list order:
// normal3 = the mean of the unit vectors from the observers' centres, min_max2 = the distance to the reference keyframe's centre times
// its level's scale factor, and that over the last level's.  The callers differ in three things, handed over as callables:
//   alive(e)    whether observation e counts (the divisor is the number that do);
//   centre(k)   the centre of keyframe k as a double3 - three VALUES: a callable that picks between two tables loads both and selects by
//               value, never a pointer ("The map-table helpers", has the compiler finding behind this rule);
//   level(e)    the reference level, given the last alive observation e whose keyframe is `ref`, or -1 when there is none.
// Returns MT_ND_*; which status bit a failure raises is the caller's business.
template <class Alive, class Centre, class Level>
__device__ __forceinline__ int mt_normal_depth(const int32_t* obs_kf, int lo, int hi, int nkf, double x, double y, double z, int ref, const float* scale_factors,
                                               int n_levels, double* normal3, float* min_max2, Alive alive, Centre centre, Level level) {
  double nx = 0.0, ny = 0.0, nz = 0.0;
  int n = 0, ref_e = -1;
  for (int e = lo; e < hi; e++) {                                              // (:356-364) normal + normali / normali.norm()
    if (!alive(e)) continue;
    const int k = obs_kf[e];
    if (k < 0 || k >= nkf) return MT_ND_KF;
    const double3 c = centre(k);
    const double vx = x - c.x, vy = y - c.y, vz = z - c.z;
    const double nn = sqrt((vx * vx + vy * vy) + vz * vz);
    nx = nx + vx / nn; ny = ny + vy / nn; nz = nz + vz / nn;
    n++;
    if (k == ref) ref_e = e;
  }
  if (n == 0) return MT_ND_EMPTY;
  if (ref < 0 || ref >= nkf) return MT_ND_REF;
  const int lvl = level(ref_e);
  if (lvl < 0 || lvl >= n_levels) return MT_ND_LEVEL;
  const double dn = (double)n;
  normal3[0] = nx / dn; normal3[1] = ny / dn; normal3[2] = nz / dn;             // (:376)
  const double3 c = centre(ref);
  const double px = x - c.x, py = y - c.y, pz = z - c.z;
  const float dist = (float)sqrt((px * px + py * py) + pz * pz);               // (:366-368)
  const float mx = dist * scale_factors[lvl];                                  // (:374)
  min_max2[0] = mx / scale_factors[n_levels - 1];
  min_max2[1] = mx;
  return MT_ND_OK;
}

// the common case: every observation counts, the centres are rows of kf_center, the reference level is the caller's
__device__ __forceinline__ int mt_normal_depth(const int32_t* obs_kf, int lo, int hi, int nkf, const double* kf_center, double x, double y, double z, int ref, int lvl,
                                               const float* scale_factors, int n_levels, double* normal3, float* min_max2) {
  return mt_normal_depth(obs_kf, lo, hi, nkf, x, y, z, ref, scale_factors, n_levels, normal3, min_max2, [](int) { return true; },
                         [=](int k) { return make_double3(kf_center[3 * (size_t)k], kf_center[3 * (size_t)k + 1], kf_center[3 * (size_t)k + 2]); },
                         [=](int) { return lvl; });
}

}  // namespace orbhip
