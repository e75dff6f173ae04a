// orb_sim3solver.inc -- Sim3Solver::iterate (src/Sim3Solver.cc:147-212: RANSAC, ComputeSim3 = Horn's closed form on three
// correspondences :225-363, CheckInliers :365-385) for a BATCH of loop candidates (orbt_sim3_*).  Textually included by orb_track.hip.
//
// One call = one `iterate` of every candidate.  The minimal sets are an input (the reference draws them lazily from the process-global
// DUtils::Random, :169-182), the best-so-far state (n_best_inliers_, is_best_inliers_, best_rotation_ / translation_ / scale_) is an
// in/out argument.  Four launches, one stream, no allocation, no host synchronisation:
//   k_sim3_prep    one workgroup per candidate: checks offsets, counts, set entries and the incoming state; a bad candidate fails alone.
//                  FromCameraToImage (:418-436) of both point sets, once, into the workspace.
//   k_sim3_hyp     one LANE per (candidate, set): ComputeSim3 in double, everything in registers.  The eigenvector of Horn's N comes
//                  from i_jacobi_sym4 (small_dense.h): with three points N's eigenvalues are pairs +-lambda, which the one-sided Jacobi
//                  cannot tell apart.  Every hypothesis of the call is computed, also those after the one the sequential rule stops at.
//   k_sim3_count   one wave per (candidate, set): CheckInliers with the reference's float / double narrowings, count only.
//   k_sim3_select  one workgroup per candidate walks the counts in order (:188-205): a count >= the best replaces it (ties go to the
//                  LATER set), a replacement with STRICTLY more than min_inliers ends the call.  Only the last replacement is visible
//                  afterwards, so only its mask is recomputed.
// tests/npsim3solver.py restates every step in this operation order; DESIGN.md section 2 ("Sim3 RANSAC") says what is pinned.
#include "small_dense.h"
namespace orbhip {

#define SIM3_WG 256
#define SIM3_HYP_LANES 64
#define SIM3_CNT_LANES 64

struct Sim3Cand {                     // per-candidate record in the workspace
  int32_t status;                     // 0 = runs, else ORBT_SIM3_TOO_FEW / ORBT_SIM3_BAD_INPUT
  int32_t off, n, n_sets, min_inl, fix_scale;
};

struct Sim3Args {
  int ncand, n_total, iterations;
  const double* X1; const double* X2; const float* max_err1; const float* max_err2; const int32_t* off; const float* K1; const float* K2;
  const int32_t* fix_scale; const int32_t* min_inl; const int32_t* n_sets; const int32_t* sets;
  int32_t* best_count; uint8_t* best_mask; double* best_R; double* best_t; float* best_scale;
  orbt_sim3_result* result; uint8_t* inliers;
  // workspace
  Sim3Cand* cand;
  double* im1; double* im2;           // [n_total][2]: FromCameraToImage of X1 under K1, of X2 under K2
  double* hyp;                        // [ncand][iterations][16]: R (9) | t (3) | scale (the float, widened) | relgap | 0 | 0
  int32_t* count;                     // [ncand][iterations]
};

// (:400-414, :421-434) fx, fy, cx, cy float; invz = float of a double quotient; x, y = float of a double product; fx * x + cx in float
__device__ __forceinline__ void sim3_to_image(const double* Pc, const float* K, double* uv) {
  const float invz = (float)(1.0 / Pc[2]);
  const float x = (float)(Pc[0] * (double)invz);
  const float y = (float)(Pc[1] * (double)invz);
  uv[0] = (double)(K[0] * x + K[2]);
  uv[1] = (double)(K[1] * y + K[3]);
}

// T12i_ and T21i_ (:347-362) of one hypothesis: sR = s R, t; sRi = (1 / s) R^T, ti = -(sRi t).  s is the FLOAT scale, widened.
struct Sim3Pose { double sR[9], t[3], sRi[9], ti[3]; };
__device__ __forceinline__ void sim3_pose(const double* R, const double* t, double s, Sim3Pose& P) {
  const double is = 1.0 / s;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { P.sR[3 * i + j] = s * R[3 * i + j]; P.sRi[3 * i + j] = is * R[3 * j + i]; }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    P.t[i] = t[i];
    P.ti[i] = -((P.sRi[3 * i] * t[0] + P.sRi[3 * i + 1] * t[1]) + P.sRi[3 * i + 2] * t[2]);
  }
}

// CheckInliers for one correspondence (:367-384): err1, err2 are floats of double dot products; a NaN compares false
__device__ __forceinline__ bool sim3_inlier(const Sim3Pose& P, const float* K1, const float* K2, const double* x1, const double* x2, const double* im1,
                                            const double* im2, float me1, float me2) {
  double p21[3], p12[3], uv21[2], uv12[2];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    p21[i] = ((P.sR[3 * i] * x2[0] + P.sR[3 * i + 1] * x2[1]) + P.sR[3 * i + 2] * x2[2]) + P.t[i];       // point 2 in camera 1 (T12)
    p12[i] = ((P.sRi[3 * i] * x1[0] + P.sRi[3 * i + 1] * x1[1]) + P.sRi[3 * i + 2] * x1[2]) + P.ti[i];   // point 1 in camera 2 (T21)
  }
  sim3_to_image(p21, K1, uv21);
  sim3_to_image(p12, K2, uv12);
  const double d10 = im1[0] - uv21[0], d11 = im1[1] - uv21[1], d20 = uv12[0] - im2[0], d21 = uv12[1] - im2[1];
  const float err1 = (float)(d10 * d10 + d11 * d11);
  const float err2 = (float)(d20 * d20 + d21 * d21);
  return err1 < me1 && err2 < me2;
}

// ComputeSim3 (:225-345) on three correspondences: a[k], b[k] = point k of set 1 / set 2.  R row-major, *scale the float of :336.
__device__ inline void sim3_horn(const double (&a)[3][3], const double (&b)[3][3], bool fix_scale, double* R, double* t, float* scale, double* relgap) {
  double O1[3], O2[3], Pr1[3][3], Pr2[3][3];                     // Pr[k][i] = coordinate i of centred point k
#pragma unroll
  for (int i = 0; i < 3; i++) {
    O1[i] = ((a[0][i] + a[1][i]) + a[2][i]) / 3.0;
    O2[i] = ((b[0][i] + b[1][i]) + b[2][i]) / 3.0;
  }
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int i = 0; i < 3; i++) { Pr1[k][i] = a[k][i] - O1[i]; Pr2[k][i] = b[k][i] - O2[i]; }
  double M[3][3];                                                // M = Pr2 Pr1^T (:244)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[i][j] = (Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j];
  double N[4][4], V[4][4];                                       // (:252-264)
  N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  N[0][1] = M[1][2] - M[2][1];
  N[0][2] = M[2][0] - M[0][2];
  N[0][3] = M[0][1] - M[1][0];
  N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  N[1][2] = M[0][1] + M[1][0];
  N[1][3] = M[2][0] + M[0][2];
  N[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
  N[2][3] = M[1][2] + M[2][1];
  N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
#pragma unroll
  for (int i = 1; i < 4; i++)
#pragma unroll
    for (int j = 0; j < i; j++) N[i][j] = N[j][i];
  i_jacobi_sym4(N, V);
  // (:275-277) the largest eigenvalue, first index on ties; the runner-up for the gap
  int mi = 0;
  double l3 = N[0][0];
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (N[k][k] > l3) { l3 = N[k][k]; mi = k; }
  double l2 = -1e300;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k != mi && N[k][k] > l2) l2 = N[k][k];
  *relgap = (l3 - l2) / l3;
  double q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = mi == 0 ? V[i][0] : mi == 1 ? V[i][1] : mi == 2 ? V[i][2] : V[i][3];
  // (:279-280) q.normalized().toRotationMatrix()
  const double nq = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
  float s = 1.0f;
  if (!fix_scale) {                                              // (:326-336) P3 = R Pr2; nom over the points, den over rows then columns
    double P3[3][3];                                             // P3[k][i] = coordinate i of rotated point k
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int i = 0; i < 3; i++) P3[k][i] = (R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1]) + R[3 * i + 2] * Pr2[k][2];
    double nom = 0, den = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) nom += (Pr1[k][0] * P3[k][0] + Pr1[k][1] * P3[k][1]) + Pr1[k][2] * P3[k][2];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) den += P3[k][i] * P3[k][i];
    s = (float)(nom / den);
  }
  *scale = s;
  const double sd = (double)s;                                   // (:342) t = O1 - (s R) O2
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = O1[i] - (((sd * R[3 * i]) * O2[0] + (sd * R[3 * i + 1]) * O2[1]) + (sd * R[3 * i + 2]) * O2[2]);
}

__global__ __launch_bounds__(SIM3_WG) void k_sim3_prep(Sim3Args a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  Sim3Cand& C = a.cand[c];
  __shared__ int s_bad, s_pop;
  const int o = a.off[c], e = a.off[c + 1], ns = a.n_sets[c], mi = a.min_inl[c], bcnt = a.best_count[c];
  const bool shape_ok = o >= 0 && o <= e && e <= a.n_total && e - o <= ORBT_SIM3_MAX_N && ns >= 0 && ns <= a.iterations && mi >= 3;
  if (!shape_ok) {
    if (tid == 0) { C.status = ORBT_SIM3_BAD_INPUT; C.off = 0; C.n = 0; C.n_sets = 0; C.min_inl = 0; C.fix_scale = 0; }
    return;
  }
  const int n = e - o;
  if (n < mi) {                                                  // (:153-156) before any set or the state is looked at
    if (tid == 0) { C.status = ORBT_SIM3_TOO_FEW; C.off = o; C.n = n; C.n_sets = 0; C.min_inl = mi; C.fix_scale = 0; }
    return;
  }
  if (tid == 0) { s_bad = 0; s_pop = 0; }
  __syncthreads();
  const int32_t* sets = a.sets + (size_t)c * a.iterations * 3;
  for (int s = tid; s < ns; s += SIM3_WG) {
    const int i0 = sets[3 * s], i1 = sets[3 * s + 1], i2 = sets[3 * s + 2];
    const bool in = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n;
    if (!in || i0 == i1 || i0 == i2 || i1 == i2) atomicOr(&s_bad, 1);
  }
  const float* K1 = a.K1 + 4 * (size_t)c;
  const float* K2 = a.K2 + 4 * (size_t)c;
  int pop = 0;
  for (int i = tid; i < n; i += SIM3_WG) {
    const size_t r = (size_t)o + i;
    pop += a.best_mask[r] != 0;
    sim3_to_image(a.X1 + 3 * r, K1, a.im1 + 2 * r);
    sim3_to_image(a.X2 + 3 * r, K2, a.im2 + 2 * r);
  }
  pop = i_wave_sum(pop);
  if ((tid & 63) == 0) atomicAdd(&s_pop, pop);
  __syncthreads();
  if (tid == 0) {
    const bool state_ok = bcnt >= 0 && bcnt <= n && s_pop == bcnt;
    C.status = (s_bad || !state_ok) ? ORBT_SIM3_BAD_INPUT : 0;
    C.off = o; C.n = n; C.n_sets = ns; C.min_inl = mi; C.fix_scale = a.fix_scale[c] != 0;
  }
}

__global__ __launch_bounds__(SIM3_HYP_LANES) void k_sim3_hyp(Sim3Args a) {
  const int c = blockIdx.y, it = blockIdx.x * SIM3_HYP_LANES + threadIdx.x;
  const Sim3Cand& C = a.cand[c];
  if (C.status || it >= C.n_sets) return;
  const int32_t* set = a.sets + ((size_t)c * a.iterations + it) * 3;
  double p1[3][3], p2[3][3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const size_t r = (size_t)C.off + set[k];                     // (prep has checked the entries of every set below n_sets)
#pragma unroll
    for (int i = 0; i < 3; i++) { p1[k][i] = a.X1[3 * r + i]; p2[k][i] = a.X2[3 * r + i]; }
  }
  double R[9], t[3], relgap;
  float s;
  sim3_horn(p1, p2, C.fix_scale != 0, R, t, &s, &relgap);
  double* out = a.hyp + ((size_t)c * a.iterations + it) * 16;
#pragma unroll
  for (int k = 0; k < 9; k++) out[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) out[9 + k] = t[k];
  out[12] = (double)s; out[13] = relgap; out[14] = 0.0; out[15] = 0.0;
}

__global__ __launch_bounds__(SIM3_CNT_LANES) void k_sim3_count(Sim3Args a) {
  const int it = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const Sim3Cand& C = a.cand[c];
  if (C.status || it >= C.n_sets) return;
  const double* h = a.hyp + ((size_t)c * a.iterations + it) * 16;
  Sim3Pose P;
  sim3_pose(h, h + 9, h[12], P);
  const float* K1 = a.K1 + 4 * (size_t)c;
  const float* K2 = a.K2 + 4 * (size_t)c;
  int cnt = 0;
  for (int i = tid; i < C.n; i += SIM3_CNT_LANES) {
    const size_t r = (size_t)C.off + i;
    cnt += sim3_inlier(P, K1, K2, a.X1 + 3 * r, a.X2 + 3 * r, a.im1 + 2 * r, a.im2 + 2 * r, a.max_err1[r], a.max_err2[r]);
  }
  cnt = i_wave_sum(cnt);
  if (tid == 0) a.count[(size_t)c * a.iterations + it] = cnt;
}

__global__ __launch_bounds__(SIM3_WG) void k_sim3_select(Sim3Args a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const Sim3Cand C = a.cand[c];
  orbt_sim3_result& res = a.result[c];
  if (C.status == ORBT_SIM3_BAD_INPUT) {                         // status only: the pose, the mask and the state stay as they were
    if (tid == 0) { res.status = ORBT_SIM3_BAD_INPUT; res.consumed = 0; res.n_inliers = 0; }
    return;
  }
  uint8_t* inl = a.inliers + C.off;
  uint8_t* bm = a.best_mask + C.off;
  double* bR = a.best_R + 9 * (size_t)c;
  double* bt = a.best_t + 3 * (size_t)c;
  int best = a.best_count[c];
  int best_it = -1, found_it = -1;
  if (C.status == 0) {
    const int32_t* cnt = a.count + (size_t)c * a.iterations;
    for (int it = 0; it < C.n_sets; it++) {                      // (every lane walks the same counts)
      const int k = cnt[it];
      if (k >= best) {                                           // (:188) ties go to the later set
        best = k; best_it = it;
        if (k > C.min_inl) { found_it = it; break; }             // (:198) strictly more
      }
    }
  }
  if (best_it >= 0) {                                            // (:189-194) the last replacement becomes the state
    const double* h = a.hyp + ((size_t)c * a.iterations + best_it) * 16;
    Sim3Pose P;
    sim3_pose(h, h + 9, h[12], P);
    const float* K1 = a.K1 + 4 * (size_t)c;
    const float* K2 = a.K2 + 4 * (size_t)c;
    for (int i = tid; i < C.n; i += SIM3_WG) {
      const size_t r = (size_t)C.off + i;
      bm[i] = sim3_inlier(P, K1, K2, a.X1 + 3 * r, a.X2 + 3 * r, a.im1 + 2 * r, a.im2 + 2 * r, a.max_err1[r], a.max_err2[r]);
    }
    if (tid == 0) {
      for (int k = 0; k < 9; k++) bR[k] = h[k];
      for (int k = 0; k < 3; k++) bt[k] = h[9 + k];
      a.best_scale[c] = (float)h[12];
      a.best_count[c] = best;
    }
    __syncthreads();                                             // the state is read back below
  }
  const bool found = found_it >= 0;
  for (int i = tid; i < C.n; i += SIM3_WG) inl[i] = found ? bm[i] : (uint8_t)0;
  if (tid == 0) {
    res.status = C.status == ORBT_SIM3_TOO_FEW ? ORBT_SIM3_TOO_FEW : found ? ORBT_SIM3_FOUND : ORBT_SIM3_NOT_FOUND;
    res.consumed = C.status ? 0 : found ? found_it + 1 : C.n_sets;
    res.n_inliers = found ? best : 0;
    const float s = a.best_scale[c];
    res.scale = s;
    for (int k = 0; k < 9; k++) res.R[k] = bR[k];
    for (int k = 0; k < 3; k++) res.t[k] = bt[k];
    for (int i = 0; i < 4; i++)                                  // (:204, :211) best_T12_ = [s R | t], or identity
      for (int j = 0; j < 4; j++)
        res.T12[4 * i + j] = !found ? (i == j ? 1.0 : 0.0) : i == 3 ? (j == 3 ? 1.0 : 0.0) : j == 3 ? bt[i] : (double)s * bR[3 * i + j];
  }
}

// workspace layout (bytes, 256-aligned pieces)
struct Sim3Ws {
  size_t cand, im1, im2, hyp, count, total;
};
static Sim3Ws sim3_ws_layout(int ncand, int n_total, int iterations) {
  Sim3Ws w;
  Carve blk;
  const size_t Cn = (size_t)ncand, N = (size_t)n_total, I = (size_t)iterations;
  w.cand = blk.take(sizeof(Sim3Cand) * Cn); w.im1 = blk.take(16 * N); w.im2 = blk.take(16 * N); w.hyp = blk.take(16 * 8 * Cn * I); w.count = blk.take(4 * Cn * I);
  w.total = blk.total;
  return w;
}

static bool sim3_counts_ok(int ncand, int n_total, int iterations) {
  return ncand >= 1 && ncand <= ORBT_SIM3_MAX_CANDIDATES && n_total >= 0 && iterations >= 1 && iterations <= ORBT_SIM3_MAX_ITERATIONS &&
         (long long)n_total <= (long long)ORBT_SIM3_MAX_N * ncand;
}

}  // namespace orbhip

extern "C" {

int orbt_sim3_ransac_params(int n, double probability, int min_inliers, int max_iterations, orbt_sim3_params* out) {
  ORBHIP_REQUIRE(out, ORBHIP_EINVAL, "orbt_sim3_ransac_params: NULL argument");
  ORBHIP_REQUIRE(n >= 0 && n <= ORBT_SIM3_MAX_N, ORBHIP_EINVAL, "orbt_sim3_ransac_params: n out of range");
  ORBHIP_REQUIRE(probability > 0.0 && probability < 1.0, ORBHIP_EINVAL, "orbt_sim3_ransac_params: probability must be inside (0, 1)");
  ORBHIP_REQUIRE(min_inliers >= 0 && max_iterations >= 1, ORBHIP_EINVAL, "orbt_sim3_ransac_params: min_inliers < 0 or max_iterations < 1");
  // (:131-142) epsilon is a float quotient, pow() runs in double
  int its = 1;
  if (min_inliers != n && n > 0) {
    const float epsilon = (float)min_inliers / (float)n;
    // n < min_inliers: log of a negative number, the quotient is not a number; so is 0 / 0 for min_inliers == 0.  Both end at 1.
    const double v = std::ceil(std::log(1.0 - probability) / std::log(1.0 - std::pow((double)epsilon, 3)));
    its = !(v >= 1.0) ? 1 : v > (double)max_iterations ? max_iterations : (int)v;
  }
  if (its > max_iterations) its = max_iterations;
  if (its < 1) its = 1;
  out->n = n; out->min_inliers = min_inliers; out->max_iterations = its; out->reserved = 0;
  return 0;
}

int orbt_sim3_iterate_workspace(int n_candidates, int n_total, int iterations, size_t* bytes) {
  using namespace orbhip;
  ORBHIP_REQUIRE(bytes && sim3_counts_ok(n_candidates, n_total, iterations), ORBHIP_EINVAL, "orbt_sim3_iterate_workspace: count out of range");
  *bytes = sim3_ws_layout(n_candidates, n_total, iterations).total;
  return 0;
}

int orbt_sim3_iterate_batch_device(int n_candidates, const double* d_X1c, const double* d_X2c, const float* d_max_err1, const float* d_max_err2,
                                   const int32_t* d_off, int n_total, const float* d_K1, const float* d_K2, const int32_t* d_fix_scale,
                                   const int32_t* d_min_inliers, const int32_t* d_n_sets, int iterations, const int32_t* d_sets, int32_t* d_best_count,
                                   uint8_t* d_best_mask, double* d_best_R, double* d_best_t, float* d_best_scale, orbt_sim3_result* d_result,
                                   uint8_t* d_inliers, void* d_workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(sim3_counts_ok(n_candidates, n_total, iterations), ORBHIP_EINVAL, "orbt_sim3_iterate: count out of range");
  ORBHIP_REQUIRE(d_X1c && d_X2c && d_max_err1 && d_max_err2 && d_off && d_K1 && d_K2 && d_fix_scale && d_min_inliers && d_n_sets && d_sets &&
                 d_best_count && d_best_mask && d_best_R && d_best_t && d_best_scale && d_result && d_inliers && d_workspace, ORBHIP_EINVAL,
                 "orbt_sim3_iterate: NULL argument");
  const Sim3Ws w = sim3_ws_layout(n_candidates, n_total, iterations);
  uint8_t* ws = (uint8_t*)d_workspace;
  Sim3Args A;
  A.ncand = n_candidates; A.n_total = n_total; A.iterations = iterations;
  A.X1 = d_X1c; A.X2 = d_X2c; A.max_err1 = d_max_err1; A.max_err2 = d_max_err2; A.off = d_off; A.K1 = d_K1; A.K2 = d_K2; A.fix_scale = d_fix_scale;
  A.min_inl = d_min_inliers; A.n_sets = d_n_sets; A.sets = d_sets;
  A.best_count = d_best_count; A.best_mask = d_best_mask; A.best_R = d_best_R; A.best_t = d_best_t; A.best_scale = d_best_scale;
  A.result = d_result; A.inliers = d_inliers;
  A.cand = (Sim3Cand*)(ws + w.cand); A.im1 = (double*)(ws + w.im1); A.im2 = (double*)(ws + w.im2); A.hyp = (double*)(ws + w.hyp);
  A.count = (int32_t*)(ws + w.count);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sim3_prep, dim3(n_candidates), dim3(SIM3_WG), 0, st, A);
  hipLaunchKernelGGL(k_sim3_hyp, dim3((iterations + SIM3_HYP_LANES - 1) / SIM3_HYP_LANES, n_candidates), dim3(SIM3_HYP_LANES), 0, st, A);
  hipLaunchKernelGGL(k_sim3_count, dim3(iterations, n_candidates), dim3(SIM3_CNT_LANES), 0, st, A);
  hipLaunchKernelGGL(k_sim3_select, dim3(n_candidates), dim3(SIM3_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbt_sim3_iterate(const double* X1c, const double* X2c, const float* max_err1, const float* max_err2, int n, const float* K1, const float* K2,
                      int fix_scale, int min_inliers, const int32_t* sets, int n_sets, int32_t* best_count, uint8_t* best_mask, double* best_R,
                      double* best_t, float* best_scale, orbt_sim3_result* result, uint8_t* inliers, const orbt_sim3_trace* trace) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(n >= 0 && n <= ORBT_SIM3_MAX_N, ORBHIP_EINVAL, "orbt_sim3_iterate: point count out of range");
  ORBHIP_REQUIRE(n_sets >= 0 && n_sets <= ORBT_SIM3_MAX_ITERATIONS, ORBHIP_EINVAL, "orbt_sim3_iterate: n_sets out of range");
  ORBHIP_REQUIRE(min_inliers >= 3, ORBHIP_EINVAL, "orbt_sim3_iterate: min_inliers below the minimal set (3)");
  ORBHIP_REQUIRE((X1c || n == 0) && (X2c || n == 0) && (max_err1 || n == 0) && (max_err2 || n == 0) && K1 && K2 && (sets || n_sets == 0) && best_count &&
                 (best_mask || n == 0) && best_R && best_t && best_scale && result && (inliers || n == 0), ORBHIP_EINVAL,
                 "orbt_sim3_iterate: NULL argument");
  if (n >= min_inliers) {
    for (int s = 0; s < n_sets; s++) {
      const int32_t* q = sets + 3 * (size_t)s;
      for (int j = 0; j < 3; j++) {
        ORBHIP_REQUIRE(q[j] >= 0 && q[j] < n, ORBHIP_EINVAL, "orbt_sim3_iterate: set entry outside [0, n)");
        for (int k = 0; k < j; k++) ORBHIP_REQUIRE(q[j] != q[k], ORBHIP_EINVAL, "orbt_sim3_iterate: an index is repeated inside a set");
      }
    }
    int pop = 0;
    for (int i = 0; i < n; i++) pop += best_mask[i] != 0;
    ORBHIP_REQUIRE(*best_count >= 0 && *best_count <= n && pop == *best_count, ORBHIP_EINVAL, "orbt_sim3_iterate: best_count does not match best_mask");
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const int iterations = n_sets > 0 ? n_sets : 1;
  const int32_t off[2] = {0, n};
  const int32_t zero_set[3] = {0, 0, 0};
  const int32_t fs = fix_scale != 0;
  ThreadWs::Pack in;
  const int pX1 = in.add(X1c, 24 * (size_t)n), pX2 = in.add(X2c, 24 * (size_t)n), pE1 = in.add(max_err1, 4 * (size_t)n), pE2 = in.add(max_err2, 4 * (size_t)n);
  const int pO = in.add(off, 8), pK1 = in.add(K1, 16), pK2 = in.add(K2, 16), pFs = in.add(&fs, 4), pMi = in.add(&min_inliers, 4), pNs = in.add(&n_sets, 4);
  const int pS = n_sets > 0 ? in.add(sets, 12 * (size_t)n_sets) : in.add(zero_set, 12);
  const int pBc = in.add(best_count, 4), pBm = in.add(best_mask, (size_t)n), pBr = in.add(best_R, 72), pBt = in.add(best_t, 24), pBs = in.add(best_scale, 4);
  const int pIn = in.add(inliers, (size_t)n);
  orbt_sim3_result r0 = *result;
  const int pR = in.add(&r0, sizeof(orbt_sim3_result));
  const Sim3Ws lay = sim3_ws_layout(1, n, iterations);
  uint8_t* dws = W.d<uint8_t>(lay.total, &rc);
  if (rc || (rc = W.commit(in))) return rc;
  if ((rc = orbt_sim3_iterate_batch_device(1, in.dev<double>(pX1), in.dev<double>(pX2), in.dev<float>(pE1), in.dev<float>(pE2), in.dev<int32_t>(pO), n,
                                           in.dev<float>(pK1), in.dev<float>(pK2), in.dev<int32_t>(pFs), in.dev<int32_t>(pMi), in.dev<int32_t>(pNs),
                                           iterations, in.dev<int32_t>(pS), in.dev<int32_t>(pBc), in.dev<uint8_t>(pBm), in.dev<double>(pBr),
                                           in.dev<double>(pBt), in.dev<float>(pBs), in.dev<orbt_sim3_result>(pR), in.dev<uint8_t>(pIn), dws, W.s))) return rc;
  // the in/out pieces lie between best_count and the result in the packed block: one download
  const size_t o0 = in.pieces[pBc].off, o1 = in.pieces[pR].off + sizeof(orbt_sim3_result);
  const uint8_t* hb = W.down(in.dbase + o0, o1 - o0, &rc);
  const bool want_trace = trace && (trace->R || trace->t || trace->scale || trace->count || trace->relgap);
  const uint8_t* hw = want_trace ? W.down(dws, lay.total, &rc) : nullptr;
  if (rc || (rc = W.sync())) return rc;
  const orbt_sim3_result res = *(const orbt_sim3_result*)(hb + (in.pieces[pR].off - o0));
  *result = res;
  if (res.status != ORBT_SIM3_BAD_INPUT) {
    *best_count = *(const int32_t*)(hb + (in.pieces[pBc].off - o0));
    if (n) std::memcpy(best_mask, hb + (in.pieces[pBm].off - o0), (size_t)n);
    std::memcpy(best_R, hb + (in.pieces[pBr].off - o0), 72);
    std::memcpy(best_t, hb + (in.pieces[pBt].off - o0), 24);
    std::memcpy(best_scale, hb + (in.pieces[pBs].off - o0), 4);
    if (n) std::memcpy(inliers, hb + (in.pieces[pIn].off - o0), (size_t)n);
  }
  if (hw) {                                                      // the trace: read back from the workspace, the consumed iterations only
    const double* hyp = (const double*)(hw + lay.hyp);
    const int32_t* cnt = (const int32_t*)(hw + lay.count);
    const bool ran = res.status == ORBT_SIM3_FOUND || res.status == ORBT_SIM3_NOT_FOUND;
    for (int it = 0; it < n_sets; it++) {
      const bool used = ran && it < res.consumed;
      const double* h = hyp + 16 * (size_t)it;
      if (trace->R) for (int k = 0; k < 9; k++) trace->R[9 * (size_t)it + k] = used ? h[k] : 0.0;
      if (trace->t) for (int k = 0; k < 3; k++) trace->t[3 * (size_t)it + k] = used ? h[9 + k] : 0.0;
      if (trace->scale) trace->scale[it] = used ? h[12] : 0.0;
      if (trace->relgap) trace->relgap[it] = used ? h[13] : 0.0;
      if (trace->count) trace->count[it] = used ? cnt[it] : 0;
    }
  }
  return 0;
}

}  // extern "C"
