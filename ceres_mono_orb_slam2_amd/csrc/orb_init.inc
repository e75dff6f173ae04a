// orb_init.inc -- Initializer::Initialize (src/Initializer.cc:54-889, monocular) for a BATCH of frame pairs (orbt_initialize*).
// Textually included by orb_frame.hip (after tri_math.h: CheckRT's 4x4 triangulation calls null_vector4_dev).
//
// The reference draws all 200 minimal sets before it evaluates any hypothesis (:75-101), so the sets are an input and every
// hypothesis is independent.  Six launches per call, one stream, no host synchronisation:
//   k_init_prep     one workgroup per pair: checks the pair's data, compacts the match list in ascending i1 (:60-72), Normalize
//                   (:714-755) of both frames.  The float sums run on one lane each in index order, reading the keypoints
//                   from global memory: bound by that lane's load latency and n dependent adds per pass.
//   k_init_hyp      one lane per (pair, iteration, model), both models in one launch: ComputeH21 / ComputeF21 (:228-304), the null vector of the 16 x 9 or
//                   8 x 9 system by one-sided Jacobi on A itself (the operation order of null_vector4_dev), F's rank-2 step through
//                   a 3 x 3 SVD, the denormalisation (:168-169, :215) and H12.
//   k_init_score    one workgroup per (pair, iteration, model): the per-match terms of CheckHomography / CheckFundamental
//                   (:306-444) in parallel into LDS, then ONE lane adds them in match order, the two terms of a match interleaved
//                   (the reference's float rounding; a tree would move the argmax on near-ties).
//   k_init_select   one workgroup per pair: the argmax of each model (`>` from 0, first index on ties, :173-177), the winners'
//                   inlier masks (recomputed with the scoring code), RH (:120-131) and the motions of the chosen model
//                   (ReconstructH's 8, :556-651, or DecomposeE's 4, :866-889).
//   k_init_checkrt  (motion x inlier) in parallel: CheckRT's per-match body (:793-853).
//   k_init_decide   one workgroup per pair, a wave per motion: nGood (integer reduction), sorted_cos[min(50, nGood - 1)] by an
//                   exact bitwise select on the float's order key (NaN after every number), the decision rules of ReconstructH /
//                   ReconstructF on one lane, then the winner's rows and the report.
// tests/npinit.py restates every step with the same operation order; DESIGN.md section 2 says what is pinned.
#include "small_dense.h"               /* i_mm3, i_inv3, i_jacobi, i_svd3, i_wave_sum: shared with orb_pnp.inc */
namespace orbhip {

#define INIT_WG 256
#define INIT_CHUNK 1024               /* k_init_score: matches per LDS chunk (2 terms each) */
#define INIT_RT_BLOCKS 8              /* k_init_checkrt: workgroups per (pair, motion) */
#define INIT_TH_COS 0.99998

struct InitPair {                     // per-pair state in the workspace
  int32_t status;                     // 0 = still running, else the ORBT_INIT_* reason that stopped the pair
  int32_t n_matches, n1, n2, off1, off2;
  int32_t model, best_h, best_f, n_inl_h, n_inl_f, n_motions;
  float score_h, score_f, rh, th2;
  double K[9], T1[9], T2[9];
  double R[8][9], t[8][3];
};

struct InitArgs {
  int npairs, n1_total, n2_total, iterations;
  float sigma;
  const float* kps1; const int32_t* off1; const float* kps2; const int32_t* off2; const int32_t* matches12; const float* K4; const int32_t* sets;
  double* R21; double* t21; double* P3D; uint8_t* tri; orbt_init_report* report;
  // workspace
  InitPair* pair;
  int32_t* mlist;                     // [n1_total][2] (i1, i2) of the pair's k-th match at off1 + k
  float* pn1; float* pn2;             // [n1_total][2], [n2_total][2] normalised keypoints
  double* hyp;                        // [npairs][iterations][27]: H21 | H12 | F21
  float* score;                       // [npairs][iterations][2]: SH, SF
  uint8_t* inl;                       // [2][n1_total]: the H and the F winner's inlier masks
  double* rt_p;                       // [8][n1_total][3] CheckRT's points
  float* rt_cos;                      // [8][n1_total]
  uint8_t* rt_flag;                   // [8][n1_total]: 1 = good, 2 = triangulated
};

// CheckHomography / CheckFundamental for one match: the two score terms (0 where chi2 > th: x + 0 == x for every x the
// sum can hold, it never holds -0) and the inlier bit.  model 0: Ma = H21, Mb = H12; model 1: Ma = F21.
__device__ __forceinline__ bool i_terms(int model, const double* Ma, const double* Mb, float u1, float v1, float u2, float v2, float invS2,
                                        float& ta, float& tb) {
  const double du1 = u1, dv1 = v1, du2 = u2, dv2 = v2;
  float chi1, chi2, th;
  if (model == 0) {
    th = 5.991f;
    const double x = (Mb[0] * du2 + Mb[1] * dv2) + Mb[2], y = (Mb[3] * du2 + Mb[4] * dv2) + Mb[5], z = (Mb[6] * du2 + Mb[7] * dv2) + Mb[8];
    const float u2in1 = (float)(x / z), v2in1 = (float)(y / z);
    const float sq1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    chi1 = sq1 * invS2;
    const double x2 = (Ma[0] * du1 + Ma[1] * dv1) + Ma[2], y2 = (Ma[3] * du1 + Ma[4] * dv1) + Ma[5], z2 = (Ma[6] * du1 + Ma[7] * dv1) + Ma[8];
    const float u1in2 = (float)(x2 / z2), v1in2 = (float)(y2 / z2);
    const float sq2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    chi2 = sq2 * invS2;
  } else {
    th = 3.841f;
    const double l20 = (Ma[0] * du1 + Ma[1] * dv1) + Ma[2], l21 = (Ma[3] * du1 + Ma[4] * dv1) + Ma[5], l22 = (Ma[6] * du1 + Ma[7] * dv1) + Ma[8];
    const float num2 = (float)((du2 * l20 + dv2 * l21) + l22);
    const float sq1 = (float)((double)(num2 * num2) / (l20 * l20 + l21 * l21));
    chi1 = sq1 * invS2;
    const double l10 = (du2 * Ma[0] + dv2 * Ma[3]) + Ma[6], l11 = (du2 * Ma[1] + dv2 * Ma[4]) + Ma[7], l12 = (du2 * Ma[2] + dv2 * Ma[5]) + Ma[8];
    const float num1 = (float)((l10 * du1 + l11 * dv1) + l12);
    const float sq2 = (float)((double)(num1 * num1) / (l10 * l10 + l11 * l11));
    chi2 = sq2 * invS2;
  }
  const float ths = 5.991f;
  ta = chi1 > th ? 0.0f : ths - chi1;
  tb = chi2 > th ? 0.0f : ths - chi2;
  return !(chi1 > th) && !(chi2 > th);
}

// the order key of a float: ascending keys = ascending values, every NaN last (0xffffffff)
__device__ __forceinline__ uint32_t i_key(float f) {
  const uint32_t b = __float_as_uint(f);
  if (f != f) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float i_unkey(uint32_t k) {
  if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(INIT_WG) void k_init_prep(InitArgs a) {
  const int p = blockIdx.x, tid = threadIdx.x;
  InitPair& P = a.pair[p];
  __shared__ int s_bad, s_nm;
  __shared__ float s_stat[8];
  const int o1 = a.off1[p], e1 = a.off1[p + 1], o2 = a.off2[p], e2 = a.off2[p + 1];
  const bool shape_ok = o1 >= 0 && o1 <= e1 && e1 <= a.n1_total && o2 >= 0 && o2 <= e2 && e2 <= a.n2_total && e1 - o1 <= ORBT_INIT_MAX_N &&
                        e2 - o2 <= ORBT_INIT_MAX_N;
  if (!shape_ok) {                                             // (every field the report reads is set: the pair fails alone)
    if (tid == 0) {
      P.status = ORBT_INIT_BAD_INPUT; P.n_matches = 0; P.n1 = P.n2 = 0; P.off1 = P.off2 = 0;
      P.model = -1; P.best_h = P.best_f = -1; P.n_inl_h = P.n_inl_f = 0; P.n_motions = 0;
      P.score_h = P.score_f = 0.0f; P.rh = 0.0f;
    }
    return;
  }
  const int n1 = e1 - o1, n2 = e2 - o2;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int i = tid; i < n1; i += INIT_WG) {
    const int m = a.matches12[o1 + i];
    if (m < -1 || m >= n2) atomicOr(&s_bad, 1);
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0 && wave == 0) {                                // (:60-72) the match list, ascending i1
    int k = 0;
    for (int i = 0; i < n1; i++) {
      const int m = a.matches12[o1 + i];
      if (m >= 0) { a.mlist[2 * (size_t)(o1 + k)] = i; a.mlist[2 * (size_t)(o1 + k) + 1] = m; k++; }
    }
    s_nm = k;
  } else if (lane == 0 && (wave == 1 || wave == 2)) {          // (:714-755) Normalize: float sums in index order, one lane per frame
    const float* kp = wave == 1 ? a.kps1 + 2 * (size_t)o1 : a.kps2 + 2 * (size_t)o2;
    const int n = wave == 1 ? n1 : n2;
    float mx = 0, my = 0;
    for (int i = 0; i < n; i++) { mx += kp[2 * i]; my += kp[2 * i + 1]; }
    mx = mx / n; my = my / n;
    float dx = 0, dy = 0;
    for (int i = 0; i < n; i++) { dx += fabsf(kp[2 * i] - mx); dy += fabsf(kp[2 * i + 1] - my); }
    dx = dx / n; dy = dy / n;
    const float sx = (float)(1.0 / (double)dx), sy = (float)(1.0 / (double)dy);
    float* st = s_stat + 4 * (wave - 1);
    st[0] = mx; st[1] = my; st[2] = sx; st[3] = sy;
  }
  __syncthreads();
  const int nm = s_nm;
  const size_t nset = (size_t)a.iterations * 8;
  const int32_t* sets = a.sets + (size_t)p * nset;
  for (size_t j = tid; j < nset; j += INIT_WG)
    if (sets[j] < 0 || sets[j] >= nm) atomicOr(&s_bad, 1);
  for (int i = tid; i < n1; i += INIT_WG) {
    a.pn1[2 * (size_t)(o1 + i)] = (a.kps1[2 * (size_t)(o1 + i)] - s_stat[0]) * s_stat[2];
    a.pn1[2 * (size_t)(o1 + i) + 1] = (a.kps1[2 * (size_t)(o1 + i) + 1] - s_stat[1]) * s_stat[3];
  }
  for (int i = tid; i < n2; i += INIT_WG) {
    a.pn2[2 * (size_t)(o2 + i)] = (a.kps2[2 * (size_t)(o2 + i)] - s_stat[4]) * s_stat[6];
    a.pn2[2 * (size_t)(o2 + i) + 1] = (a.kps2[2 * (size_t)(o2 + i) + 1] - s_stat[5]) * s_stat[7];
  }
  __syncthreads();
  if (tid == 0) {
    P.status = (s_bad || nm < 8) ? ORBT_INIT_BAD_INPUT : 0;
    P.n_matches = nm; P.n1 = n1; P.n2 = n2; P.off1 = o1; P.off2 = o2;
    P.best_h = P.best_f = -1; P.n_inl_h = P.n_inl_f = 0; P.n_motions = 0; P.model = -1;
    P.score_h = P.score_f = 0.0f; P.rh = 0.0f;
    const float* K4 = a.K4 + 4 * (size_t)p;
    const double K[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    for (int k = 0; k < 9; k++) P.K[k] = K[k];
    for (int f = 0; f < 2; f++) {
      const float* st = s_stat + 4 * f;
      double* T = f == 0 ? P.T1 : P.T2;
      T[0] = st[2]; T[1] = 0; T[2] = (double)(-st[0] * st[2]);
      T[3] = 0; T[4] = st[3]; T[5] = (double)(-st[1] * st[3]);
      T[6] = 0; T[7] = 0; T[8] = 1.0;
    }
    const float sigma2 = a.sigma * a.sigma;
    P.th2 = (float)(4.0 * (double)sigma2);
  }
}

// (:135-225) one hypothesis of model MODEL (0 = H, 1 = F) per lane
template <int MODEL>
__device__ __forceinline__ void init_hyp(const InitArgs& a) {
  const int p = blockIdx.z, it = blockIdx.x * 64 + threadIdx.x;
  const InitPair& P = a.pair[p];
  if (P.status || it >= a.iterations) return;
  const int32_t* set = a.sets + ((size_t)p * a.iterations + it) * 8;
  constexpr int M = MODEL == 0 ? 16 : 8;
  double U[M][9], V[9][9];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const size_t k = (size_t)P.off1 + set[j];
    const int i1 = a.mlist[2 * k], i2 = a.mlist[2 * k + 1];
    const float u1 = a.pn1[2 * ((size_t)P.off1 + i1)], v1 = a.pn1[2 * ((size_t)P.off1 + i1) + 1];
    const float u2 = a.pn2[2 * ((size_t)P.off2 + i2)], v2 = a.pn2[2 * ((size_t)P.off2 + i2) + 1];
    if (MODEL == 0) {                                          // (:234-253)
      double* r0 = U[(2 * j) % M]; double* r1 = U[(2 * j + 1) % M];
      r0[0] = -u1; r0[1] = -v1; r0[2] = -1.0; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = u1 * u2; r0[7] = v1 * u2; r0[8] = u2;
      r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = -u1; r1[4] = -v1; r1[5] = -1.0; r1[6] = u1 * v2; r1[7] = v1 * v2; r1[8] = v2;
    } else {                                                   // (:270-285)
      double* r = U[j % M];
      r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1.0;
    }
  }
  i_jacobi<M, 9>(U, V);
  const int c = i_min_col<M, 9>(U);
  double Mn[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    double v = V[k][0];
#pragma unroll
    for (int j = 1; j < 9; j++) v = c == j ? V[k][j] : v;
    Mn[k] = v;                                                 // row-major: Map<Matrix3d>(V.col(8)).transpose()
  }
  double* out = a.hyp + ((size_t)p * a.iterations + it) * 27;
  if (MODEL == 0) {
    double T2i[9], tmp[9], H21[9], H12[9];
    i_inv3(P.T2, T2i);
    i_mm3(T2i, Mn, tmp); i_mm3(tmp, P.T1, H21);               // (:168) T2^-1 Hn T1
    i_inv3(H21, H12);                                          // (:169)
#pragma unroll
    for (int k = 0; k < 9; k++) { out[k] = H21[k]; out[9 + k] = H12[k]; }
  } else {
    double Us[9], S[3], Vs[9], W[9], Fn[9], T2t[9], tmp[9], F21[9];
    i_svd3(Mn, Us, S, Vs);                                     // (:293-301) rank 2
    const double Sz[3] = {S[0], S[1], 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) W[3 * i + k] = Us[3 * i + k] * Sz[k];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Fn[3 * i + j] = (W[3 * i] * Vs[3 * j] + W[3 * i + 1] * Vs[3 * j + 1]) + W[3 * i + 2] * Vs[3 * j + 2];
    i_tr3(P.T2, T2t);
    i_mm3(T2t, Fn, tmp); i_mm3(tmp, P.T1, F21);               // (:215) T2^T Fn T1
#pragma unroll
    for (int k = 0; k < 9; k++) out[18 + k] = F21[k];
  }
}

// both models in one launch (blockIdx.y): each fills only iterations / 64 waves per pair, side by side they share the GPU
__global__ __launch_bounds__(64) void k_init_hyp(InitArgs a) {
  if (blockIdx.y == 0) init_hyp<0>(a);
  else init_hyp<1>(a);
}

__device__ __forceinline__ void i_match_pts(const InitArgs& a, const InitPair& P, int k, float& u1, float& v1, float& u2, float& v2) {
  const int i1 = a.mlist[2 * ((size_t)P.off1 + k)], i2 = a.mlist[2 * ((size_t)P.off1 + k) + 1];
  u1 = a.kps1[2 * ((size_t)P.off1 + i1)]; v1 = a.kps1[2 * ((size_t)P.off1 + i1) + 1];
  u2 = a.kps2[2 * ((size_t)P.off2 + i2)]; v2 = a.kps2[2 * ((size_t)P.off2 + i2) + 1];
}

// (:306-444) the score of one hypothesis: terms in parallel, the float sum on one lane in match order
__global__ __launch_bounds__(INIT_WG) void k_init_score(InitArgs a) {
  const int it = blockIdx.x, model = blockIdx.y, p = blockIdx.z, tid = threadIdx.x;
  const InitPair& P = a.pair[p];
  if (P.status) return;
  const double* Mx = a.hyp + ((size_t)p * a.iterations + it) * 27;
  double Ma[9], Mb[9];
#pragma unroll
  for (int k = 0; k < 9; k++) { Ma[k] = model == 0 ? Mx[k] : Mx[18 + k]; Mb[k] = Mx[9 + k]; }
  const float invS2 = (float)(1.0 / (double)(a.sigma * a.sigma));
  __shared__ float terms[2 * INIT_CHUNK];
  float score = 0.0f;
  const int n = P.n_matches;
  for (int base = 0; base < n; base += INIT_CHUNK) {
    const int cnt = min(INIT_CHUNK, n - base);
    for (int k = tid; k < cnt; k += INIT_WG) {
      float u1, v1, u2, v2, ta, tb;
      i_match_pts(a, P, base + k, u1, v1, u2, v2);
      i_terms(model, Ma, Mb, u1, v1, u2, v2, invS2, ta, tb);
      terms[2 * k] = ta; terms[2 * k + 1] = tb;
    }
    __syncthreads();
    if (tid == 0)
      for (int k = 0; k < 2 * cnt; k++) score += terms[k];
    __syncthreads();
  }
  if (tid == 0) a.score[((size_t)p * a.iterations + it) * 2 + model] = score;
}

// the motions of ReconstructH (:556-651); false = d1 / d2 or d2 / d3 below 1.00001 (:573-575)
__device__ inline bool i_motions_h(InitPair& P, const double* H21) {
  double Ki[9], tmp[9], A[9], U[9], S[3], V[9], Vt[9];
  i_inv3(P.K, Ki);
  i_mm3(Ki, H21, tmp); i_mm3(tmp, P.K, A);
  i_svd3(A, U, S, V);
  const float s = (float)(i_det3(U) * i_det3(V));
  const float d1 = (float)S[0], d2 = (float)S[1], d3 = (float)S[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  double sU[9];
  for (int k = 0; k < 9; k++) sU[k] = (double)s * U[k];
  i_tr3(V, Vt);
  for (int m = 0; m < 8; m++) {
    const int i = m & 3;
    double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tp[3];
    if (m < 4) {                                               // d' = d2
      Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
      const double f = (double)(d1 - d3);
      tp[0] = (double)x1[i] * f; tp[1] = 0.0 * f; tp[2] = (double)(-x3[i]) * f;
    } else {                                                   // d' = -d2
      Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1; Rp[6] = sphi[i]; Rp[8] = -cphi;
      const double f = (double)(d1 + d3);
      tp[0] = (double)x1[i] * f; tp[1] = 0.0 * f; tp[2] = (double)x3[i] * f;
    }
    i_mm3(sU, Rp, tmp); i_mm3(tmp, Vt, P.R[m]);
    double t[3];
    for (int r = 0; r < 3; r++) t[r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
    const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int r = 0; r < 3; r++) P.t[m][r] = t[r] / nt;
  }
  P.n_motions = 8;
  return true;
}

// ReconstructF's E21 = K^T F21 K (:457) and DecomposeE (:866-889): motions (R1, t), (R2, t), (R1, -t), (R2, -t)
__device__ inline void i_motions_f(InitPair& P, const double* F21) {
  double Kt[9], tmp[9], E[9], U[9], S[3], V[9], Vt[9], R1[9], R2[9];
  i_tr3(P.K, Kt);
  i_mm3(Kt, F21, tmp); i_mm3(tmp, P.K, E);
  i_svd3(E, U, S, V);
  i_tr3(V, Vt);
  const double W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
  i_mm3(U, W, tmp); i_mm3(tmp, Vt, R1);
  i_mm3(U, Wt, tmp); i_mm3(tmp, Vt, R2);
  double t[3] = {U[2], U[5], U[8]};
  const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  for (int r = 0; r < 3; r++) t[r] = t[r] / nt;
  if (i_det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
  if (i_det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
  for (int m = 0; m < 4; m++) {
    const double* R = (m & 1) ? R2 : R1;
    for (int k = 0; k < 9; k++) P.R[m][k] = R[k];
    for (int r = 0; r < 3; r++) P.t[m][r] = m < 2 ? t[r] : -t[r];
  }
  P.n_motions = 4;
}

__global__ __launch_bounds__(INIT_WG) void k_init_select(InitArgs a) {
  const int p = blockIdx.x, tid = threadIdx.x;
  InitPair& P = a.pair[p];
  if (P.status) return;
  __shared__ int s_best[2], s_cnt[2];
  __shared__ float s_sc[2];
  if (tid < 2) {                                               // (:173-177, :219-223)
    float best = 0.0f; int bi = -1;
    for (int it = 0; it < a.iterations; it++) {
      const float s = a.score[((size_t)p * a.iterations + it) * 2 + tid];
      if (s > best) { best = s; bi = it; }
    }
    s_best[tid] = bi; s_sc[tid] = best; s_cnt[tid] = 0;
  }
  __syncthreads();
  const float invS2 = (float)(1.0 / (double)(a.sigma * a.sigma));
  const int n = P.n_matches;
  for (int model = 0; model < 2; model++) {
    const int bi = s_best[model];
    uint8_t* inl = a.inl + (size_t)model * a.n1_total + P.off1;
    if (bi < 0) { for (int k = tid; k < n; k += INIT_WG) inl[k] = 0; continue; }
    const double* Mx = a.hyp + ((size_t)p * a.iterations + bi) * 27;
    double Ma[9], Mb[9];
    for (int k = 0; k < 9; k++) { Ma[k] = model == 0 ? Mx[k] : Mx[18 + k]; Mb[k] = Mx[9 + k]; }
    int cnt = 0;
    for (int k = tid; k < n; k += INIT_WG) {
      float u1, v1, u2, v2, ta, tb;
      i_match_pts(a, P, k, u1, v1, u2, v2);
      const bool in = i_terms(model, Ma, Mb, u1, v1, u2, v2, invS2, ta, tb);
      inl[k] = in; cnt += in;
    }
    cnt = i_wave_sum(cnt);
    if ((tid & 63) == 0) atomicAdd(&s_cnt[model], cnt);
  }
  __syncthreads();
  if (tid == 0) {
    P.best_h = s_best[0]; P.best_f = s_best[1]; P.score_h = s_sc[0]; P.score_f = s_sc[1];
    P.n_inl_h = s_cnt[0]; P.n_inl_f = s_cnt[1];
    const float SH = s_sc[0], SF = s_sc[1];
    const float RH = SH / (SH + SF);                           // (:120-131)
    P.rh = RH;
    P.model = (double)RH > 0.40 ? 0 : 1;
    const int bi = s_best[P.model];
    if (bi < 0) { P.status = ORBT_INIT_NO_MODEL; return; }
    const double* Mx = a.hyp + ((size_t)p * a.iterations + bi) * 27;
    if (P.model == 0) {
      if (!i_motions_h(P, Mx)) P.status = ORBT_INIT_H_DEGENERATE;
    } else {
      i_motions_f(P, Mx + 18);
    }
  }
}

// (:757-853) CheckRT's body for (motion, inlier match)
__global__ __launch_bounds__(INIT_WG) void k_init_checkrt(InitArgs a) {
  const int m = blockIdx.y, p = blockIdx.z;
  const InitPair& P = a.pair[p];
  if (P.status || m >= P.n_motions) return;
  const double* K = P.K;
  const float fx = (float)K[0], fy = (float)K[4], cx = (float)K[2], cy = (float)K[5];
  const double* R = P.R[m]; const double* t = P.t[m];
  double P1[12] = {K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0}, Rt[12], P2[12], O2[3];
  for (int i = 0; i < 3; i++) { Rt[4 * i] = R[3 * i]; Rt[4 * i + 1] = R[3 * i + 1]; Rt[4 * i + 2] = R[3 * i + 2]; Rt[4 * i + 3] = t[i]; }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) P2[4 * i + j] = (K[3 * i] * Rt[j] + K[3 * i + 1] * Rt[4 + j]) + K[3 * i + 2] * Rt[8 + j];
  for (int i = 0; i < 3; i++) O2[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];
  const uint8_t* inl = a.inl + (size_t)P.model * a.n1_total + P.off1;
  const size_t base = (size_t)m * a.n1_total + P.off1;
  const float th2 = P.th2;
  for (int k = blockIdx.x * INIT_WG + threadIdx.x; k < P.n_matches; k += gridDim.x * INIT_WG) {
    uint8_t flag = 0;
    if (inl[k]) {
      float x1p, y1p, x2p, y2p;
      i_match_pts(a, P, k, x1p, y1p, x2p, y2p);
      double A[16], X4[4];
      for (int j = 0; j < 4; j++) {                            // (:697-712)
        A[j] = (double)x1p * P1[8 + j] - P1[j];
        A[4 + j] = (double)y1p * P1[8 + j] - P1[4 + j];
        A[8 + j] = (double)x2p * P2[8 + j] - P2[j];
        A[12 + j] = (double)y2p * P2[8 + j] - P2[4 + j];
      }
      null_vector4_dev(A, X4);
      const double p0 = X4[0] / X4[3], p1 = X4[1] / X4[3], p2 = X4[2] / X4[3];
      do {
        if (!isfinite(p0) || !isfinite(p1) || !isfinite(p2)) break;
        const float dist1 = (float)sqrt((p0 * p0 + p1 * p1) + p2 * p2);
        const double n2x = p0 - O2[0], n2y = p1 - O2[1], n2z = p2 - O2[2];
        const float dist2 = (float)sqrt((n2x * n2x + n2y * n2y) + n2z * n2z);
        const float cosp = (float)(((p0 * n2x + p1 * n2y) + p2 * n2z) / (double)(dist1 * dist2));
        if (p2 <= 0 && (double)cosp < INIT_TH_COS) break;
        const double q0 = ((R[0] * p0 + R[1] * p1) + R[2] * p2) + t[0];
        const double q1 = ((R[3] * p0 + R[4] * p1) + R[5] * p2) + t[1];
        const double q2 = ((R[6] * p0 + R[7] * p1) + R[8] * p2) + t[2];
        if (q2 <= 0 && (double)cosp < INIT_TH_COS) break;
        const float invZ1 = (float)(1.0 / p2);
        const float im1x = (float)((double)fx * p0 * (double)invZ1 + (double)cx), im1y = (float)((double)fy * p1 * (double)invZ1 + (double)cy);
        const float e1 = (im1x - x1p) * (im1x - x1p) + (im1y - y1p) * (im1y - y1p);
        if (e1 > th2) break;
        const float invZ2 = (float)(1.0 / q2);
        const float im2x = (float)((double)fx * q0 * (double)invZ2 + (double)cx), im2y = (float)((double)fy * q1 * (double)invZ2 + (double)cy);
        const float e2 = (im2x - x2p) * (im2x - x2p) + (im2y - y2p) * (im2y - y2p);
        if (e2 > th2) break;
        flag = 1 | ((double)cosp < INIT_TH_COS ? 2 : 0);
        a.rt_cos[base + k] = cosp;
        a.rt_p[3 * (base + k)] = p0; a.rt_p[3 * (base + k) + 1] = p1; a.rt_p[3 * (base + k) + 2] = p2;
      } while (0);
    }
    a.rt_flag[base + k] = flag;
  }
}

// nGood, parallax, the decision rules (:653-693 / :484-538) and the winner's rows
__global__ __launch_bounds__(512) void k_init_decide(InitArgs a) {
  const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  InitPair& P = a.pair[p];
  __shared__ int s_good[8], s_win;
  __shared__ float s_par[8];
  const bool run = P.status == 0;
  const int n = run ? P.n_matches : 0;
  if (run && wave < P.n_motions) {
    const size_t base = (size_t)wave * a.n1_total + P.off1;
    int g = 0;
    for (int k = lane; k < n; k += 64) g += a.rt_flag[base + k] & 1;
    g = i_wave_sum(g);
    float par = 0.0f;
    if (g > 0) {
      const int kth = min(50, g - 1);                          // sorted_cos[kth]: the largest key with fewer than kth + 1 keys below it
      uint32_t res = 0;
      for (int bit = 31; bit >= 0; bit--) {
        const uint32_t cand = res | (1u << bit);
        int below = 0;
        for (int k = lane; k < n; k += 64)
          if ((a.rt_flag[base + k] & 1) && i_key(a.rt_cos[base + k]) < cand) below++;
        below = i_wave_sum(below);
        if (below <= kth) res = cand;
      }
      par = (float)((double)(acosf(i_unkey(res)) * 180.0f) / 3.14159265358979323846);
    }
    if (lane == 0) { s_good[wave] = g; s_par[wave] = par; }
  } else if (lane == 0) {
    s_good[wave] = 0; s_par[wave] = 0.0f;
  }
  __syncthreads();
  if (tid == 0) {
    int win = -1, reason = P.status;
    if (run && P.model == 0) {
      const int N = P.n_inl_h;
      int bestGood = 0, second = 0, bi = -1; float bestPar = -1;
      for (int i = 0; i < 8; i++) {
        if (s_good[i] > bestGood) { second = bestGood; bestGood = s_good[i]; bi = i; bestPar = s_par[i]; }
        else if (s_good[i] > second) second = s_good[i];
      }
      if (!(second < 0.75 * bestGood)) reason = ORBT_INIT_H_AMBIGUOUS;
      else if (!(bestPar >= 1.0f)) reason = ORBT_INIT_H_PARALLAX;
      else if (!(bestGood > 50) || !(bestGood > 0.9 * N)) reason = ORBT_INIT_H_FEW;
      else win = bi;
    } else if (run) {
      const int N = P.n_inl_f;
      const int maxGood = max(s_good[0], max(s_good[1], max(s_good[2], s_good[3])));
      const int nMinGood = max((int)(0.9 * N), 50);
      int nsimilar = 0;
      for (int i = 0; i < 4; i++) nsimilar += s_good[i] > 0.7 * maxGood;
      if (maxGood < nMinGood) reason = ORBT_INIT_F_FEW;
      else if (nsimilar > 1) reason = ORBT_INIT_F_AMBIGUOUS;
      else {
        int k = 0;
        while (s_good[k] != maxGood) k++;                     // the first branch that matches; no fall-through
        if (s_par[k] > 1.0f) win = k; else reason = ORBT_INIT_F_PARALLAX;
      }
    }
    if (win >= 0) reason = ORBT_INIT_OK;
    s_win = win;
    orbt_init_report& r = a.report[p];
    r.model = P.model; r.reason = reason; r.score_h = P.score_h; r.score_f = P.score_f; r.rh = P.rh;
    r.best_h = P.best_h; r.best_f = P.best_f; r.n_matches = P.n_matches;
    r.n_inliers = P.model == 0 ? P.n_inl_h : P.model == 1 ? P.n_inl_f : 0;
    r.motion = win;
    for (int i = 0; i < 8; i++) { r.n_good[i] = s_good[i]; r.parallax[i] = s_par[i]; }
    if (win >= 0) {
      for (int k = 0; k < 9; k++) a.R21[9 * (size_t)p + k] = P.R[win][k];
      for (int k = 0; k < 3; k++) a.t21[3 * (size_t)p + k] = P.t[win][k];
    }
  }
  __syncthreads();
  const int win = s_win;
  if (win < 0) return;                                         // rejected: the outputs stay as they were
  for (int i = tid; i < P.n1; i += 512) a.tri[(size_t)P.off1 + i] = 0;
  __syncthreads();
  const size_t base = (size_t)win * a.n1_total + P.off1;
  for (int k = tid; k < n; k += 512) {
    const uint8_t f = a.rt_flag[base + k];
    if (!(f & 1)) continue;
    const size_t row = (size_t)P.off1 + a.mlist[2 * ((size_t)P.off1 + k)];
    for (int c = 0; c < 3; c++) a.P3D[3 * row + c] = a.rt_p[3 * (base + k) + c];
    if (f & 2) a.tri[row] = 1;
  }
}

// workspace layout (bytes, 256-aligned pieces)
struct InitWs {
  size_t pair, mlist, pn1, pn2, hyp, score, inl, rt_p, rt_cos, rt_flag, total;
};
static InitWs init_ws_layout(int npairs, int n1_total, int n2_total, int iterations) {
  InitWs w;
  Carve blk;
  const size_t P = (size_t)npairs, N1 = (size_t)n1_total, N2 = (size_t)n2_total, I = (size_t)iterations;
  w.pair = blk.take(sizeof(InitPair) * P); w.mlist = blk.take(8 * N1); w.pn1 = blk.take(8 * N1); w.pn2 = blk.take(8 * N2);
  w.hyp = blk.take(27 * 8 * P * I); w.score = blk.take(2 * 4 * P * I); w.inl = blk.take(2 * N1);
  w.rt_p = blk.take(8 * 24 * N1); w.rt_cos = blk.take(8 * 4 * N1); w.rt_flag = blk.take(8 * N1);
  w.total = blk.total;
  return w;
}

static bool init_counts_ok(int npairs, int n1_total, int n2_total, int iterations) {
  return npairs >= 1 && npairs <= ORBT_INIT_MAX_PAIRS && n1_total >= 0 && n2_total >= 0 && iterations >= 1 && iterations <= ORBT_INIT_MAX_ITERATIONS &&
         (long long)n1_total <= (long long)ORBT_INIT_MAX_N * npairs && (long long)n2_total <= (long long)ORBT_INIT_MAX_N * npairs;
}

}  // namespace orbhip

extern "C" {

int orbt_initialize_workspace(int npairs, int n1_total, int n2_total, int iterations, size_t* bytes) {
  using namespace orbhip;
  ORBHIP_REQUIRE(bytes && init_counts_ok(npairs, n1_total, n2_total, iterations), ORBHIP_EINVAL, "orbt_initialize_workspace: count out of range");
  *bytes = init_ws_layout(npairs, n1_total, n2_total, iterations).total;
  return 0;
}

int orbt_initialize_batch_device(int npairs, const float* d_kps1, const int32_t* d_off1, int n1_total, const float* d_kps2, const int32_t* d_off2,
                                 int n2_total, const int32_t* d_matches12, const float* d_K4, float sigma, int iterations, const int32_t* d_ransac_sets,
                                 double* d_R21, double* d_t21, double* d_P3D, uint8_t* d_triangulated, orbt_init_report* d_report, void* d_workspace,
                                 void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(init_counts_ok(npairs, n1_total, n2_total, iterations), ORBHIP_EINVAL, "orbt_initialize: count out of range");
  ORBHIP_REQUIRE(sigma > 0.0f && sigma < INFINITY, ORBHIP_EINVAL, "orbt_initialize: sigma must be positive and finite");
  ORBHIP_REQUIRE(d_kps1 && d_off1 && d_kps2 && d_off2 && d_matches12 && d_K4 && d_ransac_sets && d_R21 && d_t21 && d_P3D && d_triangulated && d_report &&
                 d_workspace, ORBHIP_EINVAL, "orbt_initialize: NULL argument");
  const InitWs w = init_ws_layout(npairs, n1_total, n2_total, iterations);
  uint8_t* ws = (uint8_t*)d_workspace;
  InitArgs A;
  A.npairs = npairs; A.n1_total = n1_total; A.n2_total = n2_total; A.iterations = iterations; A.sigma = sigma;
  A.kps1 = d_kps1; A.off1 = d_off1; A.kps2 = d_kps2; A.off2 = d_off2; A.matches12 = d_matches12; A.K4 = d_K4; A.sets = d_ransac_sets;
  A.R21 = d_R21; A.t21 = d_t21; A.P3D = d_P3D; A.tri = d_triangulated; A.report = d_report;
  A.pair = (InitPair*)(ws + w.pair); A.mlist = (int32_t*)(ws + w.mlist); A.pn1 = (float*)(ws + w.pn1); A.pn2 = (float*)(ws + w.pn2);
  A.hyp = (double*)(ws + w.hyp); A.score = (float*)(ws + w.score); A.inl = ws + w.inl;
  A.rt_p = (double*)(ws + w.rt_p); A.rt_cos = (float*)(ws + w.rt_cos); A.rt_flag = ws + w.rt_flag;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_init_prep, dim3(npairs), dim3(INIT_WG), 0, st, A);
  hipLaunchKernelGGL(k_init_hyp, dim3((iterations + 63) / 64, 2, npairs), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_init_score, dim3(iterations, 2, npairs), dim3(INIT_WG), 0, st, A);
  hipLaunchKernelGGL(k_init_select, dim3(npairs), dim3(INIT_WG), 0, st, A);
  hipLaunchKernelGGL(k_init_checkrt, dim3(INIT_RT_BLOCKS, 8, npairs), dim3(INIT_WG), 0, st, A);
  hipLaunchKernelGGL(k_init_decide, dim3(npairs), dim3(512), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbt_initialize(const float* kps1, int n1, const float* kps2, int n2, const int32_t* matches12, const float* K4, float sigma, int iterations,
                    const int32_t* ransac_sets, double* R21, double* t21, double* P3D, uint8_t* triangulated, orbt_init_report* report,
                    const orbt_init_trace* trace) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(n1 >= 0 && n1 <= ORBT_INIT_MAX_N && n2 >= 0 && n2 <= ORBT_INIT_MAX_N, ORBHIP_EINVAL, "orbt_initialize: keypoint count out of range");
  ORBHIP_REQUIRE(iterations >= 1 && iterations <= ORBT_INIT_MAX_ITERATIONS, ORBHIP_EINVAL, "orbt_initialize: iterations out of range");
  ORBHIP_REQUIRE(sigma > 0.0f && sigma < INFINITY, ORBHIP_EINVAL, "orbt_initialize: sigma must be positive and finite");
  ORBHIP_REQUIRE((kps1 || n1 == 0) && (kps2 || n2 == 0) && (matches12 || n1 == 0) && K4 && ransac_sets && R21 && t21 && (P3D || n1 == 0) &&
                 (triangulated || n1 == 0) && report, ORBHIP_EINVAL, "orbt_initialize: NULL argument");
  int nm = 0;
  for (int i = 0; i < n1; i++) {
    ORBHIP_REQUIRE(matches12[i] >= -1 && matches12[i] < n2, ORBHIP_EINVAL, "orbt_initialize: matches12 entry outside [-1, n2)");
    nm += matches12[i] >= 0;
  }
  ORBHIP_REQUIRE(nm >= 8, ORBHIP_EINVAL, "orbt_initialize: fewer than 8 matches");
  for (size_t j = 0; j < (size_t)iterations * 8; j++)
    ORBHIP_REQUIRE(ransac_sets[j] >= 0 && ransac_sets[j] < nm, ORBHIP_EINVAL, "orbt_initialize: RANSAC set entry outside [0, n_matches)");
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const int32_t off1[2] = {0, n1}, off2[2] = {0, n2};
  ThreadWs::Pack in;
  const int pK1 = in.add(kps1, 8 * (size_t)n1), pK2 = in.add(kps2, 8 * (size_t)n2), pM = in.add(matches12, 4 * (size_t)n1);
  const int pO1 = in.add(off1, 8), pO2 = in.add(off2, 8), pK = in.add(K4, 16), pS = in.add(ransac_sets, 32 * (size_t)iterations);
  const int pP = in.add(P3D, 24 * (size_t)n1);                // (the device copy starts as the caller's rows: untouched rows keep them)
  // outputs in one block: [R21 | t21 | triangulated | report]
  Carve blk;
  const size_t oR = blk.take(72), oT = blk.take(24), oG = blk.take((size_t)n1), oRep = blk.take(sizeof(orbt_init_report));
  const InitWs lay = init_ws_layout(1, n1, n2, iterations);
  uint8_t* dblk = W.d<uint8_t>(blk.total, &rc);
  uint8_t* dws = W.d<uint8_t>(lay.total, &rc);
  if (rc || (rc = W.commit(in))) return rc;
  double* dP = in.dev<double>(pP);
  if ((rc = orbt_initialize_batch_device(1, in.dev<float>(pK1), in.dev<int32_t>(pO1), n1, in.dev<float>(pK2), in.dev<int32_t>(pO2), n2, in.dev<int32_t>(pM),
                                         in.dev<float>(pK), sigma, iterations, in.dev<int32_t>(pS), (double*)(dblk + oR), (double*)(dblk + oT), dP,
                                         dblk + oG, (orbt_init_report*)(dblk + oRep), dws, W.s))) return rc;
  const uint8_t* hb = W.down(dblk, blk.total, &rc);
  const double* hP = W.down(dP, 3 * (size_t)n1, &rc);
  const bool want_trace = trace && (trace->H21 || trace->H12 || trace->F21 || trace->score_h || trace->score_f || trace->motion_R || trace->motion_t ||
                                    trace->inliers_h || trace->inliers_f);
  const uint8_t* hw = want_trace ? W.down(dws, lay.total, &rc) : nullptr;
  if (rc || (rc = W.sync())) return rc;
  const orbt_init_report rep = *(const orbt_init_report*)(hb + oRep);
  *report = rep;
  if (rep.reason == ORBT_INIT_OK) {                            // on failure the outputs stay as they were (:496-498, :693)
    std::memcpy(R21, hb + oR, 72); std::memcpy(t21, hb + oT, 24);
    std::memcpy(triangulated, hb + oG, (size_t)n1);
    std::memcpy(P3D, hP, 24 * (size_t)n1);
  }
  if (hw) {                                                    // the trace: read back from the workspace
    const InitPair& Pp = *(const InitPair*)(hw + lay.pair);
    const double* hyp = (const double*)(hw + lay.hyp);
    const float* sc = (const float*)(hw + lay.score);
    const bool ran = Pp.status != ORBT_INIT_BAD_INPUT;
    for (int it = 0; it < iterations; it++) {
      if (trace->H21) std::memcpy(trace->H21 + 9 * (size_t)it, hyp + 27 * (size_t)it, 72);
      if (trace->H12) std::memcpy(trace->H12 + 9 * (size_t)it, hyp + 27 * (size_t)it + 9, 72);
      if (trace->F21) std::memcpy(trace->F21 + 9 * (size_t)it, hyp + 27 * (size_t)it + 18, 72);
      if (trace->score_h) trace->score_h[it] = sc[2 * (size_t)it];
      if (trace->score_f) trace->score_f[it] = sc[2 * (size_t)it + 1];
    }
    const int nmot = ran ? Pp.n_motions : 0;
    for (int m = 0; m < 8; m++) {
      if (trace->motion_R) for (int k = 0; k < 9; k++) trace->motion_R[9 * m + k] = m < nmot ? Pp.R[m][k] : 0.0;
      if (trace->motion_t) for (int k = 0; k < 3; k++) trace->motion_t[3 * m + k] = m < nmot ? Pp.t[m][k] : 0.0;
    }
    const uint8_t* inl = hw + lay.inl;
    if (trace->inliers_h) for (int k = 0; k < nm; k++) trace->inliers_h[k] = ran && Pp.best_h >= 0 ? inl[k] : 0;
    if (trace->inliers_f) for (int k = 0; k < nm; k++) trace->inliers_f[k] = ran && Pp.best_f >= 0 ? inl[(size_t)n1 + k] : 0;
  }
  return 0;
}

}  // extern "C"
