// orb_pnp.inc -- PnPsolver::iterate (src/PnPsolver.cc:166-345: RANSAC, CheckInliers, Refine) with EPnP's compute_pose (:380-957) for a
// BATCH of relocalisation candidates (orbt_pnp_*).  Textually included by orb_track.hip.
//
// One call = one `iterate` of every candidate.  The minimal sets are an input (the reference draws them lazily from the process-global
// DUtils::Random, :192-203; the library cannot see that sequence), the best-so-far state (mnBestInliers, mvbBestInliers, mBestTcw) is an
// in/out argument.  Four launches, one stream, no allocation, no host synchronisation:
//   k_pnp_prep    one workgroup per candidate: checks offsets, counts, set entries and the incoming state; a bad candidate fails alone.
//   k_pnp_hyp     one LANE per (candidate, iteration): compute_pose on the 4 points of the set, in double.  The 12 x 12 MtM and its
//                 rotation matrix (2.3 KB together) live in LDS, element-major over the 16 lanes of a workgroup; everything else is
//                 per-lane.  16 lanes per workgroup, not 64: the chains are independent and latency-bound (a relocalisation has
//                 35 x a few tens of them), a wave waits for its slowest lane's Jacobi sweeps, and 16-lane groups spread the chains
//                 over four times as many compute units.  Every hypothesis of the call is computed, also those after the one the
//                 sequential rule stops at: they are speculative and leave no trace in any output.
//   k_pnp_count   one workgroup per (candidate, iteration): CheckInliers with the reference's float / double promotions (:313-345),
//                 the count by an integer reduction (order-free).
//   k_pnp_select  one workgroup per candidate walks the iterations in order: the running strict maximum from the incoming state
//                 (:210-227), Refine (:263-310) on the best-so-far mask - once per new record, and once for the incoming mask when an
//                 iteration qualifies before any new record, because Refine depends on nothing but that mask - and stops at the first
//                 refit with more than min_inliers inliers.  Refine's compute_pose runs on n = |best mask| points with the whole
//                 workgroup: every sum over the points is 256 strided partial sums (lane j adds points j, j + 256, ... in order)
//                 combined by a fixed binary tree (s = 128, 64, ... 1: p[j] += p[j + s]); the dense part runs on lane 0.
// The 4-point compute_pose is the same code with one partial sum (plain index order).  tests/nppnp.py restates every step in this
// operation order; DESIGN.md section 2 ("PnP RANSAC") says what is pinned and what cannot be.
#include "small_dense.h"
namespace orbhip {

#define PNP_WG 256
#define PNP_HYP_LANES 16

struct PnpCand {                      // per-candidate record in the workspace
  int32_t status;                     // 0 = runs, else ORBT_PNP_TOO_FEW / ORBT_PNP_BAD_INPUT
  int32_t off, n, n_sets, min_inl, pad;
};

struct PnpArgs {
  int ncand, n_total, iterations;
  const float* p3d; const float* p2d; const float* max_err; const int32_t* off; const float* K4; const int32_t* min_inl; const int32_t* n_sets;
  const int32_t* sets;
  int32_t* best_count; uint8_t* best_mask; double* best_T;
  orbt_pnp_result* result; uint8_t* inliers;
  // workspace
  PnpCand* cand;
  double* hyp;                        // [ncand][iterations][16]: R (9) | t (3) | reprojection error | chosen approximation N
  int32_t* count;                     // [ncand][iterations]
  int32_t* ridx;                      // [n_total]: the indices Refine fits, ascending
  double* refit;                      // [ncand][iterations][14]: iteration | R (9) | t (3) | count
};

// the points one compute_pose call fits: rows idx[0 .. n) of the candidate's p3d / p2d
struct PnpPts {
  const float* p3d; const float* p2d; const int32_t* idx; int n;
  double fu, fv, uc, vc;
};
__device__ __forceinline__ void pnp_pw(const PnpPts& P, int i, double* pw) {
  const float* p = P.p3d + 3 * (size_t)P.idx[i];
  pw[0] = p[0]; pw[1] = p[1]; pw[2] = p[2];
}
__device__ __forceinline__ void pnp_uv(const PnpPts& P, int i, double& u, double& v) {
  const float* p = P.p2d + 2 * (size_t)P.idx[i];
  u = p[0]; v = p[1];
}

// ---- who adds: one lane (a hypothesis) or a workgroup (a refit)
struct PnpLane {
  DView A, V;
  __device__ __forceinline__ bool leader() const { return true; }
  __device__ __forceinline__ void sync() const {}
  template <int K, class F>
  __device__ __forceinline__ void sum(int n, F f, double* out) const {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = 0.0;
    for (int i = 0; i < n; i++) {
      double v[K];
      f(i, v);
#pragma unroll
      for (int k = 0; k < K; k++) acc[k] += v[k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = acc[k];
  }
  __device__ __forceinline__ void bcast(double*, int) const {}
};
struct PnpWg {
  DView A, V;
  double* red;                        // LDS [12][PNP_WG]
  double* bc;                         // LDS [36]
  int tid;
  __device__ __forceinline__ bool leader() const { return tid == 0; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  template <int K, class F>
  __device__ __forceinline__ void sum(int n, F f, double* out) const {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += PNP_WG) {
      double v[K];
      f(i, v);
#pragma unroll
      for (int k = 0; k < K; k++) acc[k] += v[k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) red[k * PNP_WG + tid] = acc[k];
    __syncthreads();
    for (int s = PNP_WG / 2; s >= 1; s >>= 1) {
      if (tid < s) {
#pragma unroll
        for (int k = 0; k < K; k++) red[k * PNP_WG + tid] += red[k * PNP_WG + tid + s];
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = red[k * PNP_WG];
    __syncthreads();
  }
  __device__ __forceinline__ void bcast(double* x, int n) const {
    if (tid == 0) for (int i = 0; i < n; i++) bc[i] = x[i];
    __syncthreads();
    for (int i = 0; i < n; i++) x[i] = bc[i];
    __syncthreads();
  }
};

__device__ __forceinline__ double pnp_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// (:428-438) barycentric coordinates of one point
__device__ __forceinline__ void pnp_alphas(const double* pw, const double* c0, const double* ci, double* a) {
  const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
#pragma unroll
  for (int j = 0; j < 3; j++) a[1 + j] = (ci[3 * j] * d0 + ci[3 * j + 1] * d1) + ci[3 * j + 2] * d2;
  a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

// (:865-957) qr_solve for the 6 x 4 Gauss-Newton system.  A singular column (eta == 0) ends the reference's function before it writes
// X, which is uninitialised on the first step there: here that is a step of zero.
__device__ inline void pnp_qr_solve(double* A, double* b, double* X) {
  const int nr = 6, nc = 4;
  double A1[4], A2[4];
  for (int k = 0; k < nc; k++) X[k] = 0.0;
  for (int k = 0; k < nc; k++) {
    double eta = fabs(A[k * nc + k]);
    for (int i = k + 1; i < nr; i++) {                         // (:885-890: the pointer starts at row k and is read before it moves: rows k .. nr - 2)
      const double elt = fabs(A[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) return;
    const double inv_eta = 1.0 / eta;
    double sum = 0.0;
    for (int i = k; i < nr; i++) { A[i * nc + k] *= inv_eta; sum += A[i * nc + k] * A[i * nc + k]; }
    double sigma = sqrt(sum);
    if (A[k * nc + k] < 0) sigma = -sigma;
    A[k * nc + k] += sigma;
    A1[k] = sigma * A[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double s2 = 0;
      for (int i = k; i < nr; i++) s2 += A[i * nc + k] * A[i * nc + j];
      const double tau = s2 / A1[k];
      for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
    }
  }
  for (int j = 0; j < nc; j++) {                               // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
    tau /= A1[j];
    for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
  }
  X[nc - 1] = b[nc - 1] / A2[nc - 1];                          // X = R^-1 b
  for (int i = nc - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * X[j];
    X[i] = (b[i] - sum) / A2[i];
  }
}

// (:845-863, :817-843) five Gauss-Newton steps on the betas
__device__ inline void pnp_gauss_newton(const double* L, const double* rho, double* betas) {
  for (int k = 0; k < 5; k++) {
    double A[24], b[6], x[4];
    for (int i = 0; i < 6; i++) {
      const double* r = L + 10 * i;
      A[4 * i] = (((2 * r[0]) * betas[0] + r[1] * betas[1]) + r[3] * betas[2]) + r[6] * betas[3];
      A[4 * i + 1] = ((r[1] * betas[0] + (2 * r[2]) * betas[1]) + r[4] * betas[2]) + r[7] * betas[3];
      A[4 * i + 2] = ((r[3] * betas[0] + r[4] * betas[1]) + (2 * r[5]) * betas[2]) + r[8] * betas[3];
      A[4 * i + 3] = ((r[6] * betas[0] + r[7] * betas[1]) + r[8] * betas[2]) + (2 * r[9]) * betas[3];
      double s = (r[0] * betas[0]) * betas[0];
      s += (r[1] * betas[0]) * betas[1];
      s += (r[2] * betas[1]) * betas[1];
      s += (r[3] * betas[0]) * betas[2];
      s += (r[4] * betas[1]) * betas[2];
      s += (r[5] * betas[2]) * betas[2];
      s += (r[6] * betas[0]) * betas[3];
      s += (r[7] * betas[1]) * betas[3];
      s += (r[8] * betas[2]) * betas[3];
      s += (r[9] * betas[3]) * betas[3];
      b[i] = rho[i] - s;
    }
    pnp_qr_solve(A, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

// The dense middle of compute_pose (:492-521 without the sums over the points): the eigenvectors of MtM (A, destroyed; V), L_6x10 and
// rho, the three find_betas_approx_* each followed by gauss_newton, and compute_ccs for each: ccs3[a][j][k], a = approximation 1..3.
// cvSVD's Ut rows 11, 10, 9, 8 are the columns of V with the four smallest |A V_j|^2, ascending; the order of all twelve is the
// stable descending sort of those squared norms.
__device__ inline void pnp_betas(const DView A, const DView V, const double (*cws)[3], double* ccs3) {
  d_jacobi(A, 12, 12, V);
  double nrm2[12];
  d_col_norm2(A, 12, 12, nrm2);
  int ord[12];
  for (int i = 0; i < 12; i++) ord[i] = i;
  for (int i = 1; i < 12; i++)                                 // insertion sort, descending, stable
    for (int j = i; j > 0 && nrm2[ord[j - 1]] < nrm2[ord[j]]; j--) { const int tmp = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = tmp; }
  int vc[4];
  for (int i = 0; i < 4; i++) vc[i] = ord[11 - i];             // v[i] = Ut row 11 - i
  double L[60], rho[6];
  {                                                            // compute_L_6x10 (:765-805)
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
      int a = 0, b = 1;
      for (int j = 0; j < 6; j++) {
        for (int k = 0; k < 3; k++) dv[i][j][k] = V[(3 * a + k) * 12 + vc[i]] - V[(3 * b + k) * 12 + vc[i]];
        b++;
        if (b > 3) { a++; b = a + 1; }
      }
    }
    for (int i = 0; i < 6; i++) {
      double* row = L + 10 * i;
      row[0] = pnp_dot3(dv[0][i], dv[0][i]);
      row[1] = 2.0 * pnp_dot3(dv[0][i], dv[1][i]);
      row[2] = pnp_dot3(dv[1][i], dv[1][i]);
      row[3] = 2.0 * pnp_dot3(dv[0][i], dv[2][i]);
      row[4] = 2.0 * pnp_dot3(dv[1][i], dv[2][i]);
      row[5] = pnp_dot3(dv[2][i], dv[2][i]);
      row[6] = 2.0 * pnp_dot3(dv[0][i], dv[3][i]);
      row[7] = 2.0 * pnp_dot3(dv[1][i], dv[3][i]);
      row[8] = 2.0 * pnp_dot3(dv[2][i], dv[3][i]);
      row[9] = pnp_dot3(dv[3][i], dv[3][i]);
    }
  }
  {                                                            // compute_rho (:807-815)
    int k = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a + 1; b < 4; b++) {
        const double d0 = cws[a][0] - cws[b][0], d1 = cws[a][1] - cws[b][1], d2 = cws[a][2] - cws[b][2];
        rho[k++] = (d0 * d0 + d1 * d1) + d2 * d2;
      }
  }
  double betas[3][4];
  double tA[30], tV[25], x[5];
  const DView vA = {tA, 1}, vV = {tV, 1};
  {                                                            // find_betas_approx_1 (:672-699): columns 0, 1, 3, 6
    const int cols[4] = {0, 1, 3, 6};
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 4; j++) tA[4 * i + j] = L[10 * i + cols[j]];
    d_lstsq(vA, 6, 4, vV, rho, x);
    double* be = betas[0];
    if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = -x[1] / be[0]; be[2] = -x[2] / be[0]; be[3] = -x[3] / be[0]; }
    else { be[0] = sqrt(x[0]); be[1] = x[1] / be[0]; be[2] = x[2] / be[0]; be[3] = x[3] / be[0]; }
  }
  {                                                            // find_betas_approx_2 (:704-731): columns 0, 1, 2
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 3; j++) tA[3 * i + j] = L[10 * i + j];
    d_lstsq(vA, 6, 3, vV, rho, x);
    double* be = betas[1];
    if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0; }
    else { be[0] = sqrt(x[0]); be[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0; }
    if (x[1] < 0) be[0] = -be[0];
    be[2] = 0.0; be[3] = 0.0;
  }
  {                                                            // find_betas_approx_3 (:736-763): columns 0 .. 4
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 5; j++) tA[5 * i + j] = L[10 * i + j];
    d_lstsq(vA, 6, 5, vV, rho, x);
    double* be = betas[2];
    if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0; }
    else { be[0] = sqrt(x[0]); be[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0; }
    if (x[1] < 0) be[0] = -be[0];
    be[2] = x[3] / be[0];
    be[3] = 0.0;
  }
  for (int a = 0; a < 3; a++) {
    pnp_gauss_newton(L, rho, betas[a]);
    for (int j = 0; j < 12; j++) {                             // compute_ccs (:458-469)
      double s = 0.0;
      for (int i = 0; i < 4; i++) s += betas[a][i] * V[j * 12 + vc[i]];
      ccs3[12 * a + j] = s;
    }
  }
}

// compute_pose (:482-530).  Called by every lane of the context; R (9, row-major), t (3), the chosen approximation (1..3) and its
// mean reprojection error come back in every lane.
template <class Ctx>
__device__ inline void pnp_compute_pose(const Ctx& cx, const PnpPts& P, double* R, double* t, int* Nsel, double* errsel) {
  const int n = P.n;
  const double dn = (double)n;
  // choose_control_points (:380-414)
  double c0[3];
  cx.template sum<3>(n, [&](int i, double* v) { pnp_pw(P, i, v); }, c0);
#pragma unroll
  for (int j = 0; j < 3; j++) c0[j] = c0[j] / dn;
  double c6[6];
  cx.template sum<6>(n, [&](int i, double* v) {
    double pw[3];
    pnp_pw(P, i, pw);
    const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
    v[0] = d0 * d0; v[1] = d0 * d1; v[2] = d0 * d2; v[3] = d1 * d1; v[4] = d1 * d2; v[5] = d2 * d2;
  }, c6);
  double cws[4][3], ci[9];
  {
    const double cov[9] = {c6[0], c6[1], c6[2], c6[1], c6[3], c6[4], c6[2], c6[4], c6[5]};
    double Uc[9], dc[3], Vc[9];
    i_svd3(cov, Uc, dc, Vc);
#pragma unroll
    for (int j = 0; j < 3; j++) cws[0][j] = c0[j];
#pragma unroll
    for (int i = 1; i < 4; i++) {
      const double k = sqrt(dc[i - 1] / dn);
#pragma unroll
      for (int j = 0; j < 3; j++) cws[i][j] = c0[j] + k * Vc[3 * j + (i - 1)];
    }
    // compute_barycentric_coordinates (:416-426): cvInvert(CV_SVD) = V S^+ U^T, a singular value at or below 1e-12 of the largest is zero
    double cc[9], U[9], S[3], V[9], sinv[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
    i_svd3(cc, U, S, V);
#pragma unroll
    for (int k = 0; k < 3; k++) sinv[k] = S[k] > 1e-12 * S[0] ? 1.0 / S[k] : 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        ci[3 * r + c] = ((V[3 * r] * sinv[0]) * U[3 * c] + (V[3 * r + 1] * sinv[1]) * U[3 * c + 1]) + (V[3 * r + 2] * sinv[2]) * U[3 * c + 2];
  }
  // fill_M (:441-456) and MtM = M^T M, one row of the upper triangle per pass: a point adds M1[r] M1[c] + M2[r] M2[c]
  for (int r = 0; r < 12; r++) {
    double row[12];
    cx.template sum<12>(n, [&](int i, double* v) {
      double pw[3], a[4], u, vv, M1[12], M2[12];
      pnp_pw(P, i, pw);
      pnp_uv(P, i, u, vv);
      pnp_alphas(pw, c0, ci, a);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        M1[3 * k] = a[k] * P.fu; M1[3 * k + 1] = 0.0; M1[3 * k + 2] = a[k] * (P.uc - u);
        M2[3 * k] = 0.0; M2[3 * k + 1] = a[k] * P.fv; M2[3 * k + 2] = a[k] * (P.vc - vv);
      }
      double m1r = M1[0], m2r = M2[0];
#pragma unroll
      for (int k = 1; k < 12; k++) { m1r = r == k ? M1[k] : m1r; m2r = r == k ? M2[k] : m2r; }
#pragma unroll
      for (int c = 0; c < 12; c++) v[c] = c >= r ? m1r * M1[c] + m2r * M2[c] : 0.0;
    }, row);
    if (cx.leader())
      for (int c = r; c < 12; c++) { cx.A[r * 12 + c] = row[c]; cx.A[c * 12 + r] = row[c]; }
  }
  cx.sync();
  double ccs3[36];
  if (cx.leader()) pnp_betas(cx.A, cx.V, cws, ccs3);
  cx.bcast(ccs3, 36);
  // compute_R_and_t (:656-667) per approximation
  double pw_0[3], a_0[4];
  pnp_pw(P, 0, pw_0);
  pnp_alphas(pw_0, c0, ci, a_0);
  double best_err = 0.0;
  int best_n = 0;
  for (int ap = 0; ap < 3; ap++) {
    double ccs[12];
#pragma unroll
    for (int k = 0; k < 12; k++) ccs[k] = ccs3[12 * ap + k];
    // solve_for_sign (:641-654) on the z of the first point
    const double z0 = ((a_0[0] * ccs[2] + a_0[1] * ccs[5]) + a_0[2] * ccs[8]) + a_0[3] * ccs[11];
    if (z0 < 0.0) {
#pragma unroll
      for (int k = 0; k < 12; k++) ccs[k] = -ccs[k];
    }
    auto pc_of = [&](int i, double* pw, double* pc) {           // compute_pcs (:471-480)
      double a[4];
      pnp_pw(P, i, pw);
      pnp_alphas(pw, c0, ci, a);
#pragma unroll
      for (int j = 0; j < 3; j++) pc[j] = ((a[0] * ccs[j] + a[1] * ccs[3 + j]) + a[2] * ccs[6 + j]) + a[3] * ccs[9 + j];
    };
    // estimate_R_and_t (:574-632); pw0 is the centroid c0 (the same sum, the same division)
    double pc0[3];
    cx.template sum<3>(n, [&](int i, double* v) { double pw[3]; pc_of(i, pw, v); }, pc0);
#pragma unroll
    for (int j = 0; j < 3; j++) pc0[j] = pc0[j] / dn;
    double abt[9];
    cx.template sum<9>(n, [&](int i, double* v) {
      double pw[3], pc[3];
      pc_of(i, pw, pc);
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double dj = pc[j] - pc0[j];
        v[3 * j] = dj * (pw[0] - c0[0]); v[3 * j + 1] = dj * (pw[1] - c0[1]); v[3 * j + 2] = dj * (pw[2] - c0[2]);
      }
    }, abt);
    double U[9], S[3], V[9], Ra[9], ta[3];
    i_svd3(abt, U, S, V);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) Ra[3 * i + j] = (U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1]) + U[3 * i + 2] * V[3 * j + 2];
    const double det = (((((Ra[0] * Ra[4]) * Ra[8] + (Ra[1] * Ra[5]) * Ra[6]) + (Ra[2] * Ra[3]) * Ra[7]) - (Ra[2] * Ra[4]) * Ra[6]) -
                        (Ra[1] * Ra[3]) * Ra[8]) - (Ra[0] * Ra[5]) * Ra[7];
    if (det < 0) { Ra[6] = -Ra[6]; Ra[7] = -Ra[7]; Ra[8] = -Ra[8]; }
#pragma unroll
    for (int i = 0; i < 3; i++) ta[i] = pc0[i] - pnp_dot3(Ra + 3 * i, c0);
    // reprojection_error (:555-572): the mean of the distances (not of their squares)
    double e1[1];
    cx.template sum<1>(n, [&](int i, double* v) {
      double pw[3], u, vv;
      pnp_pw(P, i, pw);
      pnp_uv(P, i, u, vv);
      const double Xc = pnp_dot3(Ra, pw) + ta[0], Yc = pnp_dot3(Ra + 3, pw) + ta[1], inv_Zc = 1.0 / (pnp_dot3(Ra + 6, pw) + ta[2]);
      const double ue = P.uc + (P.fu * Xc) * inv_Zc, ve = P.vc + (P.fv * Yc) * inv_Zc;
      v[0] = sqrt((u - ue) * (u - ue) + (vv - ve) * (vv - ve));
    }, e1);
    const double err = e1[0] / dn;
    // (:523-525) N = 1; if (e2 < e1) N = 2; if (e3 < e[N]) N = 3
    if (ap == 0 || err < best_err) {
      best_err = err; best_n = ap + 1;
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = Ra[k];
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = ta[k];
    }
  }
  *Nsel = best_n; *errsel = best_err;
}

// CheckInliers for one point (:319-342): Xc, Yc, invZc float (a double expression, narrowed), ue / ve double, distX / distY / error2 float
__device__ __forceinline__ bool pnp_inlier(const double* R, const double* t, double fu, double fv, double uc, double vc, const float* p3, const float* p2,
                                           float max_err) {
  const double x = p3[0], y = p3[1], z = p3[2];
  const float Xc = (float)(((R[0] * x + R[1] * y) + R[2] * z) + t[0]);
  const float Yc = (float)(((R[3] * x + R[4] * y) + R[5] * z) + t[1]);
  const float invZc = (float)(1.0 / (((R[6] * x + R[7] * y) + R[8] * z) + t[2]));
  const double ue = uc + (fu * (double)Xc) * (double)invZc;
  const double ve = vc + (fv * (double)Yc) * (double)invZc;
  const float distX = (float)((double)p2[0] - ue);
  const float distY = (float)((double)p2[1] - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < max_err;
}

__global__ __launch_bounds__(PNP_WG) void k_pnp_prep(PnpArgs a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  PnpCand& C = a.cand[c];
  __shared__ int s_bad, s_pop;
  const int o = a.off[c], e = a.off[c + 1], ns = a.n_sets[c], mi = a.min_inl[c], bcnt = a.best_count[c];
  const bool shape_ok = o >= 0 && o <= e && e <= a.n_total && e - o <= ORBT_PNP_MAX_N && ns >= 0 && ns <= a.iterations && mi >= 4;
  if (!shape_ok) {
    if (tid == 0) { C.status = ORBT_PNP_BAD_INPUT; C.off = 0; C.n = 0; C.n_sets = 0; C.min_inl = 0; }
    return;
  }
  const int n = e - o;
  if (n < mi) {                                                // (:174-178) before any set or the state is looked at
    if (tid == 0) { C.status = ORBT_PNP_TOO_FEW; C.off = o; C.n = n; C.n_sets = 0; C.min_inl = mi; }
    return;
  }
  if (tid == 0) { s_bad = 0; s_pop = 0; }
  __syncthreads();
  const int32_t* sets = a.sets + (size_t)c * a.iterations * 4;
  for (int s = tid; s < ns; s += PNP_WG) {
    const int i0 = sets[4 * s], i1 = sets[4 * s + 1], i2 = sets[4 * s + 2], i3 = sets[4 * s + 3];
    const bool in = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n && i3 >= 0 && i3 < n;
    const bool distinct = i0 != i1 && i0 != i2 && i0 != i3 && i1 != i2 && i1 != i3 && i2 != i3;
    if (!in || !distinct) atomicOr(&s_bad, 1);
  }
  int pop = 0;
  for (int i = tid; i < n; i += PNP_WG) pop += a.best_mask[(size_t)o + i] != 0;
  pop = i_wave_sum(pop);
  if ((tid & 63) == 0) atomicAdd(&s_pop, pop);
  __syncthreads();
  if (tid == 0) {
    const bool state_ok = bcnt >= 0 && bcnt <= n && s_pop == bcnt;
    C.status = (s_bad || !state_ok) ? ORBT_PNP_BAD_INPUT : 0;
    C.off = o; C.n = n; C.n_sets = ns; C.min_inl = mi;
  }
}

__global__ __launch_bounds__(PNP_HYP_LANES) void k_pnp_hyp(PnpArgs a) {
  const int c = blockIdx.y, lane = threadIdx.x, it = blockIdx.x * PNP_HYP_LANES + lane;
  __shared__ double sA[144 * PNP_HYP_LANES], sV[144 * PNP_HYP_LANES];
  const PnpCand& C = a.cand[c];
  if (C.status || it >= C.n_sets) return;
  const float* K4 = a.K4 + 4 * (size_t)c;
  PnpPts P;
  P.p3d = a.p3d + 3 * (size_t)C.off; P.p2d = a.p2d + 2 * (size_t)C.off;
  P.idx = a.sets + ((size_t)c * a.iterations + it) * 4; P.n = 4;
  P.fu = K4[0]; P.fv = K4[1]; P.uc = K4[2]; P.vc = K4[3];
  PnpLane cx;
  cx.A = DView{sA + lane, PNP_HYP_LANES}; cx.V = DView{sV + lane, PNP_HYP_LANES};
  double R[9], t[3], err; int N;
  pnp_compute_pose(cx, P, R, t, &N, &err);
  double* out = a.hyp + ((size_t)c * a.iterations + it) * 16;
  for (int k = 0; k < 9; k++) out[k] = R[k];
  for (int k = 0; k < 3; k++) out[9 + k] = t[k];
  out[12] = err; out[13] = (double)N; out[14] = 0.0; out[15] = 0.0;
}

__global__ __launch_bounds__(PNP_WG) void k_pnp_count(PnpArgs a) {
  const int it = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const PnpCand& C = a.cand[c];
  if (C.status || it >= C.n_sets) return;
  __shared__ int s_cnt;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const double* h = a.hyp + ((size_t)c * a.iterations + it) * 16;
  double R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = h[k];
  for (int k = 0; k < 3; k++) t[k] = h[9 + k];
  const float* K4 = a.K4 + 4 * (size_t)c;
  const double fu = K4[0], fv = K4[1], uc = K4[2], vc = K4[3];
  int cnt = 0;
  for (int i = tid; i < C.n; i += PNP_WG) {
    const size_t r = (size_t)C.off + i;
    cnt += pnp_inlier(R, t, fu, fv, uc, vc, a.p3d + 3 * r, a.p2d + 2 * r, a.max_err[r]);
  }
  cnt = i_wave_sum(cnt);
  if ((tid & 63) == 0) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (tid == 0) a.count[(size_t)c * a.iterations + it] = s_cnt;
}

// mask[i] = CheckInliers of (R, t) over the candidate's points; returns the count in every lane
__device__ inline int pnp_mask(const PnpArgs& a, const PnpCand& C, const double* R, const double* t, const double* K, uint8_t* mask, int* s_cnt) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_cnt = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < C.n; i += PNP_WG) {
    const size_t r = (size_t)C.off + i;
    const bool in = pnp_inlier(R, t, K[0], K[1], K[2], K[3], a.p3d + 3 * r, a.p2d + 2 * r, a.max_err[r]);
    mask[r] = in; cnt += in;
  }
  cnt = i_wave_sum(cnt);
  if ((tid & 63) == 0) atomicAdd(s_cnt, cnt);
  __syncthreads();
  const int total = *s_cnt;
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(PNP_WG) void k_pnp_select(PnpArgs a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const PnpCand C = a.cand[c];
  orbt_pnp_result& res = a.result[c];
  __shared__ double sA[144], sV[144], s_red[12 * PNP_WG], s_bc[36];
  __shared__ int s_cnt, s_scan[PNP_WG];
  if (C.status == ORBT_PNP_BAD_INPUT) {                        // status only: Tcw, the mask and the state stay as they were
    if (tid == 0) { res.status = ORBT_PNP_BAD_INPUT; res.consumed = 0; res.n_inliers = 0; res.n_refits = 0; }
    return;
  }
  const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  uint8_t* inl = a.inliers;                                    // (rows C.off .. C.off + C.n)
  if (C.status == ORBT_PNP_TOO_FEW) {                          // (:174-178) identity, no inliers, the state untouched
    for (int i = tid; i < C.n; i += PNP_WG) inl[(size_t)C.off + i] = 0;
    if (tid == 0) {
      res.status = ORBT_PNP_TOO_FEW; res.consumed = 0; res.n_inliers = 0; res.n_refits = 0;
      for (int k = 0; k < 16; k++) res.Tcw[k] = ident[k];
    }
    return;
  }
  const float* K4 = a.K4 + 4 * (size_t)c;
  const double K[4] = {K4[0], K4[1], K4[2], K4[3]};
  PnpWg cx;
  cx.A = DView{sA, 1}; cx.V = DView{sV, 1}; cx.red = s_red; cx.bc = s_bc; cx.tid = tid;
  int best = a.best_count[c];
  bool refit_known = false;                                    // Refine's outcome for the current best mask is known (and was a failure)
  int n_refits = 0;
  double* rf = a.refit + (size_t)c * a.iterations * 14;
  for (int it = 0; it < C.n_sets; it++) {
    const int cnt = a.count[(size_t)c * a.iterations + it];
    if (cnt < C.min_inl) continue;                             // (:210)
    if (cnt > best) {                                          // (:213-227) a new record: its mask and pose become the state
      const double* h = a.hyp + ((size_t)c * a.iterations + it) * 16;
      double R[9], t[3];
      for (int k = 0; k < 9; k++) R[k] = h[k];
      for (int k = 0; k < 3; k++) t[k] = h[9 + k];
      best = pnp_mask(a, C, R, t, K, a.best_mask, &s_cnt);
      if (tid == 0) {
        double* T = a.best_T + 16 * (size_t)c;
        for (int i = 0; i < 3; i++) { T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2]; T[4 * i + 3] = t[i]; }
        T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
        a.best_count[c] = best;
      }
      refit_known = false;
    }
    if (refit_known) continue;                                 // the same mask gives the same refit: it failed, it fails again
    // Refine (:263-310): the indices of the best mask, ascending (a workgroup scan over contiguous chunks)
    const int chunk = (C.n + PNP_WG - 1) / PNP_WG, lo = min(tid * chunk, C.n), hi = min(lo + chunk, C.n);
    int mine = 0;
    for (int i = lo; i < hi; i++) mine += a.best_mask[(size_t)C.off + i] != 0;
    s_scan[tid] = mine;
    __syncthreads();
    if (tid == 0) {
      int run = 0;
      for (int k = 0; k < PNP_WG; k++) { const int v = s_scan[k]; s_scan[k] = run; run += v; }
      s_cnt = run;
    }
    __syncthreads();
    int w = s_scan[tid];
    for (int i = lo; i < hi; i++)
      if (a.best_mask[(size_t)C.off + i]) a.ridx[(size_t)C.off + w++] = i;
    const int nfit = s_cnt;
    __syncthreads();
    PnpPts P;
    P.p3d = a.p3d + 3 * (size_t)C.off; P.p2d = a.p2d + 2 * (size_t)C.off; P.idx = a.ridx + C.off; P.n = nfit;
    P.fu = K[0]; P.fv = K[1]; P.uc = K[2]; P.vc = K[3];
    double R[9], t[3], err; int N;
    pnp_compute_pose(cx, P, R, t, &N, &err);
    const int rcnt = pnp_mask(a, C, R, t, K, inl, &s_cnt);     // (a failed refit's mask is overwritten below or by a later refit)
    if (tid == 0) {
      double* q = rf + 14 * (size_t)n_refits;
      q[0] = (double)it;
      for (int k = 0; k < 9; k++) q[1 + k] = R[k];
      for (int k = 0; k < 3; k++) q[10 + k] = t[k];
      q[13] = (double)rcnt;
    }
    n_refits++;
    refit_known = true;
    if (rcnt > C.min_inl) {                                    // (:295) strictly more: iterate returns the refined pose (:229-239)
      if (tid == 0) {
        res.status = ORBT_PNP_REFINED; res.consumed = it + 1; res.n_inliers = rcnt; res.n_refits = n_refits;
        for (int i = 0; i < 3; i++) { res.Tcw[4 * i] = R[3 * i]; res.Tcw[4 * i + 1] = R[3 * i + 1]; res.Tcw[4 * i + 2] = R[3 * i + 2]; res.Tcw[4 * i + 3] = t[i]; }
        res.Tcw[12] = 0; res.Tcw[13] = 0; res.Tcw[14] = 0; res.Tcw[15] = 1;
      }
      return;
    }
  }
  // (:244-260) every set used
  const bool have = best >= C.min_inl;
  for (int i = tid; i < C.n; i += PNP_WG) inl[(size_t)C.off + i] = have ? (uint8_t)(a.best_mask[(size_t)C.off + i] != 0) : (uint8_t)0;
  if (tid == 0) {
    res.status = have ? ORBT_PNP_EXHAUSTED_BEST : ORBT_PNP_EXHAUSTED_NONE; res.consumed = C.n_sets; res.n_inliers = have ? best : 0; res.n_refits = n_refits;
    const double* T = a.best_T + 16 * (size_t)c;
    for (int k = 0; k < 16; k++) res.Tcw[k] = have ? T[k] : ident[k];
  }
}

// workspace layout (bytes, 256-aligned pieces)
struct PnpWs {
  size_t cand, hyp, count, ridx, refit, total;
};
static PnpWs pnp_ws_layout(int ncand, int n_total, int iterations) {
  PnpWs w;
  Carve blk;
  const size_t Cn = (size_t)ncand, N = (size_t)n_total, I = (size_t)iterations;
  w.cand = blk.take(sizeof(PnpCand) * Cn); w.hyp = blk.take(16 * 8 * Cn * I); w.count = blk.take(4 * Cn * I); w.ridx = blk.take(4 * N); w.refit = blk.take(14 * 8 * Cn * I);
  w.total = blk.total;
  return w;
}

static bool pnp_counts_ok(int ncand, int n_total, int iterations) {
  return ncand >= 1 && ncand <= ORBT_PNP_MAX_CANDIDATES && n_total >= 0 && iterations >= 1 && iterations <= ORBT_PNP_MAX_ITERATIONS &&
         (long long)n_total <= (long long)ORBT_PNP_MAX_N * ncand;
}

}  // namespace orbhip

extern "C" {

int orbt_pnp_ransac_params(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, orbt_pnp_params* out) {
  ORBHIP_REQUIRE(out, ORBHIP_EINVAL, "orbt_pnp_ransac_params: NULL argument");
  ORBHIP_REQUIRE(min_set == 4, ORBHIP_EINVAL, "orbt_pnp_ransac_params: min_set must be 4 (EPnP's minimal set; the reference uses no other)");
  ORBHIP_REQUIRE(n >= 0 && n <= ORBT_PNP_MAX_N, ORBHIP_EINVAL, "orbt_pnp_ransac_params: n out of range");
  ORBHIP_REQUIRE(probability > 0.0 && probability < 1.0, ORBHIP_EINVAL, "orbt_pnp_ransac_params: probability must be inside (0, 1)");
  ORBHIP_REQUIRE(min_inliers >= 0 && max_iterations >= 1, ORBHIP_EINVAL, "orbt_pnp_ransac_params: min_inliers < 0 or max_iterations < 1");
  ORBHIP_REQUIRE(epsilon > 0.0f && epsilon <= 1.0f, ORBHIP_EINVAL, "orbt_pnp_ransac_params: epsilon must be inside (0, 1]");
  // (:130-153)
  int nMin = (int)((float)n * epsilon);
  if (nMin < min_inliers) nMin = min_inliers;
  if (nMin < min_set) nMin = min_set;
  float eps = epsilon;
  int its = 1;
  if (n > 0) {
    if (eps < (float)nMin / (float)n) eps = (float)nMin / (float)n;
    if (nMin != n) {
      // ceil() of a NaN (epsilon above 1: n < nMin) or of a value outside int converts to INT_MIN on x86-64, which :153 raises to 1
      const double v = std::ceil(std::log(1.0 - probability) / std::log(1.0 - std::pow((double)eps, 3)));
      its = !(v >= 1.0) ? 1 : v > (double)max_iterations ? max_iterations : (int)v;
    }
  }
  if (its > max_iterations) its = max_iterations;
  if (its < 1) its = 1;
  out->n = n; out->min_inliers = nMin; out->max_iterations = its; out->epsilon = eps;
  return 0;
}

int orbt_pnp_iterate_workspace(int n_candidates, int n_total, int iterations, size_t* bytes) {
  using namespace orbhip;
  ORBHIP_REQUIRE(bytes && pnp_counts_ok(n_candidates, n_total, iterations), ORBHIP_EINVAL, "orbt_pnp_iterate_workspace: count out of range");
  *bytes = pnp_ws_layout(n_candidates, n_total, iterations).total;
  return 0;
}

int orbt_pnp_iterate_batch_device(int n_candidates, const float* d_p3d, const float* d_p2d, const float* d_max_err, const int32_t* d_off, int n_total,
                                  const float* d_K4, const int32_t* d_min_inliers, const int32_t* d_n_sets, int iterations, const int32_t* d_sets,
                                  int32_t* d_best_count, uint8_t* d_best_mask, double* d_best_Tcw, orbt_pnp_result* d_result, uint8_t* d_inliers,
                                  void* d_workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(pnp_counts_ok(n_candidates, n_total, iterations), ORBHIP_EINVAL, "orbt_pnp_iterate: count out of range");
  ORBHIP_REQUIRE(d_p3d && d_p2d && d_max_err && d_off && d_K4 && d_min_inliers && d_n_sets && d_sets && d_best_count && d_best_mask && d_best_Tcw &&
                 d_result && d_inliers && d_workspace, ORBHIP_EINVAL, "orbt_pnp_iterate: NULL argument");
  const PnpWs w = pnp_ws_layout(n_candidates, n_total, iterations);
  uint8_t* ws = (uint8_t*)d_workspace;
  PnpArgs A;
  A.ncand = n_candidates; A.n_total = n_total; A.iterations = iterations;
  A.p3d = d_p3d; A.p2d = d_p2d; A.max_err = d_max_err; A.off = d_off; A.K4 = d_K4; A.min_inl = d_min_inliers; A.n_sets = d_n_sets; A.sets = d_sets;
  A.best_count = d_best_count; A.best_mask = d_best_mask; A.best_T = d_best_Tcw; A.result = d_result; A.inliers = d_inliers;
  A.cand = (PnpCand*)(ws + w.cand); A.hyp = (double*)(ws + w.hyp); A.count = (int32_t*)(ws + w.count); A.ridx = (int32_t*)(ws + w.ridx);
  A.refit = (double*)(ws + w.refit);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pnp_prep, dim3(n_candidates), dim3(PNP_WG), 0, st, A);
  hipLaunchKernelGGL(k_pnp_hyp, dim3((iterations + PNP_HYP_LANES - 1) / PNP_HYP_LANES, n_candidates), dim3(PNP_HYP_LANES), 0, st, A);
  hipLaunchKernelGGL(k_pnp_count, dim3(iterations, n_candidates), dim3(PNP_WG), 0, st, A);
  hipLaunchKernelGGL(k_pnp_select, dim3(n_candidates), dim3(PNP_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbt_pnp_iterate(const float* p3d, const float* p2d, const float* max_err, int n, const float* K4, int min_inliers, const int32_t* sets, int n_sets,
                     int32_t* best_count, uint8_t* best_mask, double* best_Tcw, orbt_pnp_result* result, uint8_t* inliers, const orbt_pnp_trace* trace) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(n >= 0 && n <= ORBT_PNP_MAX_N, ORBHIP_EINVAL, "orbt_pnp_iterate: point count out of range");
  ORBHIP_REQUIRE(n_sets >= 0 && n_sets <= ORBT_PNP_MAX_ITERATIONS, ORBHIP_EINVAL, "orbt_pnp_iterate: n_sets out of range");
  ORBHIP_REQUIRE(min_inliers >= 4, ORBHIP_EINVAL, "orbt_pnp_iterate: min_inliers below the minimal set (4)");
  ORBHIP_REQUIRE((p3d || n == 0) && (p2d || n == 0) && (max_err || n == 0) && K4 && (sets || n_sets == 0) && best_count && (best_mask || n == 0) && best_Tcw &&
                 result && (inliers || n == 0), ORBHIP_EINVAL, "orbt_pnp_iterate: NULL argument");
  if (n >= min_inliers) {
    for (int s = 0; s < n_sets; s++) {
      const int32_t* q = sets + 4 * (size_t)s;
      for (int j = 0; j < 4; j++) {
        ORBHIP_REQUIRE(q[j] >= 0 && q[j] < n, ORBHIP_EINVAL, "orbt_pnp_iterate: set entry outside [0, n)");
        for (int k = 0; k < j; k++) ORBHIP_REQUIRE(q[j] != q[k], ORBHIP_EINVAL, "orbt_pnp_iterate: an index is repeated inside a set");
      }
    }
    int pop = 0;
    for (int i = 0; i < n; i++) pop += best_mask[i] != 0;
    ORBHIP_REQUIRE(*best_count >= 0 && *best_count <= n && pop == *best_count, ORBHIP_EINVAL, "orbt_pnp_iterate: best_count does not match best_mask");
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const int iterations = n_sets > 0 ? n_sets : 1;
  const int32_t off[2] = {0, n};
  const int32_t zero_set[4] = {0, 0, 0, 0};
  ThreadWs::Pack in;
  const int pP3 = in.add(p3d, 12 * (size_t)n), pP2 = in.add(p2d, 8 * (size_t)n), pE = in.add(max_err, 4 * (size_t)n), pO = in.add(off, 8), pK = in.add(K4, 16);
  const int pMi = in.add(&min_inliers, 4), pNs = in.add(&n_sets, 4);
  const int pS = n_sets > 0 ? in.add(sets, 16 * (size_t)n_sets) : in.add(zero_set, 16);
  const int pBc = in.add(best_count, 4), pBm = in.add(best_mask, (size_t)n), pBt = in.add(best_Tcw, 128);
  const int pIn = in.add(inliers, (size_t)n);
  orbt_pnp_result r0 = *result;
  const int pR = in.add(&r0, sizeof(orbt_pnp_result));
  const PnpWs lay = pnp_ws_layout(1, n, iterations);
  uint8_t* dws = W.d<uint8_t>(lay.total, &rc);
  if (rc || (rc = W.commit(in))) return rc;
  if ((rc = orbt_pnp_iterate_batch_device(1, in.dev<float>(pP3), in.dev<float>(pP2), in.dev<float>(pE), in.dev<int32_t>(pO), n, in.dev<float>(pK),
                                          in.dev<int32_t>(pMi), in.dev<int32_t>(pNs), iterations, in.dev<int32_t>(pS), in.dev<int32_t>(pBc),
                                          in.dev<uint8_t>(pBm), in.dev<double>(pBt), in.dev<orbt_pnp_result>(pR), in.dev<uint8_t>(pIn), dws, W.s))) return rc;
  // the in/out pieces lie between best_count and the result in the packed block: one download
  const size_t o0 = in.pieces[pBc].off, o1 = in.pieces[pR].off + sizeof(orbt_pnp_result);
  const uint8_t* hb = W.down(in.dbase + o0, o1 - o0, &rc);
  const bool want_trace = trace && (trace->R || trace->t || trace->approx || trace->rep_error || trace->count || trace->refit_iteration || trace->refit_R ||
                                    trace->refit_t || trace->refit_count);
  const uint8_t* hw = want_trace ? W.down(dws, lay.total, &rc) : nullptr;
  if (rc || (rc = W.sync())) return rc;
  const orbt_pnp_result res = *(const orbt_pnp_result*)(hb + (in.pieces[pR].off - o0));
  *result = res;
  if (res.status != ORBT_PNP_BAD_INPUT) {
    *best_count = *(const int32_t*)(hb + (in.pieces[pBc].off - o0));
    if (n) std::memcpy(best_mask, hb + (in.pieces[pBm].off - o0), (size_t)n);
    std::memcpy(best_Tcw, hb + (in.pieces[pBt].off - o0), 128);
    if (n) std::memcpy(inliers, hb + (in.pieces[pIn].off - o0), (size_t)n);
  }
  if (hw) {                                                    // the trace: read back from the workspace, the consumed iterations only
    const double* hyp = (const double*)(hw + lay.hyp);
    const int32_t* cnt = (const int32_t*)(hw + lay.count);
    const double* rf = (const double*)(hw + lay.refit);
    const bool ran = res.status == ORBT_PNP_REFINED || res.status == ORBT_PNP_EXHAUSTED_BEST || res.status == ORBT_PNP_EXHAUSTED_NONE;
    for (int it = 0; it < n_sets; it++) {
      const bool used = ran && it < res.consumed;
      const double* h = hyp + 16 * (size_t)it;
      if (trace->R) for (int k = 0; k < 9; k++) trace->R[9 * (size_t)it + k] = used ? h[k] : 0.0;
      if (trace->t) for (int k = 0; k < 3; k++) trace->t[3 * (size_t)it + k] = used ? h[9 + k] : 0.0;
      if (trace->rep_error) trace->rep_error[it] = used ? h[12] : 0.0;
      if (trace->approx) trace->approx[it] = used ? (int32_t)h[13] : 0;
      if (trace->count) trace->count[it] = used ? cnt[it] : 0;
      const bool rused = ran && it < res.n_refits;
      const double* q = rf + 14 * (size_t)it;
      if (trace->refit_iteration) trace->refit_iteration[it] = rused ? (int32_t)q[0] : -1;
      if (trace->refit_R) for (int k = 0; k < 9; k++) trace->refit_R[9 * (size_t)it + k] = rused ? q[1 + k] : 0.0;
      if (trace->refit_t) for (int k = 0; k < 3; k++) trace->refit_t[3 * (size_t)it + k] = rused ? q[10 + k] : 0.0;
      if (trace->refit_count) trace->refit_count[it] = rused ? (int32_t)q[13] : 0;
    }
  }
  return 0;
}

}  // extern "C"
