// small_dense.h -- dense helpers for per-lane estimators (orb_init.inc: Initializer; orb_pnp.inc: PnPsolver / EPnP; orb_sim3solver.inc:
// Sim3Solver): 3 x 3 products / inverse / SVD, the one-sided Jacobi in the operation order of null_vector4_dev (tri_math.h) for
// compile-time shapes in registers (i_jacobi) and for run-time shapes behind a strided view (d_jacobi: 12 x 12 eigenvectors, small least
// squares), and the two-sided Jacobi for a symmetric 4 x 4 with signed eigenvalues (i_jacobi_sym4: Horn's N).
// The summation order of every function is fixed here and restated in tests/npinit.py (jacobi, svd3, inv3), tests/nppnp.py and
// tests/npsim3solver.py (jacobi_sym4).
// Domain: every comparison below is homogeneous in A, so each routine is exact under power-of-two scaling (S, U or the eigenvalues
// scale, V keeps its bits), and the routines are specified for ||A||_F within 2^+-200.  Outside that range the skip test
// |gamma| <= 1e-15 sqrt(alpha beta) overflows or underflows: a 3 x 3 with singular values 3, 2, 1 times 1e150 makes alpha beta = inf, no
// pair is rotated and i_svd3 returns 2.73, 1.83, 1.79.  No caller comes near (normalised coordinates, metric covariances).
// tests/test_small_dense_reference.py and tests/test_gpu_small_dense.py pin all of it to an mpmath reference.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace orbhip {

// ---- small 3 x 3 helpers, row-major; the summation order is fixed here and restated in tests/npinit.py
__device__ __forceinline__ void i_mm3(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void i_tr3(const double* A, double* B) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) B[3 * j + i] = A[3 * i + j];
}
__device__ __forceinline__ double i_det3(const double* a) {
  return (a[0] * (a[4] * a[8] - a[5] * a[7]) + a[1] * (a[5] * a[6] - a[3] * a[8])) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}
__device__ __forceinline__ void i_inv3(const double* a, double* r) {
  const double m[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                       a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                       a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
  const double det = (a[0] * m[0] + a[1] * m[3]) + a[2] * m[6];
#pragma unroll
  for (int k = 0; k < 9; k++) r[k] = m[k] / det;
}

// One-sided (Hestenes) Jacobi on the columns of U (M x N), V accumulates the rotations: the operation order of null_vector4_dev
// (tri_math.h) for any shape.  On return U = A V with mutually orthogonal columns.
template <int M, int N>
__device__ inline void i_jacobi(double (&U)[M][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) V[i][j] = i == j ? 1.0 : 0.0;
  // A column whose norm is below 1e-14 ||A||_F is null to working precision and is not rotated again: without this rule a
  // system with more columns than rows (F's 8 x 9) or of rank < N keeps rotating its rounding-noise column and never stops
  double fro = 0;
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int j = 0; j < N; j++) fro += U[i][j] * U[i][j];
  const double tiny = 1e-28 * fro;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; p++)
#pragma unroll
      for (int q = p + 1; q < N; q++) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int i = 0; i < M; i++) { alpha += U[i][p] * U[i][p]; beta += U[i][q] * U[i][q]; gamma += U[i][p] * U[i][q]; }
        if (gamma == 0.0 || fabs(gamma) <= 1e-15 * sqrt(alpha * beta) || alpha <= tiny || beta <= tiny) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int i = 0; i < M; i++) {
          const double up = U[i][p], uq = U[i][q];
          U[i][p] = c * up - s * uq; U[i][q] = s * up + c * uq;
        }
#pragma unroll
        for (int i = 0; i < N; i++) {
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

// Two-sided cyclic Jacobi for a SYMMETRIC 4 x 4: A <- J^T A J pair by pair until A is diagonal, V accumulates the rotations, so that on
// return A[k][k] is an eigenvalue WITH ITS SIGN and column k of V its eigenvector.  (The one-sided i_jacobi above yields singular values:
// for a matrix whose eigenvalues come in pairs +-lambda - Horn's N from three points - its column for |lambda| is an arbitrary mix of the
// two eigenvectors.)  Fixed order: at most 30 sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair is rotated when
// |A[p][q]| > 1e-18 ||A||_F of the input (the comparison is false for a NaN, so a non-finite matrix is left alone); a sweep without a
// rotation ends the run.
__device__ inline void i_jacobi_sym4(double (&A)[4][4], double (&V)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  double fro = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) fro += A[i][j] * A[i][j];
  const double tiny = 1e-18 * sqrt(fro);
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        const double apq = A[p][q];
        if (!(fabs(apq) > tiny)) continue;
        rotated = true;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[p][p] = A[p][p] - t * apq; A[q][q] = A[q][q] + t * apq;
        A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          if (r == p || r == q) continue;
          const double arp = A[r][p], arq = A[r][q];
          const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
          A[r][p] = np_; A[p][r] = np_; A[r][q] = nq_; A[q][r] = nq_;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

// the column of least norm (the smallest singular value), first on ties
template <int M, int N>
__device__ inline int i_min_col(const double (&U)[M][N]) {
  int best = 0; double bn = 1e300;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double nrm = 0;
#pragma unroll
    for (int i = 0; i < M; i++) nrm += U[i][j] * U[i][j];
    if (nrm < bn) { bn = nrm; best = j; }
  }
  return best;
}

__device__ __forceinline__ double i_sel3(const double (&B)[3][3], int i, int o) { return o == 0 ? B[i][0] : o == 1 ? B[i][1] : B[i][2]; }

// 3 x 3 SVD A = U diag(S) V^T, S descending (stable on ties), U's third column = u0 x u1 (so it is defined for rank 2), v2 signed
// so that A v2 = S2 u2 holds.  U, V row-major with the singular vectors as columns.
// For every finite A in the scale domain U and V are orthonormal and A = U diag(S) V^T to rounding, whatever the rank: a column with
// S1 <= 2e-14 S0 supplies no left vector (it is rounding noise, or 0 / 0).  2e-14 S0 covers every column the null-column rule of
// i_jacobi may have left unrotated (norm <= 1e-14 ||A||_F <= 1.74e-14 S0); dropping it moves U diag(S) V^T by at most 2e-14 S0.
// u1 is then u0's complement along the coordinate axis least aligned with u0 (first on ties), normalised; S0 == 0 gives U = I.
// S and the directions of V are never touched by this rule, and nothing changes where S1 > 2e-14 S0.
__device__ inline void i_svd3(const double* A, double* U, double* S, double* V) {
  double B[3][3], W[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) B[i][j] = A[3 * i + j];
  i_jacobi<3, 3>(B, W);
  double nrm[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) s += B[i][j] * B[i][j];
    nrm[j] = sqrt(s);
  }
  int o0 = 0, o1 = 1, o2 = 2, tmp;
  const double n0 = nrm[0], n1 = nrm[1], n2 = nrm[2];
  auto nv = [&](int o) { return o == 0 ? n0 : o == 1 ? n1 : n2; };
  if (nv(o1) > nv(o0)) { tmp = o0; o0 = o1; o1 = tmp; }
  if (nv(o2) > nv(o1)) { tmp = o1; o1 = o2; o2 = tmp; }
  if (nv(o1) > nv(o0)) { tmp = o0; o0 = o1; o1 = tmp; }
  S[0] = nv(o0); S[1] = nv(o1); S[2] = nv(o2);
  double u0[3], u1[3], u2[3], b2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { u0[i] = i_sel3(B, i, o0) / S[0]; u1[i] = i_sel3(B, i, o1) / S[1]; b2[i] = i_sel3(B, i, o2); }
  if (!(S[1] > 2e-14 * S[0])) {                                  // rank <= 1 to working precision (the comment above)
    if (!(S[0] > 0.0)) { u0[0] = 1.0; u0[1] = 0.0; u0[2] = 0.0; }
    const double a0 = fabs(u0[0]), a1 = fabs(u0[1]), a2 = fabs(u0[2]);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const double uk = k == 0 ? u0[0] : k == 1 ? u0[1] : u0[2];
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; i++) w[i] = (i == k ? 1.0 : 0.0) - uk * u0[i];
    const double wn = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) u1[i] = w[i] / wn;
  }
  u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  // b2 . u2 == 0 exactly (a zero third column: exactly planar points) leaves the sign free: V is then made proper like U (W is a product of
  // rotations, so det V is the parity of the sort), and U V^T is a rotation whatever order the columns came out in
  const double d2 = (b2[0] * u2[0] + b2[1] * u2[1]) + b2[2] * u2[2];
  const double sg = d2 < 0 ? -1.0 : d2 > 0 ? 1.0 : ((o1 - o0 + 3) % 3 == 1 ? 1.0 : -1.0);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    U[3 * i] = u0[i]; U[3 * i + 1] = u1[i]; U[3 * i + 2] = u2[i];
    V[3 * i] = i_sel3(W, i, o0); V[3 * i + 1] = i_sel3(W, i, o1); V[3 * i + 2] = sg * i_sel3(W, i, o2);
  }
}

__device__ __forceinline__ int i_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---- run-time shapes behind a strided view: element k of a matrix lives at p[k * stride].  stride = the lanes of a workgroup
// that keep one matrix each side by side in LDS (element-major: the lanes of a wave touch consecutive words), 1 = a plain array.
struct DView {
  double* p; int stride;
  __device__ __forceinline__ double& operator[](int k) const { return p[(size_t)k * stride]; }
};

// i_jacobi for an m x n matrix U (row-major, ld = n) and V (n x n) behind views: the same sweep / pair / row order, the same
// stopping and null-column rules, so tests/npinit.py's jacobi() restates it for every shape.
__device__ inline void d_jacobi(const DView U, int m, int n, const DView V) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  double fro = 0;
  for (int i = 0; i < m; i++)
    for (int j = 0; j < n; j++) fro += U[i * n + j] * U[i * n + j];
  const double tiny = 1e-28 * fro;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < m; i++) {
          const double up = U[i * n + p], uq = U[i * n + q];
          alpha += up * up; beta += uq * uq; gamma += up * uq;
        }
        if (gamma == 0.0 || fabs(gamma) <= 1e-15 * sqrt(alpha * beta) || alpha <= tiny || beta <= tiny) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < m; i++) {
          const double up = U[i * n + p], uq = U[i * n + q];
          U[i * n + p] = c * up - s * uq; U[i * n + q] = s * up + c * uq;
        }
        for (int i = 0; i < n; i++) {
          const double vp = V[i * n + p], vq = V[i * n + q];
          V[i * n + p] = c * vp - s * vq; V[i * n + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

// squared column norms of U (m x n), rows added in order
__device__ inline void d_col_norm2(const DView U, int m, int n, double* nrm2) {
  for (int j = 0; j < n; j++) {
    double s = 0;
    for (int i = 0; i < m; i++) s += U[i * n + j] * U[i * n + j];
    nrm2[j] = s;
  }
}

// Least squares min |A x - b| for A (m x n, m <= 6, n <= 5, row-major in `A`, destroyed) by the SVD the Jacobi yields: A V = U,
// sigma_j^2 = |U_j|^2, x = sum_j V_j (U_j . b) / sigma_j^2 over the columns with sigma_j^2 > 1e-24 max_k sigma_k^2 (a singular
// value at or below 1e-12 of the largest is treated as zero: the minimum-norm solution, the rule cvSolve(CV_SVD) follows with its
// own threshold).  Columns are taken in index order; every dot product adds its terms in row order.
__device__ inline void d_lstsq(const DView A, int m, int n, const DView V, const double* b, double* x) {
  d_jacobi(A, m, n, V);
  double nrm2[5], mx = 0;
  d_col_norm2(A, m, n, nrm2);
  for (int j = 0; j < n; j++) mx = nrm2[j] > mx ? nrm2[j] : mx;
  for (int k = 0; k < n; k++) x[k] = 0.0;
  for (int j = 0; j < n; j++) {
    if (!(nrm2[j] > 1e-24 * mx)) continue;
    double d = 0;
    for (int i = 0; i < m; i++) d += A[i * n + j] * b[i];
    const double w = d / nrm2[j];
    for (int k = 0; k < n; k++) x[k] += V[k * n + j] * w;
  }
}

}  // namespace orbhip
