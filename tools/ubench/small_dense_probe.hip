// Probe of csrc/small_dense.h and of null_vector4_dev (csrc/tri_math.h): every instantiation the estimators use, once per case on the
// device, for tests/test_gpu_small_dense.py to compare with the mp reference tests/npdense.py on the case table of tests/densecases.py.
// The two headers are __device__-only, so there is no host half: the numpy restatements (tests/npinit.py, nppnp.py, npsim3solver.py) play
// that part.  One lane per case in 64-thread blocks; a case's values go through registers / private memory, as they do in the estimators.
// Function 6 is the exception: 16-thread blocks with the 16 lanes' matrices side by side in LDS behind DView{p + lane, 16}, as k_pnp_hyp
// (orb_pnp.inc) lays them out.
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -o small_dense_probe small_dense_probe.hip
//   ./small_dense_probe cases.bin results.bin
// cases.bin, doubles only: sections of [function id, n, n * NIN values].  results.bin, doubles only: per section [function id, n, NOUT,
// n * NOUT values].
//   id  function                               in                         out
//   0   i_svd3                                 A 9                        U 9, S 3, V 9
//   1   i_inv3, i_det3                         A 9                        inverse 9, det
//   2   i_jacobi<16, 9>, i_min_col             A 144                      U 144, V 81, column
//   3   i_jacobi<8, 9>, i_min_col              A 72                       U 72, V 81, column
//   4   null_vector4_dev                       A 16                       x 4
//   5   d_jacobi 12 x 12, DView{p, 1}          A 144                      U 144, V 144
//   6   d_jacobi 12 x 12, DView{p + lane, 16}  A 144                      U 144, V 144
//   7   d_lstsq 6 x 3                          A 18, b 6                  x 3
//   8   d_lstsq 6 x 4                          A 24, b 6                  x 4
//   9   d_lstsq 6 x 5                          A 30, b 6                  x 5
//   10  i_jacobi_sym4                          A 16                       diagonal 4, V 16
#include "../../ceres_mono_orb_slam2_amd/csrc/small_dense.h"
#include "../../ceres_mono_orb_slam2_amd/csrc/tri_math.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace orbhip;

#define NFUNC 11
#define STRIDED_LANES 16
static const int kNin[NFUNC] = {9, 9, 144, 72, 16, 144, 144, 24, 30, 36, 16};
static const int kNout[NFUNC] = {21, 10, 226, 154, 4, 288, 288, 3, 4, 5, 20};

template <int M>
__device__ inline void probe_jacobi9(const double* __restrict__ in, double* __restrict__ out) {
  double U[M][9], V[9][9];
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int j = 0; j < 9; j++) U[i][j] = in[9 * i + j];
  i_jacobi<M, 9>(U, V);
  const int c = i_min_col<M, 9>(U);
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int j = 0; j < 9; j++) out[9 * i + j] = U[i][j];
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j < 9; j++) out[9 * M + 9 * i + j] = V[i][j];
  out[9 * M + 81] = (double)c;
}

__device__ inline void probe_lstsq(int n, const double* __restrict__ in, double* __restrict__ out) {
  double A[30], V[25], b[6], x[5];
  for (int k = 0; k < 6 * n; k++) A[k] = in[k];
  for (int k = 0; k < 6; k++) b[k] = in[6 * n + k];
  d_lstsq(DView{A, 1}, 6, n, DView{V, 1}, b, x);
  for (int k = 0; k < n; k++) out[k] = x[k];
}

// one lane per case
__global__ __launch_bounds__(64) void k_probe(int f, int n, int nin, int nout, const double* __restrict__ in, double* __restrict__ out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  const double* a = in + (size_t)c * nin;
  double* o = out + (size_t)c * nout;
  switch (f) {
    case 0: {
      double A[9], U[9], S[3], V[9];
      for (int k = 0; k < 9; k++) A[k] = a[k];
      i_svd3(A, U, S, V);
      for (int k = 0; k < 9; k++) { o[k] = U[k]; o[12 + k] = V[k]; }
      for (int k = 0; k < 3; k++) o[9 + k] = S[k];
    } break;
    case 1: {
      double A[9], R[9];
      for (int k = 0; k < 9; k++) A[k] = a[k];
      i_inv3(A, R);
      for (int k = 0; k < 9; k++) o[k] = R[k];
      o[9] = i_det3(A);
    } break;
    case 2: probe_jacobi9<16>(a, o); break;
    case 3: probe_jacobi9<8>(a, o); break;
    case 4: {
      double A[16], x[4];
      for (int k = 0; k < 16; k++) A[k] = a[k];
      null_vector4_dev(A, x);
      for (int k = 0; k < 4; k++) o[k] = x[k];
    } break;
    case 5: {
      double A[144], V[144];
      for (int k = 0; k < 144; k++) A[k] = a[k];
      d_jacobi(DView{A, 1}, 12, 12, DView{V, 1});
      for (int k = 0; k < 144; k++) { o[k] = A[k]; o[144 + k] = V[k]; }
    } break;
    case 7: probe_lstsq(3, a, o); break;
    case 8: probe_lstsq(4, a, o); break;
    case 9: probe_lstsq(5, a, o); break;
    case 10: {
      double A[4][4], V[4][4];
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) A[i][j] = a[4 * i + j];
      i_jacobi_sym4(A, V);
      for (int i = 0; i < 4; i++) {
        o[i] = A[i][i];
        for (int j = 0; j < 4; j++) o[4 + 4 * i + j] = V[i][j];
      }
    } break;
    default: break;
  }
}

// k_pnp_hyp's layout: 16 lanes a workgroup, element k of lane l's matrix at s[k * 16 + l]
__global__ __launch_bounds__(STRIDED_LANES) void k_probe_strided(int n, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double sA[144 * STRIDED_LANES], sV[144 * STRIDED_LANES];
  const int lane = threadIdx.x, c = blockIdx.x * STRIDED_LANES + lane;
  if (c >= n) return;                                            // no barrier below: a lane works on its own words only
  const DView A = {sA + lane, STRIDED_LANES}, V = {sV + lane, STRIDED_LANES};
  for (int k = 0; k < 144; k++) A[k] = in[(size_t)c * 144 + k];
  d_jacobi(A, 12, 12, V);
  for (int k = 0; k < 144; k++) { out[(size_t)c * 288 + k] = A[k]; out[(size_t)c * 288 + 144 + k] = V[k]; }
}

#define HIP_OK(call)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (call);                                                                                  \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; }           \
  } while (0)

static int run_device(int f, int n, const double* in, double* out) {
  const int nin = kNin[f], nout = kNout[f];
  double *din = nullptr, *dout = nullptr;
  HIP_OK(hipMalloc(&din, sizeof(double) * (size_t)n * nin));
  HIP_OK(hipMalloc(&dout, sizeof(double) * (size_t)n * nout));
  HIP_OK(hipMemcpy(din, in, sizeof(double) * (size_t)n * nin, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dout, 0, sizeof(double) * (size_t)n * nout));
  if (f == 6) hipLaunchKernelGGL(k_probe_strided, dim3((n + STRIDED_LANES - 1) / STRIDED_LANES), dim3(STRIDED_LANES), 0, 0, n, din, dout);
  else hipLaunchKernelGGL(k_probe, dim3((n + 63) / 64), dim3(64), 0, 0, f, n, nin, nout, din, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out, dout, sizeof(double) * (size_t)n * nout, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(din));
  HIP_OK(hipFree(dout));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::vector<double> all;
  double buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(double), 4096, fi)) > 0) all.insert(all.end(), buf, buf + got);
  fclose(fi);
  std::vector<double> res;
  size_t pos = 0;
  int nsec = 0, ncase = 0;
  while (pos < all.size()) {
    if (pos + 2 > all.size()) { fprintf(stderr, "truncated section header at %zu\n", pos); return 2; }
    const double fd = all[pos], nd = all[pos + 1];
    if (!(fd >= 0 && fd < NFUNC && fd == (int)fd) || !(nd >= 0 && nd <= 1e6 && nd == (int)nd)) { fprintf(stderr, "bad section header at %zu\n", pos); return 2; }
    const int f = (int)fd, n = (int)nd, nin = kNin[f], nout = kNout[f];
    pos += 2;
    if (pos + (size_t)n * nin > all.size()) { fprintf(stderr, "truncated section %d\n", nsec); return 2; }
    const double* in = all.data() + pos;
    pos += (size_t)n * nin;
    res.push_back(f); res.push_back(n); res.push_back(nout);
    std::vector<double> dv((size_t)n * nout, 0.0);
    if (n) { const int rc = run_device(f, n, in, dv.data()); if (rc) return rc; }
    res.insert(res.end(), dv.begin(), dv.end());
    nsec++; ncase += n;
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  const size_t wrote = fwrite(res.data(), sizeof(double), res.size(), fo);
  if (fclose(fo) != 0 || wrote != res.size()) { fprintf(stderr, "short write to %s\n", argv[2]); return 2; }
  printf("small_dense_probe: %d sections, %d cases\n", nsec, ncase);
  return 0;
}
