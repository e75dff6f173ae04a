// Probe of csrc/sim3_math.h: every function of the header once per case, on the device (one lane per case, 64-thread blocks) and on the
// host (the __host__ half of S3_HD), for tests/test_sim3_math_reference.py and tests/test_gpu_sim3_math.py to compare with an mp reference.
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -o sim3_math_probe sim3_math_probe.hip
//   ./sim3_math_probe [--host-only] cases.bin results.bin
// cases.bin, doubles only: sections of [function id, n, n * NIN values].  results.bin, doubles only: [1 if the device half ran else 0], then
// per section [function id, n, NOUT, n * NOUT device values (absent with --host-only), n * NOUT host values].
//   id  function          in                                             out
//   0   s3_exp            tangent 7                                      qt7
//   1   s3_log            qt7                                            tangent 7
//   2   s3_plus           x 7, d 7                                       tangent 7
//   3   s3_inverse        qt7                                            qt7
//   4   s3_mul            A qt7, B qt7                                   qt7
//   5   s3_adj            qt7                                            49
//   6   s3_graph_edge     lie_j 7, lie_i 7, Sji qt7                      r 7, J_i 49
//   7   s3_term_eval      K4, S qt7, P 3, uv 2, w, huber                 r 2, J 14, rho0
//   8   s3_check_outlier  K4, S qt7, P 3, uv 2, inv_sigma, thres         flag
//   9   s3_act            qt7, p 3                                       3
//   10  s3_to_pose34      qt7                                            12
#include "../../ceres_mono_orb_slam2_amd/csrc/sim3_math.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define NFUNC 11
static const int kNin[NFUNC] = {7, 7, 14, 7, 14, 7, 21, 18, 18, 10, 7};
static const int kNout[NFUNC] = {7, 7, 7, 7, 7, 49, 56, 17, 1, 3, 12};

__host__ __device__ inline void probe_one(int f, const double* in, double* out) {
  switch (f) {
    case 0: orbhip::s3_exp(in, out); break;
    case 1: orbhip::s3_log(in, out); break;
    case 2: orbhip::s3_plus(in, in + 7, out); break;
    case 3: orbhip::s3_inverse(in, out); break;
    case 4: orbhip::s3_mul(in, in + 7, out); break;
    case 5: orbhip::s3_adj(in, out); break;
    case 6: orbhip::s3_graph_edge(in, in + 7, in + 14, out, out + 7); break;
    case 7: out[16] = orbhip::s3_term_eval(in, in + 4, in + 11, in[14], in[15], in[16], in[17], out, out + 2); break;
    case 8: out[0] = (double)orbhip::s3_check_outlier(in, in + 4, in + 11, in[14], in[15], (float)in[16], in[17]); break;
    case 9: orbhip::s3_act(in, in + 7, out); break;
    case 10: orbhip::s3_to_pose34(in, out); break;
    default: break;
  }
}

// one lane per case; the case's values go through registers / private memory, as they do in the solvers
__global__ __launch_bounds__(64) void k_probe(int f, int n, int nin, int nout, const double* in, double* out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  double a[21], o[56];
  for (int q = 0; q < nin; q++) a[q] = in[(size_t)c * nin + q];
  for (int q = 0; q < nout; q++) o[q] = 0.0;
  probe_one(f, a, o);
  for (int q = 0; q < nout; q++) out[(size_t)c * nout + q] = o[q];
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
  hipLaunchKernelGGL(k_probe, dim3((n + 63) / 64), dim3(64), 0, 0, f, n, nin, nout, din, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out, dout, sizeof(double) * (size_t)n * nout, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(din));
  HIP_OK(hipFree(dout));
  return 0;
}

int main(int argc, char** argv) {
  bool host_only = false;
  const char* paths[2] = {nullptr, nullptr};
  int np = 0;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--host-only")) host_only = true;
    else if (np < 2) paths[np++] = argv[i];
    else np = 3;
  }
  if (np != 2) { fprintf(stderr, "usage: %s [--host-only] cases.bin results.bin\n", argv[0]); return 2; }
  FILE* fi = fopen(paths[0], "rb");
  if (!fi) { fprintf(stderr, "cannot read %s\n", paths[0]); return 2; }
  std::vector<double> all;
  double buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(double), 4096, fi)) > 0) all.insert(all.end(), buf, buf + got);
  fclose(fi);
  std::vector<double> res;
  res.push_back(host_only ? 0.0 : 1.0);
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
    if (!host_only) {
      std::vector<double> dv((size_t)n * nout, 0.0);
      if (n) { const int rc = run_device(f, n, in, dv.data()); if (rc) return rc; }
      res.insert(res.end(), dv.begin(), dv.end());
    }
    std::vector<double> hv((size_t)n * nout, 0.0);
    for (int c = 0; c < n; c++) probe_one(f, in + (size_t)c * nin, hv.data() + (size_t)c * nout);
    res.insert(res.end(), hv.begin(), hv.end());
    nsec++; ncase += n;
  }
  FILE* fo = fopen(paths[1], "wb");
  if (!fo) { fprintf(stderr, "cannot write %s\n", paths[1]); return 2; }
  const size_t wrote = fwrite(res.data(), sizeof(double), res.size(), fo);
  if (fclose(fo) != 0 || wrote != res.size()) { fprintf(stderr, "short write to %s\n", paths[1]); return 2; }
  printf("sim3_math_probe: %d sections, %d cases, %s\n", nsec, ncase, host_only ? "host only" : "device and host");
  return 0;
}
