// Host baseline of tools/mappoint_time.py: the mock data model's MapPoint::ComputeDistinctiveDescriptors (tests/cpp/mock_orbslam.h,
// a restatement of src/MapPoint.cc:256-315: std::map copy, N x N distances, a sorted copy of every row) looped over a batch, and the
// normal / depth loop of :335-378 over the same arrays, at -O3.  Reads the batch tools/mappoint_time.py writes:
//   int32 npts, nobs, nkf | int32 off[npts+1] | uint8 desc[nobs][32] | uint8 good[nobs] | int32 obs_kf[nobs] | double X[npts][3] |
//   double centers[nkf][3] | int32 ref_kf[npts] | int32 level[npts] | float scale[8]
// and prints one JSON line: {"desc_ms": ..., "nd_ms": ..., "reps": ...} (medians of the repetitions).
//   g++ -O3 -std=c++17 -I tests/cpp tools/cpp/mappoint_host.cpp -o /tmp/mappoint_host && /tmp/mappoint_host batch.bin 20
#include <chrono>
#include <cstdio>
#include <memory>

#include "mock_orbslam.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
using namespace mock;

template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 10;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[3]; rd(f, h, 3);
  const int npts = h[0], nobs = h[1], nkf = h[2];
  std::vector<int32_t> off(npts + 1), okf(nobs), ref(npts), lvl(npts); std::vector<uint8_t> desc(32 * (size_t)nobs), good(nobs);
  std::vector<double> X(3 * (size_t)npts), C(3 * (size_t)nkf); std::vector<float> sf(8);
  rd(f, off.data(), off.size()); rd(f, desc.data(), desc.size()); rd(f, good.data(), good.size()); rd(f, okf.data(), okf.size());
  rd(f, X.data(), X.size()); rd(f, C.data(), C.size()); rd(f, ref.data(), ref.size()); rd(f, lvl.data(), lvl.size()); rd(f, sf.data(), 8);
  std::fclose(f);
  // one mock keyframe per observation (a point's std::map needs distinct keyframes), one row each
  std::vector<std::unique_ptr<KeyFrame> > kfs(nobs);
  for (int e = 0; e < nobs; e++) {
    kfs[e].reset(new KeyFrame); kfs[e]->descriptors_ = Mat(1); std::memcpy(kfs[e]->descriptors_.ptr(0), &desc[32 * (size_t)e], 32);
    kfs[e]->is_bad_ = !good[e];
  }
  std::vector<MapPoint> mps(npts);
  for (int p = 0; p < npts; p++)
    for (int e = off[p]; e < off[p + 1]; e++) mps[p].AddObservation(kfs[e].get(), 0);
  std::vector<double> td, tn;
  double sink = 0;
  for (int r = 0; r < reps; r++) {
    auto t0 = std::chrono::steady_clock::now();
    for (MapPoint& mp : mps) mp.ComputeDistinctiveDescriptors();
    auto t1 = std::chrono::steady_clock::now();
    for (int p = 0; p < npts; p++) {
      if (off[p] == off[p + 1]) continue;
      double n[3] = {0, 0, 0};
      for (int e = off[p]; e < off[p + 1]; e++) {
        const double* O = &C[3 * (size_t)okf[e]];
        const double v[3] = {X[3 * p] - O[0], X[3 * p + 1] - O[1], X[3 * p + 2] - O[2]};
        const double nn = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        for (int k = 0; k < 3; k++) n[k] = n[k] + v[k] / nn;
      }
      const double* O = &C[3 * (size_t)ref[p]];
      const double v[3] = {X[3 * p] - O[0], X[3 * p + 1] - O[1], X[3 * p + 2] - O[2]};
      const float dist = (float)std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
      const float mx = dist * sf[lvl[p]], mn = mx / sf[7];
      sink += n[0] / (off[p + 1] - off[p]) + mn;
    }
    auto t2 = std::chrono::steady_clock::now();
    td.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); tn.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
  }
  std::sort(td.begin(), td.end()); std::sort(tn.begin(), tn.end());
  std::printf("{\"desc_ms\": %.4f, \"nd_ms\": %.4f, \"reps\": %d, \"sink\": %.3f}\n", td[td.size() / 2], tn[tn.size() / 2], reps, sink);
  return 0;
}
