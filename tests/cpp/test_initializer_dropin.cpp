// Drop-in case of InitializerT (csrc/compat/orbslam_initializer.h; HIP library underneath) over the mock data model and a stand-in
// RNG with DUtils::Random's interface.  Reads one two-view scene (written by tests/test_gpu_initializer_dropin.py), runs the
// drop-in's Initialize, then checks (1) the sets it drew equal a plain restatement of src/Initializer.cc:88-101 on the same
// generator, and (2) its outputs are bit-identical to orbt_initialize called directly on those sets.
// Prints "OK <success> <matches> <model>" on success.
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_initializer_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_initializer.h"
#include "mock_orbslam.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock

// DUtils::Random's interface over a fixed 64-bit LCG: seeded once per process, RandomInt inclusive on both ends
struct StandInRandom {
  static uint64_t state; static bool seeded;
  static void SeedRandOnce(int seed) { if (!seeded) { state = (uint64_t)seed * 2654435761u + 12345u; seeded = true; } }
  static int RandomInt(int min, int max) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return min + (int)((state >> 33) % (uint64_t)(max - min + 1));
  }
};
uint64_t StandInRandom::state = 0;
bool StandInRandom::seeded = false;

typedef ORB_SLAM2::InitializerT<mock::Types, StandInRandom> Initializer;

static int fail(const char* what) { std::printf("FAIL %s\n", what); return 1; }

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: test_initializer_dropin scene.bin");
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open the scene");
  int32_t hdr[3]; float K4[4];
  if (std::fread(hdr, 4, 3, f) != 3 || std::fread(K4, 4, 4, f) != 4) return fail("short header");
  const int n1 = hdr[0], n2 = hdr[1], iterations = hdr[2];
  std::vector<float> k1(2 * (size_t)n1), k2(2 * (size_t)n2);
  std::vector<int> m12((size_t)n1);
  if (std::fread(k1.data(), 4, k1.size(), f) != k1.size() || std::fread(k2.data(), 4, k2.size(), f) != k2.size() ||
      std::fread(m12.data(), 4, m12.size(), f) != m12.size()) return fail("short scene");
  std::fclose(f);
  mock::Frame::fx_ = K4[0]; mock::Frame::fy_ = K4[1]; mock::Frame::cx_ = K4[2]; mock::Frame::cy_ = K4[3];
  mock::Frame F1, F2;
  F1.undistort_keypoints_.resize(n1); F2.undistort_keypoints_.resize(n2);
  for (int i = 0; i < n1; i++) { F1.undistort_keypoints_[i].pt.x = k1[2 * i]; F1.undistort_keypoints_[i].pt.y = k1[2 * i + 1]; }
  for (int i = 0; i < n2; i++) { F2.undistort_keypoints_[i].pt.x = k2[2 * i]; F2.undistort_keypoints_[i].pt.y = k2[2 * i + 1]; }

  StandInRandom::SeedRandOnce(0);                              // the process's one seeding; Initialize's own call is then a no-op
  const uint64_t s0 = StandInRandom::state;
  Initializer init(F1, 1.0, iterations);
  mock::Matrix3d R21; mock::Vector3d t21; std::vector<mock::Vector3d> vP3D; std::vector<bool> tri;
  const bool ok = init.Initialize(F2, m12, R21, t21, vP3D, tri);

  // (1) :88-101 restated on the same generator
  int N = 0;
  for (int v : m12) N += v >= 0;
  StandInRandom::state = s0;
  std::vector<int32_t> sets(8 * (size_t)iterations);
  std::vector<size_t> all;
  for (int i = 0; i < N; i++) all.push_back(i);
  for (int it = 0; it < iterations; it++) {
    std::vector<size_t> avail = all;
    for (int j = 0; j < 8; j++) {
      const int r = StandInRandom::RandomInt(0, (int)avail.size() - 1);
      sets[8 * (size_t)it + j] = (int32_t)avail[r];
      avail[r] = avail.back(); avail.pop_back();
    }
  }
  if (sets != init.ransac_sets()) return fail("drawn sets differ from the restatement of :88-101");

  // (2) the library called directly on those sets
  std::vector<int32_t> m32(m12.begin(), m12.end());
  double R[9] = {0}, t[3] = {0};
  std::vector<double> P(3 * (size_t)n1, NAN);
  std::vector<uint8_t> tr((size_t)n1, 0);
  orbt_init_report rep;
  if (orbt_initialize(k1.data(), n1, k2.data(), n2, m32.data(), K4, 1.0f, iterations, sets.data(), R, t, P.data(), tr.data(), &rep, nullptr) != 0)
    return fail(orbhip_last_error());
  if (std::memcmp(&rep, &init.last_report(), sizeof rep) != 0) return fail("report differs");
  if (ok != (rep.reason == ORBT_INIT_OK)) return fail("success differs");
  if (ok) {
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) if (std::memcmp(&R[3 * r + c], &R21(r, c), 8) != 0) return fail("R21 differs");
    for (int k = 0; k < 3; k++) if (std::memcmp(&t[k], &t21[k], 8) != 0) return fail("t21 differs");
    if ((int)vP3D.size() != n1 || (int)tri.size() != n1) return fail("output sizes");
    for (int i = 0; i < n1; i++) {
      if ((tr[i] != 0) != tri[i]) return fail("is_triangulated differs");
      if (std::isnan(P[3 * (size_t)i])) continue;
      for (int k = 0; k < 3; k++) if (std::memcmp(&P[3 * (size_t)i + k], &vP3D[i][k], 8) != 0) return fail("vP3D differs");
    }
  }
  std::printf("OK %d %d %d\n", ok ? 1 : 0, N, rep.model);
  return 0;
}
