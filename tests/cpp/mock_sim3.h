// What the Sim3Solver drop-in tests need beside mock_orbslam.h: a stand-in for DUtils::Random that can be re-seeded (so that a
// second pass draws the same sequence) and the reader of the scene file tests/test_gpu_sim3solver_dropin.py writes.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mock_orbslam.h"

// DUtils::Random's RandomInt over a fixed 64-bit LCG, inclusive on both ends
struct Sim3ScriptedRandom {
  static uint64_t state;
  static void Reset(uint64_t seed) { state = seed * 2654435761u + 12345u; }
  static int RandomInt(int min, int max) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return min + (int)((state >> 33) % (uint64_t)(max - min + 1));
  }
};

// scene file: int32 n_slots, fix_scale; float K1[4], K2[4]; double T1[12], T2[12] (Tcw, row-major 3 x 4); per slot of keyframe 1:
// int32 flag1, flag2 (0 = no map point, 1 = good, 2 = bad, 3 = good but not observed in its keyframe), int32 octave1, octave2,
// double Xw1[3], Xw2[3].  Slot i is keypoint i of both keyframes.
struct Sim3Scene {
  mock::KeyFrame kf1, kf2;
  std::vector<mock::MapPoint> points1, points2;
  std::vector<mock::MapPoint*> matches12;
  int fix_scale = 0;
  static void setup(mock::KeyFrame& kf, int n, const float* K4, const double* T) {
    kf.N_ = n; kf.undistort_keypoints_.resize(n); kf.map_points_.assign(n, nullptr);
    kf.fx_ = K4[0]; kf.fy_ = K4[1]; kf.cx_ = K4[2]; kf.cy_ = K4[3];
    kf.scale_factors_.assign(8, 1.0f); kf.level_sigma2s_.assign(8, 1.0f);
    for (int i = 1; i < 8; i++) { kf.scale_factors_[i] = kf.scale_factors_[i - 1] * 1.2f; kf.level_sigma2s_[i] = kf.scale_factors_[i] * kf.scale_factors_[i]; }
    mock::Matrix4d M;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) M(r, c) = T[4 * r + c];
    kf.SetPose(M);
  }
  bool read(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t hdr[2]; float K1[4], K2[4]; double T1[12], T2[12];
    if (std::fread(hdr, 4, 2, f) != 2 || std::fread(K1, 4, 4, f) != 4 || std::fread(K2, 4, 4, f) != 4 || std::fread(T1, 8, 12, f) != 12 ||
        std::fread(T2, 8, 12, f) != 12) { std::fclose(f); return false; }
    const int n = hdr[0];
    fix_scale = hdr[1];
    setup(kf1, n, K1, T1); setup(kf2, n, K2, T2);
    points1.resize(n); points2.resize(n); matches12.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
      int32_t q[4]; double X[6];
      if (std::fread(q, 4, 4, f) != 4 || std::fread(X, 8, 6, f) != 6) { std::fclose(f); return false; }
      kf1.undistort_keypoints_[i].octave = q[2]; kf2.undistort_keypoints_[i].octave = q[3];
      points1[i].SetWorldPos(mock::Vector3d(X[0], X[1], X[2])); points2[i].SetWorldPos(mock::Vector3d(X[3], X[4], X[5]));
      points1[i].is_bad_ = q[0] == 2; points2[i].is_bad_ = q[1] == 2;
      if (q[0] == 1 || q[0] == 2) points1[i].AddObservation(&kf1, i);
      if (q[1] == 1 || q[1] == 2) points2[i].AddObservation(&kf2, i);
      kf1.map_points_[i] = q[0] ? &points1[i] : nullptr;
      matches12[i] = q[1] ? &points2[i] : nullptr;
    }
    std::fclose(f);
    return true;
  }
};
