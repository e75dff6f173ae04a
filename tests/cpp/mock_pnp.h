// What the PnPsolver drop-in tests need beside mock_orbslam.h: a stand-in for DUtils::Random that can be re-seeded (so that a
// second pass draws the same sequence) and the reader of the scene file tests/test_gpu_pnp_dropin.py writes.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mock_orbslam.h"

// DUtils::Random's RandomInt over a fixed 64-bit LCG, inclusive on both ends
struct ScriptedRandom {
  static uint64_t state;
  static void Reset(uint64_t seed) { state = seed * 2654435761u + 12345u; }
  static int RandomInt(int min, int max) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return min + (int)((state >> 33) % (uint64_t)(max - min + 1));
  }
};

// scene file: int32 n_slots; float K4[4]; per slot: int32 flag (0 = no map point, 1 = good, 2 = bad), float x, y, int32 octave,
// double X[3]
struct PnpScene {
  mock::Frame frame;
  std::vector<mock::MapPoint> points;
  std::vector<mock::MapPoint*> matches;
  bool read(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t n; float K4[4];
    if (std::fread(&n, 4, 1, f) != 1 || std::fread(K4, 4, 4, f) != 4) { std::fclose(f); return false; }
    mock::Frame::fx_ = K4[0]; mock::Frame::fy_ = K4[1]; mock::Frame::cx_ = K4[2]; mock::Frame::cy_ = K4[3];
    frame.N_ = n; frame.undistort_keypoints_.resize(n); frame.map_points_.assign(n, nullptr);
    frame.scale_factors_.assign(8, 1.0f); frame.level_sigma2s_.assign(8, 1.0f);
    for (int i = 1; i < 8; i++) { frame.scale_factors_[i] = frame.scale_factors_[i - 1] * 1.2f; frame.level_sigma2s_[i] = frame.scale_factors_[i] * frame.scale_factors_[i]; }
    points.resize(n); matches.assign(n, nullptr);
    for (int i = 0; i < n; i++) {
      int32_t flag, octave; float xy[2]; double X[3];
      if (std::fread(&flag, 4, 1, f) != 1 || std::fread(xy, 4, 2, f) != 2 || std::fread(&octave, 4, 1, f) != 1 || std::fread(X, 8, 3, f) != 3) { std::fclose(f); return false; }
      frame.undistort_keypoints_[i].pt.x = xy[0]; frame.undistort_keypoints_[i].pt.y = xy[1]; frame.undistort_keypoints_[i].octave = octave;
      points[i].SetWorldPos(mock::Vector3d(X[0], X[1], X[2]));
      points[i].is_bad_ = flag == 2;
      matches[i] = flag ? &points[i] : nullptr;
    }
    std::fclose(f);
    return true;
  }
};
