// Host baseline of tools/kfculling_time.py: LocalMapping::KeyFrameCulling as a host loop of the reference's shape (the mock data
// model's KeyFrameCullingHost, tests/cpp/mock_culling.h: per candidate, per slot, a fresh copy of the point's std::map of
// observations) on a map rebuilt from the flattened problem file.  Only the loop is timed; the map is rebuilt before every repeat.
//   kfculling_host <problem.bin> <reps>   ->   {"host_ms": median, "flagged": n}
// file: int32 {ncand, nslots, nkf, npts, nobs}, cand_kf, cand_flags (int32), slot_off, slot_pt, slot_level, obs_off, obs_kf, obs_level
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "mock_culling.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
using namespace mock;

static std::vector<int32_t> rd(FILE* f, size_t n) { std::vector<int32_t> v(n); if (n && std::fread(v.data(), 4, n, f) != n) { std::fprintf(stderr, "short file\n"); std::exit(2); } return v; }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = rd(f, 5);
  const int ncand = h[0], nslots = h[1], nkf = h[2], npts = h[3], nobs = h[4], reps = std::atoi(argv[2]);
  const std::vector<int32_t> cand_kf = rd(f, ncand), cand_flags = rd(f, ncand), slot_off = rd(f, ncand + 1), slot_pt = rd(f, nslots), slot_level = rd(f, nslots),
                             obs_off = rd(f, npts + 1), obs_kf = rd(f, nobs), obs_level = rd(f, nobs);
  std::fclose(f);
  std::vector<double> ms;
  int flagged = 0;
  for (int r = 0; r < reps; r++) {
    // keyframe nkf is the current one; a keyframe's keypoints are its observations in point order (candidates: in slot order)
    CullScene S; S.kfs.assign(nkf + 1, CullKeyFrame()); S.mps.assign(npts, CullMapPoint());
    std::vector<char> is_cand(nkf, 0);
    for (int k = 0; k <= nkf; k++) S.kfs[k].id_ = (unsigned long)(k + 1);
    for (int c = 0; c < ncand; c++) {
      CullKeyFrame& kf = S.kfs[cand_kf[c]];
      is_cand[cand_kf[c]] = 1;
      if (cand_flags[c] & 1) kf.id_ = 0;
      kf.do_not_erase_ = (cand_flags[c] & 2) != 0;
      for (int s = slot_off[c]; s < slot_off[c + 1]; s++) {
        KeyPoint kp; kp.octave = slot_level[s];
        kf.undistort_keypoints_.push_back(kp); kf.map_points_.push_back(&S.mps[slot_pt[s]]);
        S.mps[slot_pt[s]].AddObservation(&kf, kf.map_points_.size() - 1);
      }
      S.kfs[nkf].ordered_connected_keyframes_.push_back(&kf);
    }
    for (int p = 0; p < npts; p++)
      for (int e = obs_off[p]; e < obs_off[p + 1]; e++) {
        if (is_cand[obs_kf[e]]) continue;
        CullKeyFrame& kf = S.kfs[obs_kf[e]];
        KeyPoint kp; kp.octave = obs_level[e];
        kf.undistort_keypoints_.push_back(kp); kf.map_points_.push_back(&S.mps[p]);
        S.mps[p].AddObservation(&kf, kf.map_points_.size() - 1);
      }
    const auto t0 = std::chrono::steady_clock::now();
    flagged = KeyFrameCullingHost(&S.kfs[nkf]);
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"host_ms\": %.4f, \"flagged\": %d}\n", ms[ms.size() / 2], flagged);
  return 0;
}
