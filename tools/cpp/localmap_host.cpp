// Host baseline of tools/local_map_time.py: Tracking::UpdateLocalMap as host loops of the reference's shape (the mock data model's
// UpdateLocalKeyFramesHost / UpdateLocalPointsHost, tests/cpp/mock_localmap.h: a std::map<KeyFrame*, int> of votes, a copy of every local
// keyframe's slot table) on a map rebuilt from the flattened problem file, followed by the packing of the block orbt_track_local_map takes
// (position, normal, distances, descriptor, state per local point; position and state per frame slot).  The keyframes lie in memory in
// index order, so the result equals the library's with kf_rank = NULL.  Loops and packing are timed; the marks are reset between repeats.
//   localmap_host <problem.bin> <reps>   ->   {"host_ms": median, "loops_ms": median, "n_local_kf": n, "n_local_pt": n}
// file: int32 {n_kp, npts, nkf, nobs, ncov, nchild, nslots}, frame_pt, pt_bad, pt_nobs, obs_off, obs_kf, kf_bad, kf_parent, cov_off, cov_kf,
//       child_off, child_kf, kf_slot_off, kf_slot_pt (all int32)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mock_localmap.h"

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
  const std::vector<int32_t> h = rd(f, 7);
  const int n_kp = h[0], npts = h[1], nkf = h[2], nobs = h[3], ncov = h[4], nchild = h[5], nslots = h[6], reps = std::atoi(argv[2]);
  const std::vector<int32_t> frame_pt = rd(f, n_kp), pt_bad = rd(f, npts), pt_nobs = rd(f, npts), obs_off = rd(f, npts + 1), obs_kf = rd(f, nobs), kf_bad = rd(f, nkf),
                             kf_parent = rd(f, nkf), cov_off = rd(f, nkf + 1), cov_kf = rd(f, ncov), child_off = rd(f, nkf + 1), child_kf = rd(f, nchild),
                             slot_off = rd(f, nkf + 1), slot_pt = rd(f, nslots);
  std::fclose(f);
  std::vector<LmKeyFrame> kfs(nkf); std::vector<LmMapPoint> mps(npts);
  for (int k = 0; k < nkf; k++) {
    LmKeyFrame& kf = kfs[k];
    kf.id_ = (unsigned long)k; kf.is_bad_ = kf_bad[k] != 0; kf.parent_ = kf_parent[k] >= 0 ? &kfs[kf_parent[k]] : nullptr;
    for (int e = cov_off[k]; e < cov_off[k + 1]; e++) kf.ordered_connected_keyframes_.push_back(&kfs[cov_kf[e]]);
    for (int e = child_off[k]; e < child_off[k + 1]; e++) kf.childrens_.insert(&kfs[child_kf[e]]);
    for (int s = slot_off[k]; s < slot_off[k + 1]; s++) kf.map_points_.push_back(slot_pt[s] >= 0 ? &mps[slot_pt[s]] : nullptr);
  }
  for (int p = 0; p < npts; p++) {
    mps[p].is_bad_ = pt_bad[p] != 0;
    for (int e = obs_off[p]; e < obs_off[p + 1]; e++) mps[p].observations_[&kfs[obs_kf[e]]] = 0;
  }
  // the point records the packing reads (their values do not matter to the time)
  std::vector<double> Xw(3 * (size_t)npts, 1.0), normal(3 * (size_t)npts, 0.5);
  std::vector<float> mind(npts, 1.f), maxd(npts, 9.f);
  std::vector<uint8_t> desc(32 * (size_t)npts, 7);
  std::vector<double> ms, ms_loops;
  size_t n_local_kf = 0, n_local_pt = 0;
  for (int r = 0; r < reps; r++) {
    for (LmKeyFrame& k : kfs) k.track_reference_for_frame_ = 0;
    for (LmMapPoint& p : mps) p.track_reference_for_frame_ = 0;
    LmFrame F; F.id_ = 5; F.N_ = n_kp; F.map_points_.assign(n_kp, nullptr);
    for (int i = 0; i < n_kp; i++) if (frame_pt[i] >= 0) F.map_points_[i] = &mps[frame_pt[i]];
    std::vector<LmKeyFrame*> local; std::vector<LmMapPoint*> points; LmKeyFrame* reference = nullptr; LmPaths paths;
    const auto t0 = std::chrono::steady_clock::now();
    UpdateLocalKeyFramesHost(F, local, reference, &paths);
    UpdateLocalPointsHost(F, local, points);
    const auto t1 = std::chrono::steady_clock::now();
    const size_t n = points.size();
    std::vector<double> mp_X(3 * n), mp_N(3 * n), slot_X(3 * (size_t)n_kp, 0.0);
    std::vector<float> mp_min(n), mp_max(n);
    std::vector<uint8_t> mp_desc(32 * n), mp_state(n), slot_state(n_kp, 0), seen(npts, 0);
    for (int i = 0; i < n_kp; i++) {
      LmMapPoint* mp = F.map_points_[i];
      if (!mp) continue;
      const size_t p = (size_t)(mp - mps.data());
      seen[p] = 1; slot_state[i] = pt_nobs[p] > 0 ? 1 : 3;
      std::memcpy(&slot_X[3 * (size_t)i], &Xw[3 * p], 24);
    }
    for (size_t j = 0; j < n; j++) {
      const size_t p = (size_t)(points[j] - mps.data());
      std::memcpy(&mp_X[3 * j], &Xw[3 * p], 24); std::memcpy(&mp_N[3 * j], &normal[3 * p], 24);
      mp_min[j] = mind[p]; mp_max[j] = maxd[p];
      std::memcpy(&mp_desc[32 * j], &desc[32 * p], 32);
      mp_state[j] = seen[p] ? 0 : (pt_nobs[p] > 0 ? 1 : 3);
    }
    const auto t2 = std::chrono::steady_clock::now();
    ms.push_back(std::chrono::duration<double, std::milli>(t2 - t0).count());
    ms_loops.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    n_local_kf = local.size(); n_local_pt = n;
    if (mp_state.size() + slot_state.size() == (size_t)-1) std::printf("%d", (int)mp_desc[0]);      // (keeps the packing alive)
  }
  std::sort(ms.begin(), ms.end()); std::sort(ms_loops.begin(), ms_loops.end());
  std::printf("{\"host_ms\": %.4f, \"loops_ms\": %.4f, \"n_local_kf\": %zu, \"n_local_pt\": %zu}\n", ms[ms.size() / 2], ms_loops[ms_loops.size() / 2], n_local_kf, n_local_pt);
  return 0;
}
