// What the KeyFrameCulling drop-in test needs beside mock_orbslam.h: a keyframe with SetBadFlag() / do_not_erase_ / do_to_be_erased_
// (include/KeyFrame.h, src/KeyFrame.cc:460-480 as far as observations go: no covisibility graph, no spanning tree), a map point whose
// EraseObservation turns it bad at <= 2 observations and whose SetBadFlag empties the observers' slots (src/MapPoint.cc:140-191,
// monocular), the types bundle FrameOpsT takes, a builder for a consistent map, and a host KeyFrameCulling of the reference's shape
// (src/LocalMapping.cc:576-637: a copy of the observations per point, the break at th_obs) to compare against and to time.
// TEST INFRASTRUCTURE.
#pragma once
#include <map>
#include <random>
#include <vector>

#include "mock_orbslam.h"

namespace mock {

struct CullKeyFrame;

struct CullMapPoint {
  std::map<CullKeyFrame*, size_t> observations_; int n_observations_ = 0; bool is_bad_ = false;
  void AddObservation(CullKeyFrame* kf, size_t idx) { if (observations_.count(kf)) return; observations_[kf] = idx; n_observations_++; }
  std::map<CullKeyFrame*, size_t> GetObservations() { return observations_; }
  int Observations() { return n_observations_; }
  bool isBad() { return is_bad_; }
  inline void EraseObservation(CullKeyFrame* kf);
  inline void SetBadFlag();
};

struct CullKeyFrame {
  unsigned long id_ = 0;
  bool do_not_erase_ = false, do_to_be_erased_ = false, is_bad_ = false;
  std::vector<KeyPoint> undistort_keypoints_;
  std::vector<CullMapPoint*> map_points_;
  std::vector<CullKeyFrame*> ordered_connected_keyframes_;
  std::vector<CullKeyFrame*> GetVectorCovisibleKeyFrames() { return ordered_connected_keyframes_; }
  std::vector<CullMapPoint*> GetMapPointMatches() { return map_points_; }
  void EraseMapPointMatch(const size_t& i) { map_points_[i] = nullptr; }
  bool isBad() { return is_bad_; }
  void SetBadFlag() {
    if (id_ == 0) return;
    if (do_not_erase_) { do_to_be_erased_ = true; return; }
    for (size_t i = 0; i < map_points_.size(); i++) if (map_points_[i]) map_points_[i]->EraseObservation(this);
    is_bad_ = true;
  }
};

inline void CullMapPoint::EraseObservation(CullKeyFrame* kf) {
  bool bad = false;
  if (observations_.count(kf)) {
    n_observations_--;
    observations_.erase(kf);
    if (n_observations_ <= 2) bad = true;
  }
  if (bad) SetBadFlag();
}
inline void CullMapPoint::SetBadFlag() {
  std::map<CullKeyFrame*, size_t> obs = observations_;
  is_bad_ = true; observations_.clear();
  for (auto& o : obs) o.first->EraseMapPointMatch(o.second);
}

struct CullTypes {
  typedef mock::Frame Frame; typedef CullKeyFrame KeyFrame; typedef CullMapPoint MapPoint;
  typedef mock::Matrix3d Matrix3d; typedef mock::Vector3d Vector3d;
};

// The loop of the reference on the host, in its shape: per candidate, per slot, a fresh copy of the point's observations.
inline int KeyFrameCullingHost(CullKeyFrame* current, int th_obs = 3) {
  int n_flagged = 0;
  std::vector<CullKeyFrame*> local = current->GetVectorCovisibleKeyFrames();
  for (CullKeyFrame* kf : local) {
    if (kf->id_ == 0) continue;
    const std::vector<CullMapPoint*> mps = kf->GetMapPointMatches();
    int redundant = 0, n_points = 0;
    for (size_t i = 0; i < mps.size(); i++) {
      CullMapPoint* mp = mps[i];
      if (!mp || mp->isBad()) continue;
      n_points++;
      if (mp->Observations() <= th_obs) continue;
      const int level = kf->undistort_keypoints_[i].octave;
      const std::map<CullKeyFrame*, size_t> obs = mp->GetObservations();
      int n = 0;
      for (const auto& o : obs) {
        if (o.first == kf) continue;
        if (o.first->undistort_keypoints_[o.second].octave <= level + 1 && ++n >= th_obs) break;
      }
      if (n >= th_obs) redundant++;
    }
    if (redundant > 0.9 * n_points) { kf->SetBadFlag(); n_flagged++; }
  }
  return n_flagged;
}

// A consistent map: n_kf keyframes (the last one is the current keyframe, every other one its covisible neighbour in a shuffled
// order), n_mp points each seen by a run of keyframes around a centre with probability q, octaves around a base per point.
struct CullScene { std::vector<CullKeyFrame> kfs; std::vector<CullMapPoint> mps; };
inline void build_cull_scene(CullScene& S, unsigned seed, int n_kf, int n_mp, int span, double q, int lvl_jit = 1) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> U(0, 1);
  S.kfs.assign(n_kf, CullKeyFrame()); S.mps.assign(n_mp, CullMapPoint());
  for (int k = 0; k < n_kf; k++) S.kfs[k].id_ = (unsigned long)k;
  for (int p = 0; p < n_mp; p++) {
    const int c = (int)(rng() % n_kf), w = 1 + (int)(rng() % span), base = (int)(rng() % 7);
    for (int k = std::max(0, c - w); k < std::min(n_kf, c + w + 1); k++) {
      if (U(rng) >= q) continue;
      KeyPoint kp; kp.octave = std::min(7, std::max(0, base + (int)(rng() % (2 * lvl_jit + 1)) - lvl_jit));
      if (rng() % 5 == 0) { S.kfs[k].undistort_keypoints_.push_back(KeyPoint()); S.kfs[k].map_points_.push_back(nullptr); }   // (a keypoint without a point)
      S.kfs[k].undistort_keypoints_.push_back(kp); S.kfs[k].map_points_.push_back(&S.mps[p]);
      S.mps[p].AddObservation(&S.kfs[k], S.kfs[k].map_points_.size() - 1);
    }
  }
  std::vector<int> order(n_kf - 1);
  for (int k = 0; k < n_kf - 1; k++) order[k] = k;
  std::shuffle(order.begin(), order.end(), rng);
  for (int k : order) S.kfs[n_kf - 1].ordered_connected_keyframes_.push_back(&S.kfs[k]);
  for (int k = 1; k < n_kf - 1; k++) if (rng() % 10 == 0) S.kfs[k].do_not_erase_ = true;
}

}  // namespace mock
