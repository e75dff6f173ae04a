// What the UpdateLocalMap drop-in test needs beside mock_orbslam.h: a keyframe with the covisibility / spanning-tree accessors of
// include/KeyFrame.h (GetBestCovisibilityKeyFrames, GetChilds as a std::set<KeyFrame*>, GetParent) and track_reference_for_frame_, a map
// point with observations and track_reference_for_frame_, a frame with its slots, the types bundle FrameOpsT takes, a builder for a
// consistent map whose keyframes lie in memory in an order that is NOT their index order, and host loops of the shape of
// Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (src/Tracking.cc:847-977) over a real std::map<KeyFrame*, int> and the real
// std::set<KeyFrame*>, so that pointer order is the real thing there.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "mock_orbslam.h"

namespace mock {

struct LmKeyFrame;

struct LmMapPoint {
  std::map<LmKeyFrame*, size_t> observations_; bool is_bad_ = false;
  long unsigned int track_reference_for_frame_ = 0;
  bool isBad() { return is_bad_; }
  std::map<LmKeyFrame*, size_t> GetObservations() { return observations_; }
};

struct LmKeyFrame {
  long unsigned int id_ = 0, track_reference_for_frame_ = 0;
  bool is_bad_ = false;
  std::vector<LmMapPoint*> map_points_;
  std::vector<LmKeyFrame*> ordered_connected_keyframes_;
  std::set<LmKeyFrame*> childrens_;
  LmKeyFrame* parent_ = nullptr;
  bool isBad() { return is_bad_; }
  std::vector<LmMapPoint*> GetMapPointMatches() { return map_points_; }
  std::vector<LmKeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    if ((int)ordered_connected_keyframes_.size() < N) return ordered_connected_keyframes_;
    return std::vector<LmKeyFrame*>(ordered_connected_keyframes_.begin(), ordered_connected_keyframes_.begin() + N);
  }
  std::set<LmKeyFrame*> GetChilds() { return childrens_; }
  LmKeyFrame* GetParent() { return parent_; }
};

struct LmFrame {
  long unsigned int id_ = 0;
  int N_ = 0;
  std::vector<LmMapPoint*> map_points_;
  LmKeyFrame* reference_keyframe_ = nullptr;
};

struct LmTypes {
  typedef LmFrame Frame; typedef LmKeyFrame KeyFrame; typedef LmMapPoint MapPoint;
  typedef mock::Matrix3d Matrix3d; typedef mock::Vector3d Vector3d;
};

// What the host loops report about the paths they took
struct LmPaths { int no_votes = 0, over80 = 0, parent_break = 0; };

// The host loop in the reference's shape: votes into a std::map keyed by pointer, the voted keyframes in the map's order, then ONE
// pass over the voted keyframes (the end of the pass is fixed before anything is appended) that stops once the list is longer than 80.
inline void UpdateLocalKeyFramesHost(LmFrame& F, std::vector<LmKeyFrame*>& local, LmKeyFrame*& reference, LmPaths* paths) {
  std::map<LmKeyFrame*, int> counter;
  for (int i = 0; i < F.N_; i++) {
    LmMapPoint* mp = F.map_points_[i];
    if (!mp) continue;
    if (mp->isBad()) { F.map_points_[i] = nullptr; continue; }
    const std::map<LmKeyFrame*, size_t> obs = mp->GetObservations();
    for (const auto& o : obs) counter[o.first]++;
  }
  if (counter.empty()) { paths->no_votes++; return; }
  int best = 0;
  LmKeyFrame* best_kf = nullptr;
  local.clear();
  for (const auto& c : counter) {
    if (c.first->isBad()) continue;
    if (c.second > best) { best = c.second; best_kf = c.first; }
    local.push_back(c.first);
    c.first->track_reference_for_frame_ = F.id_;
  }
  const size_t n_voted = local.size();
  for (size_t i = 0; i < n_voted; i++) {
    if (local.size() > 80) { paths->over80++; break; }
    LmKeyFrame* kf = local[i];
    for (LmKeyFrame* nb : kf->GetBestCovisibilityKeyFrames(10))
      if (!nb->isBad() && nb->track_reference_for_frame_ != F.id_) { local.push_back(nb); nb->track_reference_for_frame_ = F.id_; break; }
    const std::set<LmKeyFrame*> children = kf->GetChilds();
    for (LmKeyFrame* ch : children)
      if (!ch->isBad() && ch->track_reference_for_frame_ != F.id_) { local.push_back(ch); ch->track_reference_for_frame_ = F.id_; break; }
    LmKeyFrame* parent = kf->GetParent();
    if (parent && parent->track_reference_for_frame_ != F.id_) { local.push_back(parent); parent->track_reference_for_frame_ = F.id_; paths->parent_break++; break; }
  }
  if (best_kf) { reference = best_kf; F.reference_keyframe_ = reference; }
}

inline void UpdateLocalPointsHost(LmFrame& F, const std::vector<LmKeyFrame*>& local, std::vector<LmMapPoint*>& points) {
  points.clear();
  for (LmKeyFrame* kf : local) {
    const std::vector<LmMapPoint*> mps = kf->GetMapPointMatches();
    for (LmMapPoint* mp : mps) {
      if (!mp || mp->track_reference_for_frame_ == F.id_ || mp->isBad()) continue;
      points.push_back(mp);
      mp->track_reference_for_frame_ = F.id_;
    }
  }
}

// A consistent map.  The keyframes live in `store` at shuffled places, so kf(i) < kf(j) says nothing about i < j: pointer order and
// index order differ.  Point p is seen from keyframes around a centre; the best covisibles are the keyframes sharing most points.
struct LmScene {
  std::vector<LmKeyFrame> store; std::vector<int> place; std::vector<LmMapPoint> mps;
  LmKeyFrame* kf(int i) { return &store[place[i]]; }
};
inline void build_lm_scene(LmScene& S, unsigned seed, int n_kf, int n_mp, int span, double q, double p_bad_kf, double p_bad_mp) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> U(0, 1);
  S.store.assign(n_kf, LmKeyFrame()); S.mps.assign(n_mp, LmMapPoint()); S.place.resize(n_kf);
  for (int k = 0; k < n_kf; k++) S.place[k] = k;
  std::shuffle(S.place.begin(), S.place.end(), rng);
  for (int k = 0; k < n_kf; k++) { S.kf(k)->id_ = (unsigned long)k; S.kf(k)->is_bad_ = k > 0 && U(rng) < p_bad_kf; }
  std::vector<std::vector<int> > share(n_kf, std::vector<int>(n_kf, 0));
  for (int p = 0; p < n_mp; p++) {
    const int c = (int)(rng() % n_kf), w = 1 + (int)(rng() % span);
    std::vector<int> seen_by;
    for (int k = std::max(0, c - w); k < std::min(n_kf, c + w + 1); k++) {
      if (U(rng) >= q) continue;
      LmKeyFrame* kf = S.kf(k);
      if (rng() % 5 == 0) kf->map_points_.push_back(nullptr);                  // (a keypoint without a point)
      kf->map_points_.push_back(&S.mps[p]);
      S.mps[p].observations_[kf] = kf->map_points_.size() - 1;
      seen_by.push_back(k);
    }
    for (int a : seen_by) for (int b : seen_by) if (a != b) share[a][b]++;
    S.mps[p].is_bad_ = U(rng) < p_bad_mp;
  }
  for (int k = 0; k < n_kf; k++) {
    std::vector<int> order;
    for (int j = 0; j < n_kf; j++) if (share[k][j] > 0) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return share[k][a] > share[k][b]; });
    for (int j : order) S.kf(k)->ordered_connected_keyframes_.push_back(S.kf(j));
    if (k > 0) { LmKeyFrame* par = S.kf(std::max(0, k - 1 - (int)(rng() % 3))); S.kf(k)->parent_ = par; par->childrens_.insert(S.kf(k)); }
  }
}

// The frame looks at the map around keyframe `centre`: each of its n slots holds, with probability `hold`, a point some keyframe within
// `window` of the centre sees (bad points included: they are to be cleared).
inline void build_lm_frame(LmScene& S, LmFrame& F, unsigned seed, int n, int centre, int window, double hold) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> U(0, 1);
  std::vector<LmMapPoint*> near;
  for (LmMapPoint& mp : S.mps)
    for (const auto& o : mp.observations_) if (std::abs((int)o.first->id_ - centre) <= window) { near.push_back(&mp); break; }
  F.N_ = n; F.map_points_.assign(n, nullptr); F.reference_keyframe_ = nullptr;
  for (int i = 0; i < n; i++) if (!near.empty() && U(rng) < hold) F.map_points_[i] = near[rng() % near.size()];
}

}  // namespace mock
