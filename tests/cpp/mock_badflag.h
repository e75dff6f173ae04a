// What the SetBadFlags drop-in test needs beside mock_orbslam.h: a keyframe with the covisibility, spanning-tree and erase members of
// include/KeyFrame.h as real containers and a SetBadFlag / EraseConnection / UpdateBestCovisibles / ChangeParent of the reference's
// shape (src/KeyFrame.cc:172-193, :405-414, :460-573) written for this mock, a map point with EraseObservation / SetBadFlag
// (src/MapPoint.cc:140-191), a map and a keyframe database that record what was erased from them, the types bundle FrameOpsT takes,
// and a builder whose keyframes lie in memory in an order that is NOT their index order.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <cmath>
#include <list>
#include <map>
#include <mutex>
#include <random>
#include <set>
#include <vector>

#include "mock_orbslam.h"

namespace ORB_SLAM2 { template <class> struct FrameOpsT; }

namespace mock {

struct BfKeyFrame;
struct BfMapPoint;

struct BfMap {
  std::set<BfKeyFrame*> erased_keyframes; std::set<BfMapPoint*> erased_points;
  void EraseKeyFrame(BfKeyFrame* kf) { erased_keyframes.insert(kf); }
  void EraseMapPoint(BfMapPoint* mp) { erased_points.insert(mp); }
};
struct BfDatabase {
  std::set<BfKeyFrame*> erased;
  void erase(BfKeyFrame* kf) { erased.insert(kf); }
};

struct BfMapPoint {
  std::map<BfKeyFrame*, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mutex_features_); return observations_; }
  int Observations() { std::unique_lock<std::mutex> lock(mutex_features_); return n_observations_; }
  bool isBad() { std::unique_lock<std::mutex> lock(mutex_features_); return is_bad_; }
  inline void EraseObservation(BfKeyFrame* keyframe);
  inline void SetBadFlag();

 protected:
  template <class> friend struct ORB_SLAM2::FrameOpsT;
  friend struct BfScene;
  friend struct BfCompare;
  std::map<BfKeyFrame*, size_t> observations_;
  int n_observations_ = 0;
  BfKeyFrame* reference_keyframe_ = nullptr;
  bool is_bad_ = false;
  BfMap* map_ = nullptr;
  std::mutex mutex_features_, mutex_pose_;
};

struct BfKeyFrame {
  unsigned long id_ = 0;
  Matrix4d GetPose() { return Tcw_; }
  Matrix4d GetPoseInverse() { return Twc_; }
  void SetPose(const Matrix4d& T) {                                 // Rwc = Rcw^T, Ow = -(Rwc tcw), each dot product (a0 b0 + a1 b1) + a2 b2
    Tcw_ = T;
    Twc_ = Matrix4d();
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Twc_(i, j) = T(j, i);
      Twc_(i, 3) = -((T(0, i) * T(0, 3) + T(1, i) * T(1, 3)) + T(2, i) * T(2, 3));
    }
  }
  std::vector<BfMapPoint*> GetMapPointMatches() { return map_points_; }
  void EraseMapPointMatch(const size_t& index) { map_points_[index] = nullptr; }
  bool isBad() { std::unique_lock<std::mutex> lock(mutex_connections_); return is_bad_; }
  std::vector<BfKeyFrame*> GetVectorCovisibleKeyFrames() { std::unique_lock<std::mutex> lock(mutex_connections_); return ordered_connected_keyframes_; }
  int GetWeight(BfKeyFrame* kf) {
    std::unique_lock<std::mutex> lock(mutex_connections_);
    auto it = connected_keyframe_weights_.find(kf);
    return it == connected_keyframe_weights_.end() ? 0 : it->second;
  }
  void AddChild(BfKeyFrame* kf) { std::unique_lock<std::mutex> lock(mutex_connections_); childrens_.insert(kf); }
  void EraseChild(BfKeyFrame* kf) { std::unique_lock<std::mutex> lock(mutex_connections_); childrens_.erase(kf); }
  void ChangeParent(BfKeyFrame* kf) { { std::unique_lock<std::mutex> lock(mutex_connections_); parent_ = kf; } kf->AddChild(this); }
  void EraseConnection(BfKeyFrame* kf) {
    bool update = false;
    {
      std::unique_lock<std::mutex> lock(mutex_connections_);
      if (connected_keyframe_weights_.count(kf)) { connected_keyframe_weights_.erase(kf); update = true; }
    }
    if (update) UpdateBestCovisibles();
  }
  void UpdateBestCovisibles() {                                     // ascending sort, then push_front: descending (weight, pointer)
    std::unique_lock<std::mutex> lock(mutex_connections_);
    std::vector<std::pair<int, BfKeyFrame*> > pairs;
    for (auto& w : connected_keyframe_weights_) pairs.push_back(std::make_pair(w.second, w.first));
    std::sort(pairs.begin(), pairs.end(), [](const std::pair<int, BfKeyFrame*>& a, const std::pair<int, BfKeyFrame*>& b) {
      return a.first != b.first ? a.first < b.first : std::less<BfKeyFrame*>()(a.second, b.second);
    });
    std::list<BfKeyFrame*> kl; std::list<int> wl;
    for (auto& p : pairs) { kl.push_front(p.second); wl.push_front(p.first); }
    ordered_connected_keyframes_.assign(kl.begin(), kl.end());
    ordered_weights_.assign(wl.begin(), wl.end());
  }
  // the whole of KeyFrame::SetBadFlag on the host: the loop the drop-in replaces
  void SetBadFlag() {
    {
      std::unique_lock<std::mutex> lock(mutex_connections_);
      if (id_ == 0) return;
      if (do_not_erase_) { do_to_be_erased_ = true; return; }
    }
    for (auto& w : connected_keyframe_weights_) w.first->EraseConnection(this);
    for (BfMapPoint* mp : map_points_) if (mp) mp->EraseObservation(this);
    {
      connected_keyframe_weights_.clear(); ordered_connected_keyframes_.clear(); ordered_weights_.clear();
      std::set<BfKeyFrame*> candidates;
      candidates.insert(parent_);
      while (!childrens_.empty()) {
        int best = -1; BfKeyFrame *child = nullptr, *parent = nullptr;
        for (BfKeyFrame* c : childrens_) {
          if (c->isBad()) continue;
          const std::vector<BfKeyFrame*> list = c->GetVectorCovisibleKeyFrames();
          for (BfKeyFrame* e : list) {
            bool is_candidate = false;
            for (BfKeyFrame* q : candidates) is_candidate |= q->id_ == e->id_;
            if (!is_candidate) continue;
            const int w = c->GetWeight(e);
            if (w > best) { best = w; child = c; parent = e; }
          }
        }
        if (!child) break;
        child->ChangeParent(parent);
        candidates.insert(child);
        childrens_.erase(child);
      }
      for (BfKeyFrame* c : childrens_) c->ChangeParent(parent_);
      parent_->EraseChild(this);
      const Matrix4d Twc = parent_->GetPoseInverse();
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) Tcp_(i, j) = ((Tcw_(i, 0) * Twc(0, j) + Tcw_(i, 1) * Twc(1, j)) + Tcw_(i, 2) * Twc(2, j)) + Tcw_(i, 3) * Twc(3, j);
      std::unique_lock<std::mutex> lock(mutex_connections_);
      is_bad_ = true;
    }
    map_->EraseKeyFrame(this);
    keyframe_database_->erase(this);
  }

 protected:
  template <class> friend struct ORB_SLAM2::FrameOpsT;              // (the line INTEGRATION.md section 4 adds to include/KeyFrame.h)
  friend struct BfScene;
  friend struct BfCompare;
  Matrix4d Tcw_, Twc_, Tcp_;
  std::vector<BfMapPoint*> map_points_;
  std::map<BfKeyFrame*, int> connected_keyframe_weights_;
  std::vector<BfKeyFrame*> ordered_connected_keyframes_;
  std::vector<int> ordered_weights_;
  BfKeyFrame* parent_ = nullptr;
  std::set<BfKeyFrame*> childrens_;
  bool do_not_erase_ = false, do_to_be_erased_ = false, is_bad_ = false;
  BfMap* map_ = nullptr;
  BfDatabase* keyframe_database_ = nullptr;
  std::mutex mutex_connections_, mutex_features_;
};

inline void BfMapPoint::EraseObservation(BfKeyFrame* keyframe) {
  bool bad = false;
  {
    std::unique_lock<std::mutex> lock(mutex_features_);
    if (observations_.count(keyframe)) {
      n_observations_--;
      observations_.erase(keyframe);
      if (reference_keyframe_ == keyframe && !observations_.empty()) reference_keyframe_ = observations_.begin()->first;
      if (n_observations_ <= 2) bad = true;
    }
  }
  if (bad) SetBadFlag();
}
inline void BfMapPoint::SetBadFlag() {
  std::map<BfKeyFrame*, size_t> observations;
  {
    std::unique_lock<std::mutex> lock1(mutex_features_);
    std::unique_lock<std::mutex> lock2(mutex_pose_);
    is_bad_ = true;
    observations.swap(observations_);
  }
  for (auto& o : observations) o.first->EraseMapPointMatch(o.second);
  map_->EraseMapPoint(this);
}

struct BfTypes {
  typedef mock::Frame Frame; typedef BfKeyFrame KeyFrame; typedef BfMapPoint MapPoint;
  typedef mock::Matrix3d Matrix3d; typedef mock::Vector3d Vector3d;
};

// n_kf keyframes along a path, keyframe index i living at store[place[i]] (a seeded shuffle), each the child of one of the six before
// it; per_kf * n_kf / 4 points each seen by 2-6 keyframes of a window, some keyframes listing a point twice; the covisibility maps
// hold the shared points / 3 (many equal weights) with one entry in ten missing on one side; two lists in three hold only the weights
// >= 2; every seventh keyframe has do_not_erase_ set.
struct BfScene {
  std::vector<BfKeyFrame> store; std::vector<BfMapPoint> mps; std::vector<int> place; BfMap map; BfDatabase db;
  BfKeyFrame& kf(int i) { return store[place[i]]; }
  int index_of(const BfKeyFrame* k) const { const int at = (int)(k - store.data()); for (size_t i = 0; i < place.size(); i++) if (place[i] == at) return (int)i; return -1; }
  void build(unsigned seed, int n_kf, int per_kf, int window) {
    std::mt19937 rng(seed);
    store = std::vector<BfKeyFrame>(n_kf); place.resize(n_kf);
    for (int i = 0; i < n_kf; i++) place[i] = i;
    std::shuffle(place.begin(), place.end(), rng);
    for (int i = 0; i < n_kf; i++) {
      BfKeyFrame& k = kf(i);
      k.id_ = (unsigned long)i; k.map_ = &map; k.keyframe_database_ = &db; k.do_not_erase_ = i % 7 == 6;
      Matrix4d T;                                                   // a rotation about z and a translation
      const double a = 0.1 * i, c = std::cos(a), s = std::sin(a);
      T(0, 0) = c; T(0, 1) = -s; T(1, 0) = s; T(1, 1) = c; T(0, 3) = 0.37 * i; T(1, 3) = -0.11 * i; T(2, 3) = 1.0 / (1 + i);
      k.SetPose(T);
      if (i > 0) { BfKeyFrame& p = kf(std::max(0, i - 1 - (int)(rng() % 6))); k.parent_ = &p; p.childrens_.insert(&k); }
    }
    const int n_mp = n_kf * per_kf / 4;
    mps = std::vector<BfMapPoint>(n_mp);
    for (int p = 0; p < n_mp; p++) {
      mps[p].map_ = &map;
      const int c = (int)(rng() % n_kf), lo = std::max(0, c - window), hi = std::min(n_kf, c + window + 1);
      std::vector<int> cand;
      for (int k = lo; k < hi; k++) cand.push_back(k);
      std::shuffle(cand.begin(), cand.end(), rng);
      const int n = std::min((int)cand.size(), 2 + (int)(rng() % 5));
      for (int j = 0; j < n; j++) {
        BfKeyFrame& k = kf(cand[j]);
        if (rng() % 6 == 0) k.map_points_.push_back(nullptr);
        k.map_points_.push_back(&mps[p]); mps[p].observations_[&k] = k.map_points_.size() - 1;
        if (rng() % 9 == 0) k.map_points_.push_back(&mps[p]);      // listed twice
      }
      mps[p].n_observations_ = n;
      auto it = mps[p].observations_.begin();
      std::advance(it, rng() % n);
      mps[p].reference_keyframe_ = it->first;
    }
    for (int i = 0; i < n_kf; i++)
      for (int j = std::max(0, i - 2 * window); j < std::min(n_kf, i + 2 * window + 1); j++) {
        if (j == i) continue;
        int shared = 0;
        for (size_t s = 0; s < kf(i).map_points_.size(); s++) {     // (a point listed twice counts through its observed slot only)
          BfMapPoint* mp = kf(i).map_points_[s];
          shared += mp && mp->observations_[&kf(i)] == s && mp->observations_.count(&kf(j));
        }
        if (shared / 3 > 0 && rng() % 10 != 0) kf(i).connected_keyframe_weights_[&kf(j)] = shared / 3;
      }
    for (int i = 0; i < n_kf; i++) {
      BfKeyFrame& k = kf(i);
      k.UpdateBestCovisibles();
      if (rng() % 3 != 0) {
        size_t keep = 0;
        while (keep < k.ordered_weights_.size() && k.ordered_weights_[keep] >= 2) keep++;
        k.ordered_connected_keyframes_.resize(keep); k.ordered_weights_.resize(keep);
      }
    }
  }
};

}  // namespace mock
