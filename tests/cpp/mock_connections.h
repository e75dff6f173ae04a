// What the UpdateConnections drop-in test needs beside mock_orbslam.h: a keyframe with the covisibility members of include/KeyFrame.h as
// real containers (std::map<KF*, int> connected_keyframe_weights_, the two ordered vectors, parent_ / childrens_ / is_first_connection_)
// and a host UpdateConnections / AddConnection / UpdateBestCovisibles of the reference's shape (src/KeyFrame.cc:158-193, :314-398) to
// compare against and to time, a map point with observations, the types bundle FrameOpsT takes, the loop of LoopClosing.cc:551-573 on
// the host, and a builder whose keyframes lie in memory in an order that is NOT their index order (so the pointer order the reference
// depends on differs from the index order).  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <list>
#include <map>
#include <mutex>
#include <random>
#include <set>
#include <vector>

#include "mock_orbslam.h"

namespace ORB_SLAM2 { template <class> struct FrameOpsT; }

namespace mock {

struct ConnKeyFrame;

struct ConnMapPoint {
  std::map<ConnKeyFrame*, size_t> observations_; bool is_bad_ = false;
  std::map<ConnKeyFrame*, size_t> GetObservations() { return observations_; }
  bool isBad() { return is_bad_; }
};

struct ConnKeyFrame {
  unsigned long id_ = 0;
  int n_writes_ = 0;                                              // how often the host loop below wrote this keyframe's tables (the tests count with it)
  std::vector<ConnMapPoint*> map_points_;
  std::vector<ConnMapPoint*> GetMapPointMatches() { return map_points_; }
  std::vector<ConnKeyFrame*> GetVectorCovisibleKeyFrames() { std::unique_lock<std::mutex> lock(mutex_connections_); return ordered_connected_keyframes_; }
  std::set<ConnKeyFrame*> GetConnectedKeyFrames() {
    std::unique_lock<std::mutex> lock(mutex_connections_);
    std::set<ConnKeyFrame*> s;
    for (auto& w : connected_keyframe_weights_) s.insert(w.first);
    return s;
  }
  void AddChild(ConnKeyFrame* kf) { std::unique_lock<std::mutex> lock(mutex_connections_); childrens_.insert(kf); }

  void AddConnection(ConnKeyFrame* kf, const int& weight) {
    {
      std::unique_lock<std::mutex> lock(mutex_connections_);
      auto it = connected_keyframe_weights_.find(kf);
      if (it != connected_keyframe_weights_.end() && it->second == weight) return;
      connected_keyframe_weights_[kf] = weight;
      n_writes_++;
    }
    UpdateBestCovisibles();
  }
  void UpdateBestCovisibles() {
    std::unique_lock<std::mutex> lock(mutex_connections_);
    std::vector<std::pair<int, ConnKeyFrame*> > pairs;
    pairs.reserve(connected_keyframe_weights_.size());
    for (auto& w : connected_keyframe_weights_) pairs.push_back(std::make_pair(w.second, w.first));
    SetOrdered(pairs);
  }
  void UpdateConnections(int th = 15) {
    std::map<ConnKeyFrame*, int> counter;
    const std::vector<ConnMapPoint*> mps = map_points_;
    for (ConnMapPoint* mp : mps) {
      if (!mp || mp->isBad()) continue;
      const std::map<ConnKeyFrame*, size_t> obs = mp->GetObservations();
      for (auto& o : obs) if (o.first->id_ != id_) counter[o.first]++;
    }
    if (counter.empty()) return;
    int nmax = 0; ConnKeyFrame* kmax = nullptr;
    std::vector<std::pair<int, ConnKeyFrame*> > pairs;
    pairs.reserve(counter.size());
    for (auto& c : counter) {
      if (c.second > nmax) { nmax = c.second; kmax = c.first; }
      if (c.second >= th) { pairs.push_back(std::make_pair(c.second, c.first)); c.first->AddConnection(this, c.second); }
    }
    if (pairs.empty()) { pairs.push_back(std::make_pair(nmax, kmax)); kmax->AddConnection(this, nmax); }
    ConnKeyFrame* parent = nullptr;
    {
      std::unique_lock<std::mutex> lock(mutex_connections_);
      connected_keyframe_weights_ = counter;
      n_writes_++;
      SetOrdered(pairs);
      if (is_first_connection_ && id_ != 0) { parent_ = ordered_connected_keyframes_.front(); parent = parent_; is_first_connection_ = false; }
    }
    if (parent) parent->AddChild(this);
  }

 protected:
  template <class> friend struct ORB_SLAM2::FrameOpsT;              // (the line INTEGRATION.md section 4 adds to include/KeyFrame.h)
  friend struct ConnScene;
  friend struct ConnCompare;
  void SetOrdered(std::vector<std::pair<int, ConnKeyFrame*> >& pairs) {        // ascending sort, then push_front: descending (weight, pointer)
    std::sort(pairs.begin(), pairs.end(), [](const std::pair<int, ConnKeyFrame*>& a, const std::pair<int, ConnKeyFrame*>& b) {
      return a.first != b.first ? a.first < b.first : std::less<ConnKeyFrame*>()(a.second, b.second);
    });
    std::list<ConnKeyFrame*> kl; std::list<int> wl;
    for (auto& p : pairs) { kl.push_front(p.second); wl.push_front(p.first); }
    ordered_connected_keyframes_.assign(kl.begin(), kl.end());
    ordered_weights_.assign(wl.begin(), wl.end());
  }
  std::map<ConnKeyFrame*, int> connected_keyframe_weights_;
  std::vector<ConnKeyFrame*> ordered_connected_keyframes_;
  std::vector<int> ordered_weights_;
  bool is_first_connection_ = true;
  ConnKeyFrame* parent_ = nullptr;
  std::set<ConnKeyFrame*> childrens_;
  std::mutex mutex_connections_;
};

struct ConnTypes {
  typedef mock::Frame Frame; typedef ConnKeyFrame KeyFrame; typedef ConnMapPoint MapPoint;
  typedef mock::Matrix3d Matrix3d; typedef mock::Vector3d Vector3d;
};

// the loop of LoopClosing::CorrectLoop (src/LoopClosing.cc:551-573) on the host
inline void UpdateConnectionsHost(const std::vector<ConnKeyFrame*>& keyframes, std::map<ConnKeyFrame*, std::set<ConnKeyFrame*> >& loop_connections, int th = 15) {
  for (ConnKeyFrame* kf : keyframes) {
    const std::vector<ConnKeyFrame*> previous = kf->GetVectorCovisibleKeyFrames();
    kf->UpdateConnections(th);
    loop_connections[kf] = kf->GetConnectedKeyFrames();
    for (ConnKeyFrame* p : previous) loop_connections[kf].erase(p);
    for (ConnKeyFrame* k2 : keyframes) loop_connections[kf].erase(k2);
  }
}

// n_kf keyframes along a path, keyframe index i living at store[place[i]] (a seeded shuffle); per_kf * n_kf / 4 points each seen by 2-6
// keyframes of a window; keyframe n_kf - 2 sees only points of its own (empty counter), n_kf - 1 shares 4 points with keyframe 0 (the
// maximum below th).  Every fifth keyframe lists some of its points twice.  The tables at entry are stale: some keyframes carry a map
// with wrong weights and a list sorted from it, some a map but an empty list, some nothing; a third have had their first connection.
struct ConnScene {
  std::vector<ConnKeyFrame> store; std::vector<ConnMapPoint> mps; std::vector<int> place;
  ConnKeyFrame& kf(int i) { return store[place[i]]; }
  int index_of(const ConnKeyFrame* k) const { const int at = (int)(k - store.data()); for (size_t i = 0; i < place.size(); i++) if (place[i] == at) return (int)i; return -1; }
  void build(unsigned seed, int n_kf, int per_kf, int window) {
    std::mt19937 rng(seed);
    store = std::vector<ConnKeyFrame>(n_kf); place.resize(n_kf);
    for (int i = 0; i < n_kf; i++) place[i] = i;
    std::shuffle(place.begin(), place.end(), rng);
    for (int i = 0; i < n_kf; i++) kf(i).id_ = (unsigned long)i;
    const int body = n_kf - 2, n_mp = body * per_kf / 4;
    mps = std::vector<ConnMapPoint>(n_mp + 9);
    auto see = [&](int k, int p) { kf(k).map_points_.push_back(&mps[p]); mps[p].observations_[&kf(k)] = kf(k).map_points_.size() - 1; };
    for (int p = 0; p < n_mp; p++) {
      const int c = (int)(rng() % body), lo = std::max(0, c - window), hi = std::min(body, c + window + 1);
      std::vector<int> cand;
      for (int k = lo; k < hi; k++) cand.push_back(k);
      std::shuffle(cand.begin(), cand.end(), rng);
      const int n = std::min((int)cand.size(), 2 + (int)(rng() % 5));
      for (int j = 0; j < n; j++) { if (rng() % 6 == 0) kf(cand[j]).map_points_.push_back(nullptr); see(cand[j], p); }
      if (rng() % 40 == 0) mps[p].is_bad_ = true;
    }
    for (int j = 0; j < 5; j++) see(n_kf - 2, n_mp + j);
    for (int j = 0; j < 4; j++) { see(0, n_mp + 5 + j); see(n_kf - 1, n_mp + 5 + j); }
    for (int i = 0; i < n_kf; i += 5) {
      ConnKeyFrame& k = kf(i);
      const size_t n = k.map_points_.size();
      for (size_t s = 0; s < n; s += 7) if (k.map_points_[s]) k.map_points_.push_back(k.map_points_[s]);
    }
    for (int i = 0; i < n_kf; i++) {
      ConnKeyFrame& k = kf(i);
      const int kind = (int)(rng() % 3);
      if (kind == 2) continue;
      for (int j = 0; j < 8; j++) {
        const int o = std::min(n_kf - 1, std::max(0, i + (int)(rng() % 9) - 4));
        if (o != i) k.connected_keyframe_weights_[&kf(o)] = 1 + (int)(rng() % 40);
      }
      if (kind == 0) k.UpdateBestCovisibles();
      k.is_first_connection_ = rng() % 3 != 0;
    }
  }
};

}  // namespace mock
