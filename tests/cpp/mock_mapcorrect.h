// What the map-correction drop-in test needs beside mock_orbslam.h: a keyframe with a pose (SetPose as src/KeyFrame.cc:119-130, the
// arithmetic order include/orbslam_hip.h states), the global-BA members, the spanning tree and the covisibility members of
// mock_connections.h; a map point with position, normal, depth range, observations in a real std::map<KF*, size_t> and the loop-closing
// stamps; a map with keyframe_origins_; the reference-shaped host loops of src/LoopClosing.cc:437-523 and :681-739 written with the
// Sim3 arithmetic of csrc/sim3_math.h restated in plain C++ (compile with -ffp-contract=off); and a builder whose keyframes lie in memory
// in an order that is NOT their index order.  TEST INFRASTRUCTURE.
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

struct McKeyFrame;

struct McMapPoint {
  std::map<McKeyFrame*, size_t> observations_; bool is_bad_ = false;
  Vector3d world_pose_, normal_vector_, global_BA_pose_; float min_distance_ = 0, max_distance_ = 0;
  McKeyFrame* reference_keyframe_ = nullptr;
  unsigned long corrected_by_keyframe_ = 0, corrected_reference_ = 0, n_BA_global_for_keyframe_ = 0;
  std::map<McKeyFrame*, size_t> GetObservations() { return observations_; }
  bool isBad() { return is_bad_; }
  Vector3d GetWorldPos() { return world_pose_; }
  void SetWorldPos(const Vector3d& p) { world_pose_ = p; }
  McKeyFrame* GetReferenceKeyFrame() { return reference_keyframe_; }
  inline void UpdateNormalAndDepth();                              // (src/MapPoint.cc:335-378; below, it needs the keyframe)
};

struct McKeyFrame {
  // ---- pose (src/KeyFrame.cc:119-141) and what UpdateNormalAndDepth reads of its reference keyframe
  Matrix4d Tcw_, Twc_; Vector3d Ow_;
  Matrix4d global_BA_Tcw_, global_BA_Bef_Tcw_; unsigned long n_BA_global_for_keyframe_ = 0;
  std::vector<KeyPoint> undistort_keypoints_; std::vector<float> scale_factors_; int n_scale_levels_ = 8;
  bool is_bad_ = false;
  void SetPose(const Matrix4d& T) {                                 // Rwc = Rcw^T, Ow = -(Rwc tcw), each dot product (a0 b0 + a1 b1) + a2 b2
    Tcw_ = T;
    Twc_ = Matrix4d();
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Twc_(i, j) = T(j, i);
      Ow_[i] = -((T(0, i) * T(0, 3) + T(1, i) * T(1, 3)) + T(2, i) * T(2, 3));
      Twc_(i, 3) = Ow_[i];
    }
  }
  Matrix4d GetPose() { return Tcw_; }
  Matrix4d GetPoseInverse() { return Twc_; }
  Vector3d GetCameraCenter() { return Ow_; }
  bool isBad() { return is_bad_; }
  std::set<McKeyFrame*> GetChilds() { std::unique_lock<std::mutex> lock(mutex_connections_); return childrens_; }
  void AddChildForTest(McKeyFrame* kf) { childrens_.insert(kf); kf->parent_ = this; kf->is_first_connection_ = false; }
  // ---- covisibility, as mock_connections.h has it
  unsigned long id_ = 0;
  int n_writes_ = 0;                                              // how often the host loop below wrote this keyframe's tables (the tests count with it)
  std::vector<McMapPoint*> map_points_;
  std::vector<McMapPoint*> GetMapPointMatches() { return map_points_; }
  std::vector<McKeyFrame*> GetVectorCovisibleKeyFrames() { std::unique_lock<std::mutex> lock(mutex_connections_); return ordered_connected_keyframes_; }
  std::set<McKeyFrame*> GetConnectedKeyFrames() {
    std::unique_lock<std::mutex> lock(mutex_connections_);
    std::set<McKeyFrame*> s;
    for (auto& w : connected_keyframe_weights_) s.insert(w.first);
    return s;
  }
  void AddChild(McKeyFrame* kf) { std::unique_lock<std::mutex> lock(mutex_connections_); childrens_.insert(kf); }

  void AddConnection(McKeyFrame* kf, const int& weight) {
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
    std::vector<std::pair<int, McKeyFrame*> > pairs;
    pairs.reserve(connected_keyframe_weights_.size());
    for (auto& w : connected_keyframe_weights_) pairs.push_back(std::make_pair(w.second, w.first));
    SetOrdered(pairs);
  }
  void UpdateConnections(int th = 15) {
    std::map<McKeyFrame*, int> counter;
    const std::vector<McMapPoint*> mps = map_points_;
    for (McMapPoint* mp : mps) {
      if (!mp || mp->isBad()) continue;
      const std::map<McKeyFrame*, size_t> obs = mp->GetObservations();
      for (auto& o : obs) if (o.first->id_ != id_) counter[o.first]++;
    }
    if (counter.empty()) return;
    int nmax = 0; McKeyFrame* kmax = nullptr;
    std::vector<std::pair<int, McKeyFrame*> > pairs;
    pairs.reserve(counter.size());
    for (auto& c : counter) {
      if (c.second > nmax) { nmax = c.second; kmax = c.first; }
      if (c.second >= th) { pairs.push_back(std::make_pair(c.second, c.first)); c.first->AddConnection(this, c.second); }
    }
    if (pairs.empty()) { pairs.push_back(std::make_pair(nmax, kmax)); kmax->AddConnection(this, nmax); }
    McKeyFrame* parent = nullptr;
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
  friend struct McScene;
  friend struct McCompare;
  void SetOrdered(std::vector<std::pair<int, McKeyFrame*> >& pairs) {        // ascending sort, then push_front: descending (weight, pointer)
    std::sort(pairs.begin(), pairs.end(), [](const std::pair<int, McKeyFrame*>& a, const std::pair<int, McKeyFrame*>& b) {
      return a.first != b.first ? a.first < b.first : std::less<McKeyFrame*>()(a.second, b.second);
    });
    std::list<McKeyFrame*> kl; std::list<int> wl;
    for (auto& p : pairs) { kl.push_front(p.second); wl.push_front(p.first); }
    ordered_connected_keyframes_.assign(kl.begin(), kl.end());
    ordered_weights_.assign(wl.begin(), wl.end());
  }
  std::map<McKeyFrame*, int> connected_keyframe_weights_;
  std::vector<McKeyFrame*> ordered_connected_keyframes_;
  std::vector<int> ordered_weights_;
  bool is_first_connection_ = true;
  McKeyFrame* parent_ = nullptr;
  std::set<McKeyFrame*> childrens_;
  std::mutex mutex_connections_;
};

inline void McMapPoint::UpdateNormalAndDepth() {
  if (is_bad_) return;
  std::map<McKeyFrame*, size_t> observations = observations_;
  if (observations.empty()) return;
  const Vector3d pos = world_pose_;
  double n[3] = {0, 0, 0}; int cnt = 0;
  for (auto& o : observations) {
    const Vector3d Owi = o.first->GetCameraCenter();
    const double v[3] = {pos[0] - Owi[0], pos[1] - Owi[1], pos[2] - Owi[2]};
    const double nn = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int k = 0; k < 3; k++) n[k] = n[k] + v[k] / nn;
    cnt++;
  }
  const Vector3d Ow = reference_keyframe_->GetCameraCenter();
  const double pc[3] = {pos[0] - Ow[0], pos[1] - Ow[1], pos[2] - Ow[2]};
  const float dist = (float)std::sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
  const int level = reference_keyframe_->undistort_keypoints_[observations[reference_keyframe_]].octave;
  max_distance_ = dist * reference_keyframe_->scale_factors_[level];
  min_distance_ = max_distance_ / reference_keyframe_->scale_factors_[reference_keyframe_->n_scale_levels_ - 1];
  for (int k = 0; k < 3; k++) normal_vector_[k] = n[k] / (double)cnt;
}

struct McMap {
  std::vector<McKeyFrame*> keyframe_origins_, keyframes_; std::vector<McMapPoint*> map_points_;
  std::mutex mutex_map_update_;
  std::vector<McKeyFrame*> GetAllKeyFrames() { return keyframes_; }
  std::vector<McMapPoint*> GetAllMapPoints() { return map_points_; }
};

struct McTypes {
  typedef mock::Frame Frame; typedef McKeyFrame KeyFrame; typedef McMapPoint MapPoint; typedef McMap Map;
  typedef mock::Matrix3d Matrix3d; typedef mock::Matrix4d Matrix4d; typedef mock::Vector3d Vector3d; typedef mock::Sim3d Sim3;
};
typedef std::map<McKeyFrame*, Sim3d> McKeyFrameAndSim3;

// ---- the Sim3 arithmetic of csrc/sim3_math.h and the pose codec, restated --------------------------------------------------------
namespace mcm {
inline void rot_scale(const double* q, const double* p, double* out) {
  const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const double cx = 2 * (q[1] * p[2] - q[2] * p[1]), cy = 2 * (q[2] * p[0] - q[0] * p[2]), cz = 2 * (q[0] * p[1] - q[1] * p[0]);
  out[0] = n2 * p[0] + (q[3] * cx + (q[1] * cz - q[2] * cy));
  out[1] = n2 * p[1] + (q[3] * cy + (q[2] * cx - q[0] * cz));
  out[2] = n2 * p[2] + (q[3] * cz + (q[0] * cy - q[1] * cx));
}
inline Vector3d act(const Sim3d& S, const Vector3d& p) { double o[3]; rot_scale(S.d, p.v, o); return Vector3d(o[0] + S.d[4], o[1] + S.d[5], o[2] + S.d[6]); }
inline Sim3d inverse(const Sim3d& S) {
  Sim3d o; const double* s = S.d;
  const double n2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3];
  o.d[0] = -s[0] / n2; o.d[1] = -s[1] / n2; o.d[2] = -s[2] / n2; o.d[3] = s[3] / n2;
  double t[3]; rot_scale(o.d, s + 4, t);
  o.d[4] = -t[0]; o.d[5] = -t[1]; o.d[6] = -t[2];
  return o;
}
inline Sim3d mul(const Sim3d& SA, const Sim3d& SB) {
  const double *A = SA.d, *B = SB.d; Sim3d o; double t[3];
  rot_scale(A, B + 4, t);
  o.d[0] = A[3] * B[0] + A[0] * B[3] + A[1] * B[2] - A[2] * B[1];
  o.d[1] = A[3] * B[1] + A[1] * B[3] + A[2] * B[0] - A[0] * B[2];
  o.d[2] = A[3] * B[2] + A[2] * B[3] + A[0] * B[1] - A[1] * B[0];
  o.d[3] = A[3] * B[3] - A[0] * B[0] - A[1] * B[1] - A[2] * B[2];
  o.d[4] = A[4] + t[0]; o.d[5] = A[5] + t[1]; o.d[6] = A[6] + t[2];
  return o;
}
inline Sim3d from_se3(const Matrix4d& T) {                           // Sophus::Sim3d(Sophus::RxSO3d(1.0, R), t)
  Sim3d S; double* q = S.d; const double (*m)[4] = T.m;
  double t = m[0][0] + m[1][1] + m[2][2];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
    q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t;
  }
  q[4] = T(0, 3); q[5] = T(1, 3); q[6] = T(2, 3);
  return S;
}
inline Matrix4d to_pose(const Sim3d& S) {                            // [R | t / s]
  const double* s = S.d;
  const double sc = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3], inv = 1.0 / std::sqrt(sc);
  const double x = s[0] * inv, y = s[1] * inv, z = s[2] * inv, w = s[3] * inv;
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  Matrix4d T;
  T(0, 0) = 1 - (tyy + tzz); T(0, 1) = txy - twz; T(0, 2) = txz + twy;
  T(1, 0) = txy + twz; T(1, 1) = 1 - (txx + tzz); T(1, 2) = tyz - twx;
  T(2, 0) = txz - twy; T(2, 1) = tyz + twx; T(2, 2) = 1 - (txx + tyy);
  const double inv_s = 1. / sc;
  for (int i = 0; i < 3; i++) T(i, 3) = inv_s * s[4 + i];
  return T;
}
inline Matrix4d mul44(const Matrix4d& A, const Matrix4d& B) {        // index order k = 0..3
  Matrix4d C;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) C(i, j) = ((A(i, 0) * B(0, j) + A(i, 1) * B(1, j)) + A(i, 2) * B(2, j)) + A(i, 3) * B(3, j);
  return C;
}
inline Vector3d apply(const Matrix4d& T, const Vector3d& x) {
  Vector3d o;
  for (int i = 0; i < 3; i++) o[i] = ((T(i, 0) * x[0] + T(i, 1) * x[1]) + T(i, 2) * x[2]) + T(i, 3);
  return o;
}
}  // namespace mcm

// LoopClosing::CorrectLoop, src/LoopClosing.cc:437-523, on the host
inline void CorrectLoopHost(McKeyFrame* current, const std::vector<McKeyFrame*>& connected, const Sim3d& Scw, McKeyFrameAndSim3& corrected, McKeyFrameAndSim3& non_corrected) {
  corrected[current] = Scw;
  const Matrix4d Twc = current->GetPoseInverse();
  for (McKeyFrame* kf : connected) {
    const Matrix4d Tiw = kf->GetPose();
    if (kf != current) corrected[kf] = mcm::mul(mcm::from_se3(mcm::mul44(Tiw, Twc)), Scw);
    non_corrected[kf] = mcm::from_se3(Tiw);
  }
  for (auto& it : corrected) {
    McKeyFrame* kf = it.first;
    const Sim3d Swi = mcm::inverse(it.second), Siw = non_corrected[kf];
    const std::vector<McMapPoint*> mps = kf->GetMapPointMatches();
    for (McMapPoint* mp : mps) {
      if (!mp || mp->isBad() || mp->corrected_by_keyframe_ == current->id_) continue;
      mp->SetWorldPos(mcm::act(Swi, mcm::act(Siw, mp->GetWorldPos())));
      mp->corrected_by_keyframe_ = current->id_;
      mp->corrected_reference_ = kf->id_;
      mp->UpdateNormalAndDepth();
    }
    kf->SetPose(mcm::to_pose(it.second));
    kf->UpdateConnections();
  }
}

// LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:681-739, on the host
inline void PropagateGlobalBAHost(McMap* map, unsigned long nLoopKF) {
  std::list<McKeyFrame*> todo(map->keyframe_origins_.begin(), map->keyframe_origins_.end());
  while (!todo.empty()) {
    McKeyFrame* kf = todo.front();
    const std::set<McKeyFrame*> childs = kf->GetChilds();
    const Matrix4d Twc = kf->GetPoseInverse();
    for (McKeyFrame* child : childs) {
      if (child->n_BA_global_for_keyframe_ != nLoopKF) {
        child->global_BA_Tcw_ = mcm::mul44(mcm::mul44(child->GetPose(), Twc), kf->global_BA_Tcw_);
        child->n_BA_global_for_keyframe_ = nLoopKF;
      }
      todo.push_back(child);
    }
    kf->global_BA_Bef_Tcw_ = kf->GetPose();
    kf->SetPose(kf->global_BA_Tcw_);
    todo.pop_front();
  }
  for (McMapPoint* mp : map->GetAllMapPoints()) {
    if (mp->isBad()) continue;
    if (mp->n_BA_global_for_keyframe_ == nLoopKF) { mp->SetWorldPos(mp->global_BA_pose_); continue; }
    McKeyFrame* ref = mp->GetReferenceKeyFrame();
    if (ref->n_BA_global_for_keyframe_ != nLoopKF) continue;
    mp->SetWorldPos(mcm::apply(ref->GetPoseInverse(), mcm::apply(ref->global_BA_Bef_Tcw_, mp->GetWorldPos())));
  }
}

}  // namespace mock
