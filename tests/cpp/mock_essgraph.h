// What the OptimizeEssentialGraph drop-in test needs beside mock_orbslam.h: a keyframe with a pose (SetPose as src/KeyFrame.cc:119-130, the
// arithmetic order include/orbslam_hip.h states), the spanning tree (GetParent, GetChilds, hasChild), loop edges, the weight map and the
// two ordered lists with GetWeight / GetCovisiblesByWeight (src/KeyFrame.cc:218-235, :312-319), undistorted keypoints and the scale
// table; a map point with its observations in a real std::map<KF*, size_t>, the reference keyframe, the two loop-closing stamps and
// UpdateNormalAndDepth (src/MapPoint.cc:335-378); a map that lists both in pointer order (the reference holds std::set) with
// mutex_map_update_.  Compile with -ffp-contract=off.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "mock_orbslam.h"

namespace mock {

struct EgKeyFrame;

struct EgMapPoint {
  std::map<EgKeyFrame*, size_t> observations_; bool is_bad_ = false;
  Vector3d world_pose_, normal_vector_; float min_distance_ = 0, max_distance_ = 0;
  EgKeyFrame* reference_keyframe_ = nullptr;
  unsigned long corrected_by_keyframe_ = ~0ul, corrected_reference_ = 0;
  int n_update_normal_calls_ = 0;
  std::map<EgKeyFrame*, size_t> GetObservations() { return observations_; }
  bool isBad() { return is_bad_; }
  Vector3d GetWorldPos() { return world_pose_; }
  void SetWorldPos(const Vector3d& p) { world_pose_ = p; }
  EgKeyFrame* GetReferenceKeyFrame() { return reference_keyframe_; }
  inline void UpdateNormalAndDepth();
};

struct EgKeyFrame {
  unsigned long id_ = 0;
  Matrix4d Tcw_; Vector3d Ow_; bool is_bad_ = false;
  std::vector<KeyPoint> undistort_keypoints_; std::vector<float> scale_factors_; int n_scale_levels_ = 8;
  std::vector<EgKeyFrame*> ordered_connected_keyframes_; std::vector<int> ordered_weights_; std::map<EgKeyFrame*, int> connected_keyframe_weights_;
  EgKeyFrame* parent_ = nullptr; std::set<EgKeyFrame*> children_, loop_edges_;
  void SetPose(const Matrix4d& T) {                                 // Rwc = Rcw^T, Ow = -(Rwc tcw), each dot product (a0 b0 + a1 b1) + a2 b2
    Tcw_ = T;
    for (int i = 0; i < 3; i++) Ow_[i] = -((T(0, i) * T(0, 3) + T(1, i) * T(1, 3)) + T(2, i) * T(2, 3));
  }
  Matrix4d GetPose() { return Tcw_; }
  Vector3d GetCameraCenter() { return Ow_; }
  bool isBad() { return is_bad_; }
  EgKeyFrame* GetParent() { return parent_; }
  std::set<EgKeyFrame*> GetChilds() { return children_; }
  bool hasChild(EgKeyFrame* kf) { return children_.count(kf) != 0; }
  std::set<EgKeyFrame*> GetLoopEdges() { return loop_edges_; }
  int GetWeight(EgKeyFrame* kf) { auto it = connected_keyframe_weights_.find(kf); return it == connected_keyframe_weights_.end() ? 0 : it->second; }
  std::vector<EgKeyFrame*> GetCovisiblesByWeight(const int& w) {
    size_t n = 0; while (n < ordered_weights_.size() && ordered_weights_[n] >= w) n++;
    if (ordered_connected_keyframes_.empty() || n == ordered_weights_.size()) return std::vector<EgKeyFrame*>();
    return std::vector<EgKeyFrame*>(ordered_connected_keyframes_.begin(), ordered_connected_keyframes_.begin() + n);
  }
};

inline void EgMapPoint::UpdateNormalAndDepth() {                    // src/MapPoint.cc:335-378
  n_update_normal_calls_++;
  if (is_bad_) return;
  std::map<EgKeyFrame*, size_t> observations = observations_;
  if (observations.empty() || !reference_keyframe_) return;
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

struct EgMap {
  std::mutex mutex_map_update_;
  std::set<EgKeyFrame*> keyframes_; std::set<EgMapPoint*> map_points_;
  std::vector<EgKeyFrame*> GetAllKeyFrames() { return std::vector<EgKeyFrame*>(keyframes_.begin(), keyframes_.end()); }
  std::vector<EgMapPoint*> GetAllMapPoints() { return std::vector<EgMapPoint*>(map_points_.begin(), map_points_.end()); }
};

struct EgTypes {
  typedef mock::Frame Frame; typedef EgKeyFrame KeyFrame; typedef EgMapPoint MapPoint; typedef EgMap Map;
  typedef mock::Matrix3d Matrix3d; typedef mock::Matrix4d Matrix4d; typedef mock::Vector2d Vector2d; typedef mock::Vector3d Vector3d;
  typedef mock::Quaterniond Quaterniond; typedef mock::Mat Mat; typedef mock::Point2f Point2f;
  typedef mock::Sim3d Sim3; typedef std::map<EgKeyFrame*, mock::Sim3d> KeyFrameAndSim3;
};

}  // namespace mock
