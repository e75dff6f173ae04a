// What the GlobalBundleAdjustemnt drop-in test needs beside mock_orbslam.h: a keyframe with a pose (SetPose as src/KeyFrame.cc:119-130, the
// arithmetic order include/orbslam_hip.h states), intrinsics, undistorted keypoints, the level tables and the two global-BA members; a map
// point with its observations in a real std::map<KF*, size_t>, the reference keyframe, UpdateNormalAndDepth (src/MapPoint.cc:335-378) and
// the two global-BA members; a map that hands over its keyframes and points in pointer order (std::set); and the reference-shaped host
// loops of src/CeresOptimizer.cc:59-176 and :190-224 in the text of CeresOptimizerT::BundleAdjustment (csrc/compat/orbslam_dropin.h), cut
// at the solve so that one solution can be written back.  Compile with -ffp-contract=off.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "mock_orbslam.h"

namespace mock {

struct GbKeyFrame;

struct GbMapPoint {
  std::map<GbKeyFrame*, size_t> observations_; bool is_bad_ = false;
  Vector3d world_pose_, normal_vector_, global_BA_pose_; float min_distance_ = 0, max_distance_ = 0;
  GbKeyFrame* reference_keyframe_ = nullptr;
  unsigned long n_BA_global_for_keyframe_ = 0;
  std::map<GbKeyFrame*, size_t> GetObservations() { return observations_; }
  bool isBad() { return is_bad_; }
  Vector3d GetWorldPos() { return world_pose_; }
  void SetWorldPos(const Vector3d& p) { world_pose_ = p; }
  GbKeyFrame* GetReferenceKeyFrame() { return reference_keyframe_; }
  inline void UpdateNormalAndDepth();
};

struct GbKeyFrame {
  unsigned long id_ = 0, n_BA_global_for_keyframe_ = 0;
  Matrix4d Tcw_, Twc_, global_BA_Tcw_; Vector3d Ow_;
  float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
  std::vector<KeyPoint> undistort_keypoints_; std::vector<float> scale_factors_, inv_level_sigma2s_; int n_scale_levels_ = 8;
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
  Vector3d GetCameraCenter() { return Ow_; }
  bool isBad() { return is_bad_; }
};

inline void GbMapPoint::UpdateNormalAndDepth() {                    // :335-378
  if (is_bad_) return;
  std::map<GbKeyFrame*, size_t> observations = observations_;
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
  const int level = reference_keyframe_->undistort_keypoints_[observations[reference_keyframe_]].octave;       // (operator[] inserts index 0)
  max_distance_ = dist * reference_keyframe_->scale_factors_[level];
  min_distance_ = max_distance_ / reference_keyframe_->scale_factors_[reference_keyframe_->n_scale_levels_ - 1];
  for (int k = 0; k < 3; k++) normal_vector_[k] = n[k] / (double)cnt;
}

struct GbMap {
  std::mutex mutex_map_update_;
  std::vector<GbKeyFrame*> keyframes_; std::vector<GbMapPoint*> map_points_;      // (kept in pointer order: what a std::set hands over)
  std::vector<GbKeyFrame*> GetAllKeyFrames() { return keyframes_; }
  std::vector<GbMapPoint*> GetAllMapPoints() { return map_points_; }
};

struct GbTypes {
  typedef mock::Frame Frame; typedef GbKeyFrame KeyFrame; typedef GbMapPoint MapPoint; typedef GbMap Map;
  typedef mock::Matrix3d Matrix3d; typedef mock::Matrix4d Matrix4d; typedef mock::Vector2d Vector2d; typedef mock::Vector3d Vector3d;
  typedef mock::Quaterniond Quaterniond; typedef mock::Mat Mat; typedef mock::Point2f Point2f;
  typedef mock::Sim3d Sim3; typedef std::map<GbKeyFrame*, mock::Sim3d> KeyFrameAndSim3;
};

// the flat problem of CeresOptimizerT::BundleAdjustment (csrc/compat/orbslam_dropin.h), as ba_solve takes it
struct GbProblem {
  std::vector<GbKeyFrame*> cams; std::vector<GbMapPoint*> pts; std::vector<std::pair<GbKeyFrame*, GbMapPoint*> > edges;
  std::vector<double> K4, poses7, pts3, obs_uv, obs_w; std::vector<int32_t> obs_cam, obs_pt; std::vector<uint8_t> cam_fixed, obs_rob;
};

inline void AssembleHost(const std::vector<GbKeyFrame*>& keyframes, const std::vector<GbMapPoint*>& map_points, bool is_robust, GbProblem* P) {
  if (keyframes.empty()) return;
  unsigned long max_keyframe_id = 0;
  std::map<GbKeyFrame*, int> cam_of;
  std::vector<GbKeyFrame*> kf_by_id(keyframes);
  std::stable_sort(kf_by_id.begin(), kf_by_id.end(), [](const GbKeyFrame* a, const GbKeyFrame* b) { return a->id_ < b->id_; });
  for (GbKeyFrame* keyframe : kf_by_id) {
    if (keyframe->isBad()) continue;
    if (cam_of.count(keyframe)) continue;
    double T[16], p7[7];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[4 * r + c] = keyframe->Tcw_(r, c);
    ba_matrix4d_to_pose7(T, p7);
    cam_of[keyframe] = (int)P->cams.size(); P->cams.push_back(keyframe);
    P->poses7.insert(P->poses7.end(), p7, p7 + 7);
    const double k4[4] = {keyframe->fx_, keyframe->fy_, keyframe->cx_, keyframe->cy_};
    P->K4.insert(P->K4.end(), k4, k4 + 4);
    P->cam_fixed.push_back(keyframe->id_ == 0 ? 1 : 0);
    if (keyframe->id_ > max_keyframe_id) max_keyframe_id = keyframe->id_;
  }
  for (GbMapPoint* map_point : map_points) {
    if (map_point->isBad()) continue;
    const std::map<GbKeyFrame*, size_t> observations = map_point->GetObservations();
    int n_edges = 0;
    const int pid = (int)P->pts.size();
    for (auto it = observations.begin(); it != observations.end(); ++it) {
      GbKeyFrame* keyframe = it->first;
      if (keyframe->isBad() || keyframe->id_ > max_keyframe_id) continue;
      auto c = cam_of.find(keyframe);
      if (c == cam_of.end()) continue;
      n_edges++;
      const KeyPoint& kp = keyframe->undistort_keypoints_[it->second];
      P->obs_cam.push_back(c->second); P->obs_pt.push_back(pid);
      P->obs_uv.push_back(kp.pt.x); P->obs_uv.push_back(kp.pt.y);
      P->obs_w.push_back((double)keyframe->inv_level_sigma2s_[kp.octave]);
      P->obs_rob.push_back(is_robust ? 1 : 0);
      P->edges.push_back(std::make_pair(keyframe, map_point));
    }
    if (n_edges == 0) continue;
    P->pts.push_back(map_point);
    for (int k = 0; k < 3; k++) P->pts3.push_back(map_point->world_pose_[k]);
  }
}

// src/CeresOptimizer.cc:190-224 with the solver's poses7 and pts3
inline void ApplyHost(GbProblem* P, const double* poses7, const double* pts3, unsigned long n_loop_keyframe) {
  for (size_t c = 0; c < P->cams.size(); c++) {
    GbKeyFrame* keyframe = P->cams[c];
    if (keyframe->isBad()) continue;
    double T[16];
    ba_pose7_to_matrix4d(poses7 + 7 * c, T);
    Matrix4d pose;
    for (int r = 0; r < 4; r++) for (int q = 0; q < 4; q++) pose(r, q) = T[4 * r + q];
    if (n_loop_keyframe == 0) keyframe->SetPose(pose);
    else { keyframe->global_BA_Tcw_ = pose; keyframe->n_BA_global_for_keyframe_ = n_loop_keyframe; }
  }
  for (size_t p = 0; p < P->pts.size(); p++) {
    GbMapPoint* map_point = P->pts[p];
    if (map_point->isBad()) continue;
    const Vector3d X(pts3[3 * p], pts3[3 * p + 1], pts3[3 * p + 2]);
    if (n_loop_keyframe == 0) { map_point->SetWorldPos(X); map_point->UpdateNormalAndDepth(); }
    else { map_point->global_BA_pose_ = X; map_point->n_BA_global_for_keyframe_ = n_loop_keyframe; }
  }
}

}  // namespace mock
