// What the LocalBundleAdjustment drop-in test needs beside mock_orbslam.h: a keyframe with a pose (SetPose as src/KeyFrame.cc:119-130, the
// arithmetic order include/orbslam_hip.h states), intrinsics, undistorted keypoints, the level tables, its slots with both
// EraseMapPointMatch forms (src/KeyFrame.cc:250-260), a covisible list the test sets, and the two BA stamps; a map point with its
// observations in a real std::map<KF*, size_t>, Observations(), the reference keyframe, EraseObservation with its SetBadFlag cascade
// (src/MapPoint.cc:140-191) and UpdateNormalAndDepth (:335-378); a map with mutex_map_update_; and the reference-shaped host loops of
// src/CeresOptimizer.cc:346-406, :423-506 (in the camera order csrc/compat/orbslam_dropin.h fixed) and :573-598.  Compile with
// -ffp-contract=off.  TEST INFRASTRUCTURE.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "mock_orbslam.h"

namespace ORB_SLAM2 { template <class> struct FrameOpsT; }

namespace mock {

struct LbKeyFrame;

struct LbMapPoint {
  std::map<LbKeyFrame*, size_t> observations_; int n_observations_ = 0; bool is_bad_ = false;
  Vector3d world_pose_, normal_vector_; float min_distance_ = 0, max_distance_ = 0;
  LbKeyFrame* reference_keyframe_ = nullptr;
  unsigned long n_BA_local_for_keyframe_ = ~0ul;
  std::map<LbKeyFrame*, size_t> GetObservations() { return observations_; }
  int Observations() { return n_observations_; }
  bool isBad() { return is_bad_; }
  Vector3d GetWorldPos() { return world_pose_; }
  void SetWorldPos(const Vector3d& p) { world_pose_ = p; }
  LbKeyFrame* GetReferenceKeyFrame() { return reference_keyframe_; }
  int GetIndexInKeyFrame(LbKeyFrame* kf) { return observations_.count(kf) ? (int)observations_[kf] : -1; }
  inline void EraseObservation(LbKeyFrame* kf);
  inline void SetBadFlag();
  inline void UpdateNormalAndDepth();
};

struct LbKeyFrame {
  unsigned long id_ = 0, n_BA_local_for_keyframe_ = ~0ul, n_BA_fixed_for_keyframe_ = ~0ul;
  Matrix4d Tcw_, Twc_; Vector3d Ow_;
  float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
  std::vector<KeyPoint> undistort_keypoints_; std::vector<float> scale_factors_, inv_level_sigma2s_; int n_scale_levels_ = 8;
  bool is_bad_ = false;
  std::vector<LbMapPoint*> map_points_;
  std::vector<LbKeyFrame*> covisible_;
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
  std::vector<LbMapPoint*> GetMapPointMatches() { return map_points_; }
  std::vector<LbKeyFrame*> GetVectorCovisibleKeyFrames() { return covisible_; }
  void EraseMapPointMatch(const size_t& index) { map_points_[index] = static_cast<LbMapPoint*>(nullptr); }
  void EraseMapPointMatch(LbMapPoint* mp) { const int index = mp->GetIndexInKeyFrame(this); if (index >= 0) map_points_[index] = static_cast<LbMapPoint*>(nullptr); }
};

inline void LbMapPoint::EraseObservation(LbKeyFrame* kf) {          // src/MapPoint.cc:140-162
  bool bad = false;
  if (observations_.count(kf)) {
    n_observations_--;
    observations_.erase(kf);
    if (reference_keyframe_ == kf && !observations_.empty()) reference_keyframe_ = observations_.begin()->first;      // (the stated departure: it stays when none is left)
    if (n_observations_ <= 2) bad = true;
  }
  if (bad) SetBadFlag();
}
inline void LbMapPoint::SetBadFlag() {                              // :174-188 (map_->EraseMapPoint stays with the caller)
  is_bad_ = true;
  std::map<LbKeyFrame*, size_t> obs = observations_;
  observations_.clear();
  for (auto& o : obs) o.first->EraseMapPointMatch(o.second);
}
inline void LbMapPoint::UpdateNormalAndDepth() {                    // :335-378
  if (is_bad_) return;
  std::map<LbKeyFrame*, size_t> observations = observations_;
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

struct LbMap { std::mutex mutex_map_update_; };

struct LbTypes {
  typedef mock::Frame Frame; typedef LbKeyFrame KeyFrame; typedef LbMapPoint MapPoint; typedef LbMap Map;
  typedef mock::Matrix3d Matrix3d; typedef mock::Matrix4d Matrix4d; typedef mock::Vector3d Vector3d; typedef mock::Sim3d Sim3;
};

// the flat problem of src/CeresOptimizer.cc:346-406 and :423-506, as the library's callers hold it
struct LbProblem {
  std::vector<LbKeyFrame*> cams, local_kfs; std::vector<LbMapPoint*> pts; std::vector<std::pair<LbKeyFrame*, LbMapPoint*> > edges;
  std::vector<double> K4, poses7, pts3, obs_uv; std::vector<float> obs_isg; std::vector<int32_t> obs_cam, obs_pt; std::vector<uint8_t> cam_fixed, cam_local;
};

inline void AssembleHost(LbKeyFrame* keyframe, LbProblem* P) {
  std::map<LbKeyFrame*, int> cam_of;
  auto add_local = [&](LbKeyFrame* kf) { if (!cam_of.count(kf)) { cam_of[kf] = -1; P->local_kfs.push_back(kf); } };
  add_local(keyframe);
  keyframe->n_BA_local_for_keyframe_ = keyframe->id_;
  for (LbKeyFrame* nb : keyframe->GetVectorCovisibleKeyFrames()) {
    nb->n_BA_local_for_keyframe_ = keyframe->id_;
    if (!nb->isBad()) add_local(nb);
  }
  std::map<LbMapPoint*, int> pt_of;
  for (LbKeyFrame* kf : P->local_kfs)
    for (LbMapPoint* mp : kf->GetMapPointMatches())
      if (mp && !mp->isBad() && mp->n_BA_local_for_keyframe_ != keyframe->id_) { pt_of[mp] = -1; mp->n_BA_local_for_keyframe_ = keyframe->id_; }
  std::map<LbKeyFrame*, int> fixed;
  for (auto& it : pt_of)
    for (auto& ob : it.first->GetObservations()) {
      LbKeyFrame* kf = ob.first;
      if (kf->n_BA_local_for_keyframe_ != keyframe->id_ && kf->n_BA_fixed_for_keyframe_ != keyframe->id_) {
        kf->n_BA_fixed_for_keyframe_ = keyframe->id_;
        if (!kf->isBad()) fixed[kf] = -1;
      }
    }
  auto push_cam = [&](LbKeyFrame* kf, bool local) {
    double T[16], p7[7];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[4 * r + c] = kf->Tcw_(r, c);
    ba_matrix4d_to_pose7(T, p7);
    cam_of[kf] = (int)P->cams.size(); P->cams.push_back(kf);
    P->poses7.insert(P->poses7.end(), p7, p7 + 7);
    const double k4[4] = {kf->fx_, kf->fy_, kf->cx_, kf->cy_};
    P->K4.insert(P->K4.end(), k4, k4 + 4);
    P->cam_local.push_back(local ? 1 : 0);
    P->cam_fixed.push_back((!local || kf->id_ == 0) ? 1 : 0);
  };
  std::vector<LbKeyFrame*> by_id(P->local_kfs);
  std::stable_sort(by_id.begin(), by_id.end(), [](const LbKeyFrame* a, const LbKeyFrame* b) { return a->id_ < b->id_; });
  for (LbKeyFrame* kf : by_id) push_cam(kf, true);
  for (auto& it : fixed) push_cam(it.first, false);
  for (auto& it : pt_of) {
    LbMapPoint* mp = it.first;
    it.second = (int)P->pts.size(); P->pts.push_back(mp);
    for (int k = 0; k < 3; k++) P->pts3.push_back(mp->world_pose_[k]);
    for (auto& ob : mp->GetObservations()) {
      LbKeyFrame* kf = ob.first;
      if (kf->isBad()) continue;
      auto c = cam_of.find(kf);
      if (c == cam_of.end() || c->second < 0) continue;
      const KeyPoint& kp = kf->undistort_keypoints_[ob.second];
      P->obs_cam.push_back(c->second); P->obs_pt.push_back(it.second);
      P->obs_uv.push_back(kp.pt.x); P->obs_uv.push_back(kp.pt.y);
      P->obs_isg.push_back(kf->inv_level_sigma2s_[kp.octave]);
      P->edges.push_back(std::make_pair(kf, mp));
    }
  }
}

// src/CeresOptimizer.cc:573-598 with the solver's poses7, pts3 and erase flags
inline void ApplyHost(LbProblem* P, const double* poses7, const double* pts3, const uint8_t* erase) {
  for (size_t i = 0; i < P->edges.size(); i++)
    if (erase[i]) { P->edges[i].first->EraseMapPointMatch(P->edges[i].second); P->edges[i].second->EraseObservation(P->edges[i].first); }
  for (size_t c = 0; c < P->cams.size(); c++) {
    if (!P->cam_local[c]) continue;
    double T[16];
    ba_pose7_to_matrix4d(poses7 + 7 * c, T);
    Matrix4d M;
    for (int r = 0; r < 4; r++) for (int q = 0; q < 4; q++) M(r, q) = T[4 * r + q];
    P->cams[c]->SetPose(M);
  }
  for (size_t p = 0; p < P->pts.size(); p++) {
    P->pts[p]->SetWorldPos(Vector3d(pts3[3 * p], pts3[3 * p + 1], pts3[3 * p + 2]));
    P->pts[p]->UpdateNormalAndDepth();
  }
}

}  // namespace mock
