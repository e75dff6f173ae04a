// ============================================================================
// orbslam_sim3solver.h -- ORB_SLAM2::Sim3Solver with the REFERENCE's public surface (reference include/Sim3Solver.h:43-57: the
// constructor, SetRansacParameters, find, iterate, GetEstimatedRotation / Translation / Scale), implemented over orbt_sim3_iterate
// (include/orbslam_hip.h).  LoopClosing::ComputeSim3's call sites compile unchanged:
//
//     Sim3Solver* pSolver = new Sim3Solver(current_keyframe_, keyframe, map_point_matches_vector[i], is_fix_scale_);   // src/LoopClosing.cc:269
//     pSolver->SetRansacParameters(0.99, 20, 300);                                                                     // :272
//     Eigen::Matrix4d Scm = pSolver->iterate(5, is_no_more, is_inliers, n_inliers);                                    // :297
//     Eigen::Matrix3d R = pSolver->GetEstimatedRotation();  ...Translation();  ...Scale();                             // :315-317
//
// Sim3SolverT<Types, Rng> is a template over a `Types` bundle naming the reference's KeyFrame, MapPoint and Eigen's Matrix3d,
// Vector3d, Matrix4d, and over the RNG that draws the minimal sets (DUtils::Random's interface: static RandomInt(int min, int max),
// inclusive).  The class owns what the library leaves to its caller: the compacted correspondences with the constructor's skip rules
// (src/Sim3Solver.cc:73-85) and matched_indices_1_, the truncated thresholds (:93-94), n_iterations_, the loop bound of one iterate
// call - min(ransac_max_iterations_ - n_iterations_, n_iterations), the reference's `&&` (:164-165) - is_no_more (:209) and the
// best-so-far state.  One iterate call draws exactly the sets that call CAN consume, with the reference's calls in the reference's
// order (:169-182), and advances n_iterations_ by what the library reports as consumed.  The one visible difference: the sets the
// reference would NOT have drawn (those after an early success) are drawn here, so a seeded reference run is not reproduced draw for
// draw after the first early return; each set is still a uniform draw without replacement.  Inside the reference tree
//     #define ORBSLAM_DROPIN_REFERENCE_TYPES      (before including this header; needs KeyFrame.h, MapPoint.h, Eigen and DUtils/Random.h)
// makes ORB_SLAM2::Sim3Solver = Sim3SolverT<Sim3SolverReferenceTypes, DUtils::Random>.  tests/cpp/ instantiates it over the mock data
// model and a stand-in RNG.  Only element access - (r, c) on matrices, [i] on vectors - is used; nothing here needs Eigen to compile.
// ============================================================================
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/orbslam_hip.h"

namespace ORB_SLAM2 {

template <class Types, class Rng>
class Sim3SolverT {
 public:
  typedef typename Types::KeyFrame KeyFrame;
  typedef typename Types::MapPoint MapPoint;
  typedef typename Types::Matrix3d Matrix3d;
  typedef typename Types::Vector3d Vector3d;
  typedef typename Types::Matrix4d Matrix4d;

  // (:47-118) the matches with a map point on both sides, neither bad, both observed in their keyframe; camera-frame positions
  Sim3SolverT(KeyFrame* keyframe_1, KeyFrame* keyframe_2, const std::vector<MapPoint*>& matched_points_1_in_2, const bool is_fixed_scale = true)
      : N1_((int)matched_points_1_in_2.size()), is_fixed_scale_(is_fixed_scale) {
    std::vector<MapPoint*> matched_points_in_1 = keyframe_1->GetMapPointMatches();
    const Matrix3d Rcw1 = keyframe_1->GetRotation(), Rcw2 = keyframe_2->GetRotation();
    const Vector3d tcw1 = keyframe_1->GetTranslation(), tcw2 = keyframe_2->GetTranslation();
    for (int i1 = 0; i1 < N1_; i1++) {
      if (!matched_points_1_in_2[i1]) continue;
      MapPoint* map_point_1 = matched_points_in_1[i1];
      MapPoint* map_point_2 = matched_points_1_in_2[i1];
      if (!map_point_1) continue;
      if (map_point_1->isBad() || map_point_2->isBad()) continue;
      const int indexKF1 = map_point_1->GetIndexInKeyFrame(keyframe_1);
      const int indexKF2 = map_point_2->GetIndexInKeyFrame(keyframe_2);
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      const float sigmaSquare1 = keyframe_1->level_sigma2s_[keyframe_1->undistort_keypoints_[indexKF1].octave];
      const float sigmaSquare2 = keyframe_2->level_sigma2s_[keyframe_2->undistort_keypoints_[indexKF2].octave];
      max_err1_.push_back((float)(size_t)(9.210 * sigmaSquare1));   // (:93-94) a std::vector<size_t> in the reference: truncated
      max_err2_.push_back((float)(size_t)(9.210 * sigmaSquare2));
      matched_indices_1_.push_back((size_t)i1);
      push_camera(Rcw1, tcw1, map_point_1->GetWorldPos(), X1c_);
      push_camera(Rcw2, tcw2, map_point_2->GetWorldPos(), X2c_);
    }
    K1_[0] = keyframe_1->fx_; K1_[1] = keyframe_1->fy_; K1_[2] = keyframe_1->cx_; K1_[3] = keyframe_1->cy_;
    K2_[0] = keyframe_2->fx_; K2_[1] = keyframe_2->fy_; K2_[2] = keyframe_2->cx_; K2_[3] = keyframe_2->cy_;
    best_R_[0] = best_R_[4] = best_R_[8] = 1.0;
    SetRansacParameters();
  }

  // (:120-145)
  void SetRansacParameters(double probability = 0.99, int min_inliers = 6, int max_iterations = 300) {
    const int N = (int)matched_indices_1_.size();
    if (orbt_sim3_ransac_params(N, probability, min_inliers, max_iterations, &params_) != 0)
      throw std::runtime_error(std::string("orbt_sim3_ransac_params failed: ") + orbhip_last_error());
    best_mask_.resize((size_t)N, 0);
    n_iterations_ = 0;
  }

  Matrix4d find(std::vector<bool>& vbInliers12, int& n_inliers) {  // (:214-217)
    bool flag;
    return iterate(params_.max_iterations, flag, vbInliers12, n_inliers);
  }

  // (:147-212) A library failure (no device, an argument the library refuses) throws std::runtime_error.
  Matrix4d iterate(int n_iterations, bool& is_no_more, std::vector<bool>& is_inliers, int& n_inliers) {
    is_no_more = false;
    is_inliers = std::vector<bool>((size_t)N1_, false);
    n_inliers = 0;
    const int N = (int)matched_indices_1_.size();
    if (N < params_.min_inliers) { is_no_more = true; return matrix(nullptr); }            // (:153-156)
    const int n_sets = std::max(0, std::min(params_.max_iterations - n_iterations_, n_iterations));   // (:164-165) the `&&` of the loop condition
    sets_.assign(3 * (size_t)n_sets, 0);
    std::vector<size_t> all_indices((size_t)N), available_indices;
    for (int i = 0; i < N; i++) all_indices[i] = i;
    for (int s = 0; s < n_sets; s++) {                           // (:169-182)
      available_indices = all_indices;
      for (short i = 0; i < 3; ++i) {
        int randi = Rng::RandomInt(0, available_indices.size() - 1);
        sets_[3 * (size_t)s + i] = (int32_t)available_indices[randi];
        available_indices[randi] = available_indices.back();
        available_indices.pop_back();
      }
    }
    std::vector<uint8_t> inl((size_t)N, 0);
    const int rc = orbt_sim3_iterate(X1c_.data(), X2c_.data(), max_err1_.data(), max_err2_.data(), N, K1_, K2_, is_fixed_scale_ ? 1 : 0,
                                     params_.min_inliers, sets_.data(), n_sets, &best_count_, best_mask_.data(), best_R_, best_t_, &best_scale_,
                                     &result_, inl.data(), nullptr);
    if (rc != 0) throw std::runtime_error(std::string("orbt_sim3_iterate failed: ") + orbhip_last_error());
    n_iterations_ += result_.consumed;
    if (result_.status == ORBT_SIM3_FOUND) {                     // (:198-205)
      n_inliers = result_.n_inliers;
      for (int i = 0; i < N; i++)
        if (inl[i]) is_inliers[matched_indices_1_[i]] = true;
      return matrix(result_.T12);
    }
    if (n_iterations_ >= params_.max_iterations) is_no_more = true;   // (:209)
    return matrix(nullptr);
  }

  Matrix3d GetEstimatedRotation() {
    Matrix3d R;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R(r, c) = best_R_[3 * r + c];
    return R;
  }
  Vector3d GetEstimatedTranslation() {
    Vector3d t;
    for (int i = 0; i < 3; i++) t[i] = best_t_[i];
    return t;
  }
  float GetEstimatedScale() { return best_scale_; }

  // not in the reference's interface; for tests and diagnostics
  const std::vector<int32_t>& last_sets() const { return sets_; }
  const orbt_sim3_result& last_result() const { return result_; }
  const orbt_sim3_params& params() const { return params_; }
  const std::vector<size_t>& matched_indices() const { return matched_indices_1_; }
  int iterations() const { return n_iterations_; }

 private:
  static void push_camera(const Matrix3d& R, const Vector3d& t, const Vector3d& X, std::vector<double>& out) {   // (:100-104) R X + t
    for (int i = 0; i < 3; i++) out.push_back(((R(i, 0) * X[0] + R(i, 1) * X[1]) + R(i, 2) * X[2]) + t[i]);
  }
  static Matrix4d matrix(const double* T) {                      // row-major 4 x 4, identity for NULL
    Matrix4d M;
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) M(r, c) = T ? T[4 * r + c] : (r == c ? 1.0 : 0.0);
    return M;
  }
  int N1_;
  bool is_fixed_scale_;
  std::vector<double> X1c_, X2c_;
  std::vector<float> max_err1_, max_err2_;
  std::vector<size_t> matched_indices_1_;
  float K1_[4], K2_[4];
  orbt_sim3_params params_ = {};
  int n_iterations_ = 0;
  int32_t best_count_ = 0;                                       // n_best_inliers_, is_best_inliers_, best_rotation_, best_translation_, best_scale_
  std::vector<uint8_t> best_mask_;
  double best_R_[9] = {}, best_t_[3] = {};
  float best_scale_ = 1.0f;
  std::vector<int32_t> sets_;
  orbt_sim3_result result_ = {};
};

}  // namespace ORB_SLAM2

#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES
// Inside the reference tree (KeyFrame.h, MapPoint.h, Eigen and lib/DBoW2/DUtils/Random.h already included): the class LoopClosing
// names.  src/Sim3Solver.cc drops out of the build; include/Sim3Solver.h becomes this header plus the define.
namespace ORB_SLAM2 {
struct Sim3SolverReferenceTypes {
  typedef ORB_SLAM2::KeyFrame KeyFrame; typedef ORB_SLAM2::MapPoint MapPoint;
  typedef Eigen::Matrix3d Matrix3d; typedef Eigen::Vector3d Vector3d; typedef Eigen::Matrix4d Matrix4d;
};
typedef Sim3SolverT<Sim3SolverReferenceTypes, DUtils::Random> Sim3Solver;
}  // namespace ORB_SLAM2
#endif
