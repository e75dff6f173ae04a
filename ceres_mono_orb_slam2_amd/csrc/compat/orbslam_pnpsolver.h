// ============================================================================
// orbslam_pnpsolver.h -- ORB_SLAM2::PnPsolver with the REFERENCE's public surface (reference include/PnPsolver.h: the constructor,
// SetRansacParameters, find, iterate), implemented over orbt_pnp_iterate (include/orbslam_hip.h).  Tracking::Relocalization's
// call sites compile unchanged:
//
//     PnPsolver* pSolver = new PnPsolver(current_frame_, map_point_matches_vector[i]);             // src/Tracking.cc:1025
//     pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);                                   // :1026
//     Eigen::Matrix4d Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);                      // :1047
//
// PnPsolverT<Types, Rng> is a template over a `Types` bundle naming the reference's Frame, MapPoint and Eigen::Matrix4d, and over
// the RNG that draws the minimal sets (DUtils::Random's interface: static RandomInt(int min, int max), inclusive).  The class owns
// what the library leaves to its caller: the compacted correspondences (src/PnPsolver.cc:79-102), mnIterations, the loop bound of
// one iterate call - max(mRansacMaxIts - mnIterations, nIterations), the reference's `||` (:183) - bNoMore and the best-so-far state.
// One iterate call draws exactly the sets that call CAN consume, with the reference's calls in the reference's order (:189-202),
// and advances mnIterations by what the library reports as consumed.  The one visible difference: the sets the reference would NOT
// have drawn (those after an early success) are drawn here, so a seeded reference run is not reproduced draw for draw after the
// first early return; each set is still a uniform draw without replacement.  Inside the reference tree
//     #define ORBSLAM_DROPIN_REFERENCE_TYPES      (before including this header; needs Frame.h, MapPoint.h, Eigen and DUtils/Random.h)
// makes ORB_SLAM2::PnPsolver = PnPsolverT<PnPsolverReferenceTypes, DUtils::Random>.  tests/cpp/ instantiates it over the mock data
// model and a stand-in RNG.  Only element access (r, c) is used on the matrix type; nothing here needs Eigen to compile.
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
class PnPsolverT {
 public:
  typedef typename Types::Frame Frame;
  typedef typename Types::MapPoint MapPoint;
  typedef typename Types::Matrix4d Matrix4d;

  // (:68-111) the non-NULL, non-bad matches, compacted; the world position narrowed to float as the reference's cv::Point3f
  PnPsolverT(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches) : n_matches_(vpMapPointMatches.size()) {
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
      MapPoint* pMP = vpMapPointMatches[i];
      if (!pMP || pMP->isBad()) continue;
      const auto& kp = F.undistort_keypoints_[i];
      p2d_.push_back(kp.pt.x); p2d_.push_back(kp.pt.y);
      sigma2_.push_back(F.level_sigma2s_[kp.octave]);
      const auto Pos = pMP->GetWorldPos();
      p3d_.push_back((float)Pos[0]); p3d_.push_back((float)Pos[1]); p3d_.push_back((float)Pos[2]);
      key_point_indices_.push_back(i);
    }
    K4_[0] = F.fx_; K4_[1] = F.fy_; K4_[2] = F.cx_; K4_[3] = F.cy_;
    best_Tcw_[0] = best_Tcw_[5] = best_Tcw_[10] = best_Tcw_[15] = 1.0;
    SetRansacParameters();
  }

  // (:122-158) minSet other than 4 throws: the reference uses no other value and EPnP on fewer points is undefined
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                           float th2 = 5.991) {
    const int N = (int)sigma2_.size();
    if (orbt_pnp_ransac_params(N, probability, minInliers, maxIterations, minSet, epsilon, &params_) != 0)
      throw std::runtime_error(std::string("orbt_pnp_ransac_params failed: ") + orbhip_last_error());
    max_err_.resize(sigma2_.size());
    for (size_t i = 0; i < sigma2_.size(); i++) max_err_[i] = sigma2_[i] * th2;
    best_mask_.resize(sigma2_.size(), 0);
  }

  Matrix4d find(std::vector<bool>& vbInliers, int& nInliers) {  // (:160-164)
    bool bFlag;
    return iterate(params_.max_iterations, bFlag, vbInliers, nInliers);
  }

  // (:166-261) A library failure (no device, an argument the library refuses) throws std::runtime_error.
  Matrix4d iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    const int N = (int)sigma2_.size();
    if (N < params_.min_inliers) { bNoMore = true; return matrix(nullptr); }     // (:174-178)
    const int n_sets = std::max(params_.max_iterations - iterations_, nIterations);   // (:183) the `||` of the loop condition
    sets_.assign(4 * (size_t)std::max(n_sets, 0), 0);
    std::vector<size_t> vAllIndices((size_t)N), vAvailableIndices;
    for (int i = 0; i < N; i++) vAllIndices[i] = i;
    for (int s = 0; s < n_sets; s++) {                           // (:189-202)
      vAvailableIndices = vAllIndices;
      for (short i = 0; i < 4; ++i) {
        int randi = Rng::RandomInt(0, vAvailableIndices.size() - 1);
        sets_[4 * (size_t)s + i] = (int32_t)vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    std::vector<uint8_t> inl((size_t)N, 0);
    const int rc = orbt_pnp_iterate(p3d_.data(), p2d_.data(), max_err_.data(), N, K4_, params_.min_inliers, sets_.data(), n_sets, &best_count_,
                                    best_mask_.data(), best_Tcw_, &result_, inl.data(), nullptr);
    if (rc != 0) throw std::runtime_error(std::string("orbt_pnp_iterate failed: ") + orbhip_last_error());
    iterations_ += result_.consumed;
    if (result_.status != ORBT_PNP_REFINED) bNoMore = true;      // (:244-246) every set used: mnIterations >= mRansacMaxIts
    if (result_.status != ORBT_PNP_REFINED && result_.status != ORBT_PNP_EXHAUSTED_BEST) return matrix(nullptr);
    nInliers = result_.n_inliers;
    vbInliers = std::vector<bool>(n_matches_, false);            // (:232-237, :250-255)
    for (int i = 0; i < N; i++)
      if (inl[i]) vbInliers[key_point_indices_[i]] = true;
    return matrix(result_.Tcw);
  }

  // not in the reference's interface; for tests and diagnostics
  const std::vector<int32_t>& last_sets() const { return sets_; }
  const orbt_pnp_result& last_result() const { return result_; }
  const orbt_pnp_params& params() const { return params_; }
  int iterations() const { return iterations_; }

 private:
  static Matrix4d matrix(const double* T) {                      // row-major 4 x 4, identity for NULL
    Matrix4d M;
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) M(r, c) = T ? T[4 * r + c] : (r == c ? 1.0 : 0.0);
    return M;
  }
  size_t n_matches_;
  std::vector<float> p3d_, p2d_, sigma2_, max_err_;
  std::vector<size_t> key_point_indices_;
  float K4_[4];
  orbt_pnp_params params_ = {};
  int iterations_ = 0;                                           // mnIterations
  int32_t best_count_ = 0;                                       // mnBestInliers, mvbBestInliers, mBestTcw
  std::vector<uint8_t> best_mask_;
  double best_Tcw_[16] = {};
  std::vector<int32_t> sets_;
  orbt_pnp_result result_ = {};
};

}  // namespace ORB_SLAM2

#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES
// Inside the reference tree (Frame.h, MapPoint.h, Eigen and lib/DBoW2/DUtils/Random.h already included): the class Tracking names.
// src/PnPsolver.cc drops out of the build; include/PnPsolver.h becomes this header plus the define.
namespace ORB_SLAM2 {
struct PnPsolverReferenceTypes {
  typedef ORB_SLAM2::Frame Frame; typedef ORB_SLAM2::MapPoint MapPoint; typedef Eigen::Matrix4d Matrix4d;
};
typedef PnPsolverT<PnPsolverReferenceTypes, DUtils::Random> PnPsolver;
}  // namespace ORB_SLAM2
#endif
