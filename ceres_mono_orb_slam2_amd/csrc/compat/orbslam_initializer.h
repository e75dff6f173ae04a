// ============================================================================
// orbslam_initializer.h -- ORB_SLAM2::Initializer with the REFERENCE's constructor and Initialize signature (reference
// include/Initializer.h:45-55), implemented over orbt_initialize (include/orbslam_hip.h).  Tracking's call sites compile unchanged:
//
//     initializer_ = new Initializer(current_frame_, 1.0, 200);                                    // src/Tracking.cc:399
//     if (initializer_->Initialize(current_frame_, init_matches_, Rcw, tcw, init_P3Ds_, is_triangulated))   // :432
//
// InitializerT<Types, Rng> is a template over a `Types` bundle naming the reference's Frame, Eigen::Matrix3d and Eigen::Vector3d,
// and over the RNG that draws the RANSAC sets.  Rng has DUtils::Random's interface: static SeedRandOnce(int) and static
// RandomInt(int min, int max) (inclusive).  Initialize draws the sets with the same calls in the same order as
// src/Initializer.cc:86-103, then hands everything else - H / F RANSAC, the model choice, ReconstructH / ReconstructF - to the
// library in ONE call.  Inside the reference tree
//     #define ORBSLAM_DROPIN_REFERENCE_TYPES      (before including this header; needs Frame.h, Eigen and DUtils/Random.h)
// makes ORB_SLAM2::Initializer = InitializerT<InitializerReferenceTypes, DUtils::Random>, so an integrated build draws exactly
// the reference's sets.  tests/cpp/ instantiates it over the mock data model and a stand-in RNG.
// The intrinsics come from Frame::fx_, fy_, cx_, cy_ (statics set from the same K as Frame::K_, src/Frame.cc:143).
// Only element access and the 3-argument constructor are used on the math types; nothing here needs Eigen to compile.
// ============================================================================
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/orbslam_hip.h"

namespace ORB_SLAM2 {

template <class Types, class Rng>
class InitializerT {
 public:
  typedef typename Types::Frame Frame;
  typedef typename Types::Matrix3d Matrix3d;
  typedef typename Types::Vector3d Vector3d;

  // (:43-52) the reference frame's undistorted keypoints and the intrinsics
  InitializerT(const Frame& reference_frame, float sigma = 1.0, int iterations = 200) : sigma_(sigma), max_iterations_(iterations) {
    K4_[0] = Frame::fx_; K4_[1] = Frame::fy_; K4_[2] = Frame::cx_; K4_[3] = Frame::cy_;
    kps1_.resize(2 * reference_frame.undistort_keypoints_.size());
    for (size_t i = 0; i < reference_frame.undistort_keypoints_.size(); i++) {
      kps1_[2 * i] = reference_frame.undistort_keypoints_[i].pt.x; kps1_[2 * i + 1] = reference_frame.undistort_keypoints_[i].pt.y;
    }
  }

  // (:54-133) true = a map can be created from R21, t21, vP3D (the rows with is_triangulated) ; false leaves the four outputs alone.
  // A library failure (no device, an argument the library refuses) throws std::runtime_error.
  bool Initialize(const Frame& current_frame, const std::vector<int>& matches, Matrix3d& R21, Vector3d& t21, std::vector<Vector3d>& vP3D,
                  std::vector<bool>& is_triangulated) {
    const int n1 = (int)(kps1_.size() / 2), n2 = (int)current_frame.undistort_keypoints_.size();
    std::vector<float> kps2(2 * (size_t)n2);
    for (int i = 0; i < n2; i++) { kps2[2 * i] = current_frame.undistort_keypoints_[i].pt.x; kps2[2 * i + 1] = current_frame.undistort_keypoints_[i].pt.y; }
    std::vector<int32_t> m12(matches.begin(), matches.end());
    m12.resize((size_t)n1, -1);                                // (matches has the reference frame's size, :66)
    int N = 0;
    for (int i = 0; i < n1; i++) N += m12[i] >= 0;
    if (N < 8) return false;                                   // (no minimal set: the reference's draw would read an empty vector)
    // (:76-103) the minimal sets, drawn with the reference's calls in the reference's order
    std::vector<size_t> vAllIndices, vAvailableIndices;
    vAllIndices.reserve(N);
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    ransac_sets_.assign(8 * (size_t)max_iterations_, 0);
    Rng::SeedRandOnce(0);
    for (int it = 0; it < max_iterations_; it++) {
      vAvailableIndices = vAllIndices;
      for (size_t j = 0; j < 8; j++) {
        int randi = Rng::RandomInt(0, vAvailableIndices.size() - 1);
        int index = vAvailableIndices[randi];
        ransac_sets_[8 * (size_t)it + j] = index;
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    double R[9], t[3];
    std::vector<double> P(3 * (size_t)n1, NAN);                // rows the winning motion accepts are finite (:802)
    std::vector<uint8_t> tri((size_t)n1, 0);
    const int rc = orbt_initialize(kps1_.data(), n1, kps2.data(), n2, m12.data(), K4_, sigma_, max_iterations_, ransac_sets_.data(), R, t, P.data(),
                                   tri.data(), &report_, nullptr);
    if (rc != 0) throw std::runtime_error(std::string("orbt_initialize failed: ") + orbhip_last_error());
    if (report_.reason != ORBT_INIT_OK) return false;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R21(r, c) = R[3 * r + c];
    t21 = Vector3d(t[0], t[1], t[2]);
    vP3D.assign((size_t)n1, Vector3d());                       // (the reference's rows the winner did not accept are default-constructed)
    is_triangulated.assign((size_t)n1, false);
    for (int i = 0; i < n1; i++) {
      if (!std::isnan(P[3 * (size_t)i])) vP3D[i] = Vector3d(P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]);
      is_triangulated[i] = tri[i] != 0;
    }
    return true;
  }

  // what the last Initialize drew and decided (not in the reference's interface; for tests and diagnostics)
  const std::vector<int32_t>& ransac_sets() const { return ransac_sets_; }
  const orbt_init_report& last_report() const { return report_; }

 private:
  std::vector<float> kps1_;
  float K4_[4];
  float sigma_;
  int max_iterations_;
  std::vector<int32_t> ransac_sets_;
  orbt_init_report report_ = {};
};

}  // namespace ORB_SLAM2

#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES
// Inside the reference tree (Frame.h, Eigen and lib/DBoW2/DUtils/Random.h already included): the class Tracking names.
// src/Initializer.cc drops out of the build; include/Initializer.h becomes this header plus the define.
namespace ORB_SLAM2 {
struct InitializerReferenceTypes {
  typedef ORB_SLAM2::Frame Frame; typedef Eigen::Matrix3d Matrix3d; typedef Eigen::Vector3d Vector3d;
};
typedef InitializerT<InitializerReferenceTypes, DUtils::Random> Initializer;
}  // namespace ORB_SLAM2
#endif
