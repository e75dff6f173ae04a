// Compile-only check of the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch of csrc/compat/orbslam_sim3solver.h.  The reference's
// headers, Eigen and DBoW2 are not in this image, so the NAMES the branch refers to - ORB_SLAM2::KeyFrame, ORB_SLAM2::MapPoint,
// Eigen::Matrix3d / Vector3d / Matrix4d, DUtils::Random - are bound here to the mock data model of tests/cpp/mock_orbslam.h and to a
// declaration of DUtils::Random::RandomInt, and the class template is instantiated.  This checks spelling and types of OUR header; it
// is not a build of the reference.
//   g++ -std=c++17 -fsyntax-only -I include -I tests/cpp tests/cpp/test_sim3solver_reference_types.cpp
#include "mock_orbslam.h"

namespace ORB_SLAM2 { typedef mock::KeyFrame KeyFrame; typedef mock::MapPoint MapPoint; }
namespace Eigen { typedef mock::Matrix3d Matrix3d; typedef mock::Vector3d Vector3d; typedef mock::Matrix4d Matrix4d; }
namespace DUtils { struct Random { static int RandomInt(int min, int max); }; }

#define ORBSLAM_DROPIN_REFERENCE_TYPES
#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_sim3solver.h"

template class ORB_SLAM2::Sim3SolverT<ORB_SLAM2::Sim3SolverReferenceTypes, DUtils::Random>;

int main() {
  ORB_SLAM2::KeyFrame current_keyframe, keyframe;
  std::vector<ORB_SLAM2::MapPoint*> matches;
  bool is_fix_scale = false;
  ORB_SLAM2::Sim3Solver* pSolver = new ORB_SLAM2::Sim3Solver(&current_keyframe, &keyframe, matches, is_fix_scale);   // src/LoopClosing.cc:269
  pSolver->SetRansacParameters(0.99, 20, 300);                                                                      // :272
  std::vector<bool> is_inliers; int n_inliers; bool is_no_more;
  Eigen::Matrix4d Scm = pSolver->iterate(5, is_no_more, is_inliers, n_inliers);                                      // :297
  Eigen::Matrix3d R = pSolver->GetEstimatedRotation();                                                               // :315-317
  Eigen::Vector3d t = pSolver->GetEstimatedTranslation();
  double s = pSolver->GetEstimatedScale();
  Eigen::Matrix4d T2 = pSolver->find(is_inliers, n_inliers);
  delete pSolver;
  return Scm(0, 0) == T2(0, 0) && R(0, 0) == 1.0 && t[0] == 0.0 && s == 1.0 ? 0 : 1;
}
