// Compile-only check of the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch of csrc/compat/orbslam_pnpsolver.h.  The reference's
// headers, Eigen and DBoW2 are not in this image, so the NAMES the branch refers to - ORB_SLAM2::Frame, ORB_SLAM2::MapPoint,
// Eigen::Matrix4d, DUtils::Random - are bound here to the mock data model of tests/cpp/mock_orbslam.h and to a declaration of
// DUtils::Random::RandomInt, and the class template is instantiated.  This checks spelling and types of OUR header; it is not a
// build of the reference.
//   g++ -std=c++17 -fsyntax-only -I include -I tests/cpp tests/cpp/test_pnpsolver_reference_types.cpp
#include "mock_orbslam.h"

namespace ORB_SLAM2 { typedef mock::Frame Frame; typedef mock::MapPoint MapPoint; }
namespace Eigen { typedef mock::Matrix4d Matrix4d; }
namespace DUtils { struct Random { static int RandomInt(int min, int max); }; }

#define ORBSLAM_DROPIN_REFERENCE_TYPES
#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_pnpsolver.h"

template class ORB_SLAM2::PnPsolverT<ORB_SLAM2::PnPsolverReferenceTypes, DUtils::Random>;

int main() {
  ORB_SLAM2::Frame current_frame;
  std::vector<ORB_SLAM2::MapPoint*> matches;
  ORB_SLAM2::PnPsolver* pSolver = new ORB_SLAM2::PnPsolver(current_frame, matches);                // src/Tracking.cc:1025
  pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);                                     // :1026
  std::vector<bool> vbInliers; int nInliers; bool bNoMore;
  Eigen::Matrix4d Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);                         // :1047
  Eigen::Matrix4d T2 = pSolver->find(vbInliers, nInliers);
  delete pSolver;
  return Tcw(0, 0) == T2(0, 0) ? 0 : 1;
}
