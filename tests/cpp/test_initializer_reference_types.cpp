// Compile-only check of the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch of csrc/compat/orbslam_initializer.h.  The reference's
// headers, Eigen and DBoW2 are not in this image, so the NAMES the branch refers to - ORB_SLAM2::Frame, Eigen::Matrix3d /
// Vector3d, DUtils::Random - are bound here to the mock data model of tests/cpp/mock_orbslam.h and to a declaration of
// DUtils::Random's two static members, and the class template is instantiated.  This checks spelling and types of OUR header;
// it is not a build of the reference.
//   g++ -std=c++17 -fsyntax-only -I include -I tests/cpp tests/cpp/test_initializer_reference_types.cpp
#include "mock_orbslam.h"

namespace ORB_SLAM2 { typedef mock::Frame Frame; }
namespace Eigen { typedef mock::Matrix3d Matrix3d; typedef mock::Vector3d Vector3d; }
namespace DUtils { struct Random { static void SeedRandOnce(int seed); static int RandomInt(int min, int max); }; }

#define ORBSLAM_DROPIN_REFERENCE_TYPES
#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_initializer.h"

template class ORB_SLAM2::InitializerT<ORB_SLAM2::InitializerReferenceTypes, DUtils::Random>;

int main() {
  ORB_SLAM2::Frame reference_frame;
  ORB_SLAM2::Initializer* initializer = new ORB_SLAM2::Initializer(reference_frame, 1.0, 200);   // src/Tracking.cc:399
  std::vector<int> init_matches;
  Eigen::Matrix3d Rcw; Eigen::Vector3d tcw; std::vector<Eigen::Vector3d> init_P3Ds; std::vector<bool> is_triangulated;
  bool ok = initializer->Initialize(reference_frame, init_matches, Rcw, tcw, init_P3Ds, is_triangulated);   // :432
  delete initializer;
  return ok ? 0 : 1;
}
