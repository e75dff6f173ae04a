// Compile-only check of the call site of FrameOpsHip::KeyFrameCulling in the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES` branch of
// csrc/compat/orbslam_dropin.h.  The reference's headers are not in this image, so the NAMES the branch refers to are bound here to the mock
// data model (tests/cpp/mock_culling.h for KeyFrame / MapPoint, tests/cpp/mock_orbslam.h for the rest).  This checks spelling and types of
// OUR header; it is not a build of the reference.
//   g++ -std=c++17 -fsyntax-only -I include -I tests/cpp tests/cpp/test_culling_reference_types.cpp
#include "mock_culling.h"

namespace ORB_SLAM2 {
typedef mock::Frame Frame; typedef mock::CullKeyFrame KeyFrame; typedef mock::CullMapPoint MapPoint; typedef mock::Map Map;
struct LoopClosing { typedef std::map<KeyFrame*, mock::Sim3d> KeyFrameAndSim3; };
}  // namespace ORB_SLAM2
namespace Eigen { typedef mock::Matrix3d Matrix3d; typedef mock::Matrix4d Matrix4d; typedef mock::Vector2d Vector2d; typedef mock::Vector3d Vector3d; typedef mock::Quaterniond Quaterniond; }
namespace cv { typedef mock::Mat Mat; typedef mock::Point2f Point2f; }
namespace Sophus { typedef mock::Sim3d Sim3d; }

#define ORBSLAM_DROPIN_REFERENCE_TYPES
#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"

int main() {
  ORB_SLAM2::KeyFrame* current_keyframe_ = new ORB_SLAM2::KeyFrame;
  const int n = ORB_SLAM2::FrameOpsHip::KeyFrameCulling(current_keyframe_);               // the body of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:576-637)
  delete current_keyframe_;
  return n;
}
