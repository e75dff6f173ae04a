// Compile-only check of the call sites of FrameOpsHip::UpdateLocalKeyFrames / UpdateLocalPoints in the `#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES`
// branch of csrc/compat/orbslam_dropin.h.  The reference's headers are not in this image, so the NAMES the branch refers to are bound here to
// the mock data model (tests/cpp/mock_localmap.h for Frame / KeyFrame / MapPoint, tests/cpp/mock_orbslam.h for the rest).  This checks
// spelling and types of OUR header; it is not a build of the reference.
//   g++ -std=c++17 -fsyntax-only -I include -I tests/cpp tests/cpp/test_local_map_reference_types.cpp
#include "mock_localmap.h"

namespace ORB_SLAM2 {
typedef mock::LmFrame Frame; typedef mock::LmKeyFrame KeyFrame; typedef mock::LmMapPoint MapPoint; typedef mock::Map Map;
struct LoopClosing { typedef std::map<KeyFrame*, mock::Sim3d> KeyFrameAndSim3; };
}  // namespace ORB_SLAM2
namespace Eigen { typedef mock::Matrix3d Matrix3d; typedef mock::Matrix4d Matrix4d; typedef mock::Vector2d Vector2d; typedef mock::Vector3d Vector3d; typedef mock::Quaterniond Quaterniond; }
namespace cv { typedef mock::Mat Mat; typedef mock::Point2f Point2f; }
namespace Sophus { typedef mock::Sim3d Sim3d; }

#define ORBSLAM_DROPIN_REFERENCE_TYPES
#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"

int main() {
  // the members of Tracking the two functions work on (include/Tracking.h)
  ORB_SLAM2::Frame current_frame_;
  std::vector<ORB_SLAM2::KeyFrame*> local_keyframes_;
  std::vector<ORB_SLAM2::MapPoint*> local_map_points_;
  ORB_SLAM2::KeyFrame* reference_keyframe_ = nullptr;
  // the body of Tracking::UpdateLocalMap (src/Tracking.cc:838-845) after map_->SetReferenceMapPoints(local_map_points_)
  ORB_SLAM2::FrameOpsHip::UpdateLocalKeyFrames(current_frame_, local_keyframes_, reference_keyframe_);
  ORB_SLAM2::FrameOpsHip::UpdateLocalPoints(current_frame_, local_keyframes_, local_map_points_);
  return (int)local_map_points_.size();
}
