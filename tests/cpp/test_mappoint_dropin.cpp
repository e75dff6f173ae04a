// Drop-in case of FrameOpsT::UpdateMapPoints (csrc/compat/orbslam_dropin.h; HIP library underneath) over the mock data model:
// two copies of the same map state (build_scene with one seed, then the same keyframes and points marked bad); on one the mock's
// own host MapPoint::ComputeDistinctiveDescriptors (tests/cpp/mock_orbslam.h, src/MapPoint.cc:256-315) runs point by point, on the
// other UpdateMapPoints(points, ORBL_MP_DESC) runs once - every descriptor_ must be byte-equal.  Then UpdateMapPoints(points,
// ORBL_MP_NORMAL_DEPTH) against a plain restatement of :335-378 (exact compare).  Prints "OK <points> <changed>" on success.
//   g++ -O1 -std=c++17 -ffp-contract=off -I include -I tests/cpp tests/cpp/test_mappoint_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <memory>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_orbslam.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::Types> Ops;

static void prepare(Scene& S) {
  build_scene(S, 1234, 24, 3000, 1);
  for (size_t k = 0; k < S.kfs.size(); k += 5) S.kfs[k].is_bad_ = true;           // keyframes 0, 5, 10, ...: skipped by the descriptor
  for (size_t p = 0; p < S.mps.size(); p += 37) S.mps[p].is_bad_ = true;
  for (size_t p = 3; p < S.mps.size(); p += 101) S.mps[p].reference_keyframe_ = &S.kfs[(p / 101) % S.kfs.size()];   // (often not in the list)
  for (MapPoint& mp : S.mps) for (auto& b : mp.descriptor_.d) b = 0x5A;            // a value no keyframe row has
}

int main() {
  std::unique_ptr<Scene> A(new Scene), B(new Scene);
  prepare(*A);
  prepare(*B);
  std::vector<MapPoint*> pa, pb;
  for (size_t p = 0; p < A->mps.size(); p++) { pa.push_back(&A->mps[p]); pb.push_back(&B->mps[p]); }
  for (MapPoint* mp : pb) mp->ComputeDistinctiveDescriptors();                      // the mock's host method
  std::vector<MapPoint*> with_null(pa);                                             // (a NULL entry, as GetMapPointMatches() has: skipped)
  with_null.insert(with_null.begin() + 7, nullptr);
  Ops::UpdateMapPoints(with_null, ORBL_MP_DESC);
  int changed = 0, maxn = 0;
  for (size_t p = 0; p < pa.size(); p++) {
    if (pa[p]->descriptor_.d != pb[p]->descriptor_.d) { std::printf("FAIL descriptor of point %zu\n", p); return 1; }
    changed += pa[p]->descriptor_.d[0] != 0x5A || pa[p]->descriptor_.d[1] != 0x5A;
    maxn = std::max(maxn, (int)pa[p]->observations_.size());
  }
  // normal and depth: the restated :335-378 on B, the library on A
  for (MapPoint* mp : pb) {
    if (mp->is_bad_ || mp->observations_.empty()) continue;
    std::map<KeyFrame*, size_t> obs = mp->observations_;
    double n[3] = {0, 0, 0};
    int nobs = 0;                                              // (the reference's counter: obs[ref] below may grow the copy)
    for (auto& o : obs) {
      nobs++;
      const Vector3d v = mp->world_pose_ - o.first->GetCameraCenter();
      const double nn = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
      for (int k = 0; k < 3; k++) n[k] = n[k] + v[k] / nn;
    }
    KeyFrame* ref = mp->reference_keyframe_;
    const Vector3d pc = mp->world_pose_ - ref->GetCameraCenter();
    const float dist = (float)std::sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
    const int level = ref->undistort_keypoints_[obs[ref]].octave;
    mp->max_distance_ = dist * ref->scale_factors_[level];
    mp->min_distance_ = mp->max_distance_ / ref->scale_factors_[ref->n_scale_levels_ - 1];
    mp->normal_vector_ = Vector3d(n[0] / nobs, n[1] / nobs, n[2] / nobs);
  }
  Ops::UpdateMapPoints(pa, ORBL_MP_NORMAL_DEPTH);
  for (size_t p = 0; p < pa.size(); p++) {
    const MapPoint &a = *pa[p], &b = *pb[p];
    if (std::memcmp(&a.max_distance_, &b.max_distance_, 4) || std::memcmp(&a.min_distance_, &b.min_distance_, 4) ||
        std::memcmp(a.normal_vector_.v, b.normal_vector_.v, 24)) { std::printf("FAIL normal / depth of point %zu\n", p); return 1; }
  }
  std::printf("OK %zu %d %d\n", pa.size(), changed, maxn);
  return 0;
}
