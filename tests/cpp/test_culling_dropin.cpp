// Drop-in case of FrameOpsT::KeyFrameCulling (csrc/compat/orbslam_dropin.h; HIP library underneath) over the mock data model of
// tests/cpp/mock_culling.h: two copies of one consistent map (build_cull_scene with one seed); on one the mock's host
// KeyFrameCulling of the reference's shape runs (src/LocalMapping.cc:576-637), on the other the drop-in's single library call followed
// by SetBadFlag() on the flagged keyframes.  The WHOLE map state must be identical afterwards: bad keyframes, do_to_be_erased_, every
// point's observations, count and bad flag, every keyframe's slots.  Then an inconsistent map (a slot without its observation, an
// observation without its slot): -1 and the map untouched.  Prints "OK <flagged> <kept by do_not_erase_> <bad points>" on success.
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_culling_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <memory>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_culling.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::CullTypes> Ops;

// the state of map A equals the state of map B (same shape, compared by index)
static bool same_state(CullScene& A, CullScene& B, const char* what) {
  for (size_t k = 0; k < A.kfs.size(); k++) {
    CullKeyFrame &a = A.kfs[k], &b = B.kfs[k];
    if (a.is_bad_ != b.is_bad_ || a.do_to_be_erased_ != b.do_to_be_erased_ || a.do_not_erase_ != b.do_not_erase_) { std::printf("FAIL %s: flags of keyframe %zu\n", what, k); return false; }
    if (a.map_points_.size() != b.map_points_.size()) { std::printf("FAIL %s: slot count of keyframe %zu\n", what, k); return false; }
    for (size_t i = 0; i < a.map_points_.size(); i++) {
      const long pa = a.map_points_[i] ? (long)(a.map_points_[i] - A.mps.data()) : -1, pb = b.map_points_[i] ? (long)(b.map_points_[i] - B.mps.data()) : -1;
      if (pa != pb) { std::printf("FAIL %s: slot %zu of keyframe %zu (%ld vs %ld)\n", what, i, k, pa, pb); return false; }
    }
  }
  for (size_t p = 0; p < A.mps.size(); p++) {
    CullMapPoint &a = A.mps[p], &b = B.mps[p];
    if (a.is_bad_ != b.is_bad_ || a.n_observations_ != b.n_observations_ || a.observations_.size() != b.observations_.size()) { std::printf("FAIL %s: point %zu\n", what, p); return false; }
    std::map<long, size_t> oa, ob;
    for (auto& o : a.observations_) oa[(long)(o.first - A.kfs.data())] = o.second;
    for (auto& o : b.observations_) ob[(long)(o.first - B.kfs.data())] = o.second;
    if (oa != ob) { std::printf("FAIL %s: observations of point %zu\n", what, p); return false; }
  }
  return true;
}

int main() {
  // a `small`-sized map: 24 keyframes, 600 points
  std::unique_ptr<CullScene> A(new CullScene), B(new CullScene);
  build_cull_scene(*A, 8, 24, 600, 12, 0.95);
  build_cull_scene(*B, 8, 24, 600, 12, 0.95);
  if (!same_state(*A, *B, "before")) return 1;
  const int flagged_host = KeyFrameCullingHost(&B->kfs.back());
  const int flagged = Ops::KeyFrameCulling(&A->kfs.back());
  if (flagged != flagged_host) { std::printf("FAIL flagged %d, host loop %d\n", flagged, flagged_host); return 1; }
  if (!same_state(*A, *B, "after")) return 1;
  int kept = 0, bad_points = 0, bad_kfs = 0;
  for (CullKeyFrame& k : A->kfs) { kept += k.do_to_be_erased_; bad_kfs += k.is_bad_; }
  for (CullMapPoint& p : A->mps) bad_points += p.is_bad_;
  if (bad_kfs + kept != flagged) { std::printf("FAIL %d bad + %d kept != %d flagged\n", bad_kfs, kept, flagged); return 1; }
  // inconsistent maps: nothing is called, nothing changes
  for (int kind = 0; kind < 3; kind++) {
    std::unique_ptr<CullScene> C(new CullScene), D(new CullScene);
    for (CullScene* S : {C.get(), D.get()}) {
      build_cull_scene(*S, 11, 12, 200, 6, 0.95);
      CullKeyFrame& kf = S->kfs[3];
      size_t i = 0;
      while (!kf.map_points_[i]) i++;
      CullMapPoint* mp = kf.map_points_[i];
      if (kind == 0) { mp->observations_.erase(&kf); }                              // a slot without its observation
      else if (kind == 1) { kf.map_points_[i] = nullptr; }                          // an observation without its slot
      else { mp->observations_[&kf] = i + 1 < kf.map_points_.size() ? i + 1 : i - 1; }   // an observation that names another slot
    }
    if (Ops::KeyFrameCulling(&C->kfs.back()) != -1) { std::printf("FAIL inconsistent map %d accepted\n", kind); return 1; }
    if (!same_state(*C, *D, "inconsistent")) return 1;
  }
  std::printf("OK %d %d %d\n", flagged, kept, bad_points);
  return 0;
}
