// Drop-in case of FrameOpsT::UpdateLocalKeyFrames / UpdateLocalPoints (csrc/compat/orbslam_dropin.h; HIP library underneath) over the
// mock data model of tests/cpp/mock_localmap.h.  On ONE map (pointer order must be the same for both runs) the host loops of the
// reference's shape run first - over a real std::map<KeyFrame*, int> and the real std::set<KeyFrame*> of GetChilds() - and their result is
// recorded; the map is put back as it was; then the drop-in's two library calls run.  The lists, reference_keyframe_, the frame's
// cleared slots and EVERY track_reference_for_frame_ of the map must be identical.  Frames: ordinary ones, one that sees nothing (the
// previous list stays), one that sees so much of a long map that more than 80 keyframes are voted.
// Prints "OK <frames> <local keyframes> <local points> <no-vote frames> <over-80 stops> <parent breaks>" on success.
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_local_map_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <memory>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_localmap.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::LmTypes> Ops;

struct Snapshot {
  std::vector<LmKeyFrame*> local; std::vector<LmMapPoint*> points, slots; LmKeyFrame *reference, *frame_reference;
  std::vector<unsigned long> kf_ref, mp_ref;
};
static Snapshot take(LmScene& S, LmFrame& F, const std::vector<LmKeyFrame*>& local, const std::vector<LmMapPoint*>& points, LmKeyFrame* reference) {
  Snapshot s; s.local = local; s.points = points; s.slots = F.map_points_; s.reference = reference; s.frame_reference = F.reference_keyframe_;
  for (LmKeyFrame& k : S.store) s.kf_ref.push_back(k.track_reference_for_frame_);
  for (LmMapPoint& p : S.mps) s.mp_ref.push_back(p.track_reference_for_frame_);
  return s;
}

int main() {
  int frames = 0, sum_kf = 0, sum_pt = 0;
  LmPaths paths;
  struct Case { unsigned seed; int n_kf, n_mp, span, n_slots, centre, window; double hold; };
  const Case cases[] = {{1, 12, 300, 3, 120, 6, 1, 0.7},     {2, 40, 1500, 4, 400, 20, 2, 0.8}, {3, 40, 1500, 4, 400, 3, 4, 0.5}, {4, 30, 800, 3, 200, 10, 2, 0.0},
                        {5, 150, 6000, 5, 1500, 75, 70, 0.9}, {6, 60, 2500, 6, 600, 55, 3, 0.6}, {7, 25, 700, 2, 64, 24, 1, 0.9},  {8, 90, 3000, 4, 900, 40, 38, 0.9}};
  for (const Case& c : cases) {
    std::unique_ptr<LmScene> S(new LmScene);
    build_lm_scene(*S, c.seed, c.n_kf, c.n_mp, c.span, 0.8, 0.06, 0.05);
    LmFrame F; F.id_ = 100 + c.seed;
    build_lm_frame(*S, F, c.seed, c.n_slots, c.centre, c.window, c.hold);
    const std::vector<LmMapPoint*> slots0 = F.map_points_;
    std::vector<LmKeyFrame*> prev;                                  // local_keyframes_ of the frame before, and its reference keyframe
    for (int k = c.n_kf - 1; k >= 0; k -= 3) prev.push_back(S->kf(k));
    LmKeyFrame* ref0 = S->kf(c.n_kf / 2);
    // the host loops
    std::vector<LmKeyFrame*> local = prev; std::vector<LmMapPoint*> points; LmKeyFrame* reference = ref0;
    UpdateLocalKeyFramesHost(F, local, reference, &paths);
    UpdateLocalPointsHost(F, local, points);
    const Snapshot want = take(*S, F, local, points, reference);
    // the map as it was
    for (LmKeyFrame& k : S->store) k.track_reference_for_frame_ = 0;
    for (LmMapPoint& p : S->mps) p.track_reference_for_frame_ = 0;
    F.map_points_ = slots0; F.reference_keyframe_ = nullptr;
    // the drop-in
    local = prev; points.clear(); reference = ref0;
    Ops::UpdateLocalKeyFrames(F, local, reference);
    Ops::UpdateLocalPoints(F, local, points);
    const Snapshot got = take(*S, F, local, points, reference);
    if (got.local != want.local) { std::printf("FAIL case %u: local keyframes (%zu vs %zu)\n", c.seed, got.local.size(), want.local.size()); return 1; }
    if (got.points != want.points) { std::printf("FAIL case %u: local map points (%zu vs %zu)\n", c.seed, got.points.size(), want.points.size()); return 1; }
    if (got.slots != want.slots) { std::printf("FAIL case %u: the frame's slots\n", c.seed); return 1; }
    if (got.reference != want.reference || got.frame_reference != want.frame_reference) { std::printf("FAIL case %u: reference keyframe\n", c.seed); return 1; }
    if (got.kf_ref != want.kf_ref || got.mp_ref != want.mp_ref) { std::printf("FAIL case %u: track_reference_for_frame_\n", c.seed); return 1; }
    frames++; sum_kf += (int)want.local.size(); sum_pt += (int)want.points.size();
  }
  std::printf("OK %d %d %d %d %d %d\n", frames, sum_kf, sum_pt, paths.no_votes, paths.over80, paths.parent_break);
  return 0;
}
