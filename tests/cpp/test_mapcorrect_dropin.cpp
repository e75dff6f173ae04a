// Drop-in case of FrameOpsT::PropagateGlobalBA and FrameOpsT::CorrectLoopPoses (csrc/compat/orbslam_dropin.h; HIP library underneath) over
// the mock data model of tests/cpp/mock_mapcorrect.h: two copies of one map (McScene::build with one seed, the keyframes shuffled in
// memory so that pointer order is not index order).  On one the reference-shaped host loops of src/LoopClosing.cc:681-739 and :437-523 run,
// on the other the two drop-in calls.  Afterwards the COMPLETE state must be equal bit for bit: poses, inverse poses and centres,
// positions, normals, depth ranges, corrected_by / corrected_reference, the global_BA_* members, both Sim3 maps and the covisibility
// tables.  Prints "OK <points moved by the write-back> <keyframes the correction reached> <points moved by the loop> <of them contested>";
// with the argument `host` only the host loops run (no library call) and print "HOST" with the same four counts.
//   g++ -O1 -std=c++17 -ffp-contract=off -I include -I tests/cpp tests/cpp/test_mapcorrect_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
// With the arguments `time loop <n_connected> <slots per keyframe> <n_points>` or `time gba <n_keyframes> <n_points> <n_outside>`: builds a
// map of that size (compile with -O2), times the host loop and the drop-in call on fresh copies, checks them equal, and prints
// "TIME host_loop_ms <x> dropin_ms <y>" (the best of five).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_mapcorrect.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;

static const unsigned long LOOP_KF = 77;          // nLoopKF of the global BA

struct McScene {
  std::vector<McKeyFrame> store; std::vector<McMapPoint> mps; std::vector<int> place; McMap map;
  McKeyFrame& kf(int i) { return store[place[i]]; }
  int index_of(const McKeyFrame* k) const { if (!k) return -1; const int at = (int)(k - store.data()); for (size_t i = 0; i < place.size(); i++) if (place[i] == at) return (int)i; return -1; }
  static Matrix4d random_pose(std::mt19937& rng, double spread) {
    std::normal_distribution<double> g(0.0, 1.0);
    double q[4] = {g(rng), g(rng), g(rng), g(rng)};
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    Sim3d S;
    for (int k = 0; k < 4; k++) S.d[k] = q[k] / n;
    for (int k = 0; k < 3; k++) S.d[4 + k] = spread * g(rng);
    return mcm::to_pose(S);
  }
  // n_kf keyframes in a spanning tree under origins 0 and 1 (the parent is one of the six keyframes before), n_out of them created while the
  // BA ran (not flagged), two cut off (erased by their parent; not flagged); n_mp points, each seen by 2-6 keyframes of a window, a tenth in
  // the BA, a few bad, a few corrected by the loop's current keyframe already; null slots and slots naming a point twice
  void build(unsigned seed, int n_kf, int n_mp, int window, int n_out, unsigned long current_id) {
    std::mt19937 rng(seed);
    store = std::vector<McKeyFrame>(n_kf); place.resize(n_kf);
    for (int i = 0; i < n_kf; i++) place[i] = i;
    std::shuffle(place.begin(), place.end(), rng);
    std::vector<float> sf(8);
    for (int l = 0; l < 8; l++) sf[l] = (float)std::pow(1.2, l);
    for (int i = 0; i < n_kf; i++) {
      McKeyFrame& k = kf(i);
      k.id_ = (unsigned long)i; k.scale_factors_ = sf; k.n_scale_levels_ = 8;
      k.SetPose(random_pose(rng, 3.0));
      k.global_BA_Tcw_ = random_pose(rng, 3.0);
      k.n_BA_global_for_keyframe_ = LOOP_KF;
      if (i >= 2) kf(std::max(0, i - 1 - (int)(rng() % 6))).AddChildForTest(&k);
      map.keyframes_.push_back(&k);
    }
    map.keyframe_origins_ = {&kf(0), &kf(1)};
    kf(1).is_first_connection_ = false;                                                   // (an origin takes no parent: only keyframe 0 is exempt by its id)
    for (int j = 0; j < n_out; j++) kf(2 + (int)(rng() % (n_kf - 2))).n_BA_global_for_keyframe_ = 0;
    for (int j = 0; j < 3; j++) kf(n_kf - 1 - 2 * j).n_BA_global_for_keyframe_ = 0;       // (with the cut below: a run outside the BA that is and one that is not reached)
    for (int i : {n_kf / 2, n_kf - 3}) {                                                  // erased by its parent
      McKeyFrame& k = kf(i);
      k.parent_->childrens_.erase(&k); k.parent_ = nullptr;
      std::vector<McKeyFrame*> sub(1, &k);                                                 // (nothing below it was in the BA either: a flagged keyframe the
      for (size_t j = 0; j < sub.size(); j++) {                                            //  walk does not reach is the one stated departure, kept out here)
        sub[j]->n_BA_global_for_keyframe_ = 0;
        for (McKeyFrame* c : sub[j]->childrens_) sub.push_back(c);
      }
    }
    mps = std::vector<McMapPoint>(n_mp);
    std::uniform_real_distribution<double> u(-10.0, 10.0);
    auto see = [&](int k, int p) {
      McKeyFrame& K = kf(k);
      K.map_points_.push_back(&mps[p]);
      KeyPoint kp; kp.octave = (int)(rng() % 8);
      K.undistort_keypoints_.resize(K.map_points_.size()); K.undistort_keypoints_.back() = kp;
      mps[p].observations_[&K] = K.map_points_.size() - 1;
    };
    for (int p = 0; p < n_mp; p++) {
      McMapPoint& m = mps[p];
      m.world_pose_ = Vector3d(u(rng), u(rng), u(rng)); m.global_BA_pose_ = Vector3d(u(rng), u(rng), u(rng));
      m.normal_vector_ = Vector3d(-7, -7, -7); m.min_distance_ = -7; m.max_distance_ = -7;
      const int c = (int)(rng() % n_kf), lo = std::max(0, c - window), hi = std::min(n_kf, c + window + 1);
      std::vector<int> cand;
      for (int k = lo; k < hi; k++) cand.push_back(k);
      std::shuffle(cand.begin(), cand.end(), rng);
      const int n = std::min((int)cand.size(), 2 + (int)(rng() % 5));
      for (int j = 0; j < n; j++) {
        if (rng() % 8 == 0) { McKeyFrame& K = kf(cand[j]); K.map_points_.push_back(nullptr); K.undistort_keypoints_.resize(K.map_points_.size()); }
        see(cand[j], p);
      }
      m.reference_keyframe_ = &kf(cand[rng() % n]);
      if (rng() % 10 == 0) m.n_BA_global_for_keyframe_ = LOOP_KF;
      if (rng() % 30 == 0) m.is_bad_ = true;
      if (rng() % 25 == 0) m.corrected_by_keyframe_ = current_id;
      map.map_points_.push_back(&m);
    }
    for (int i = 0; i < n_kf; i += 4) {                                                   // slots naming a point twice
      McKeyFrame& K = kf(i);
      const size_t n = K.map_points_.size();
      for (size_t s = 0; s < n; s += 9) if (K.map_points_[s]) { K.map_points_.push_back(K.map_points_[s]); K.undistort_keypoints_.push_back(K.undistort_keypoints_[s]); }
    }
    for (int i = 0; i < n_kf; i++) kf(i).UpdateConnections();                             // (the covisibility tables of a consistent map)
  }
};

static bool bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

struct McCompare {
  static bool same(McScene& A, McScene& B, const char* what) {
    const int n = (int)A.place.size();
    for (int i = 0; i < n; i++) {
      McKeyFrame &a = A.kf(i), &b = B.kf(i);
      if (!bits(a.Tcw_.m, b.Tcw_.m, 128) || !bits(a.Twc_.m, b.Twc_.m, 128) || !bits(a.Ow_.v, b.Ow_.v, 24)) { std::printf("FAIL %s: pose of keyframe %d\n", what, i); return false; }
      if (!bits(a.global_BA_Tcw_.m, b.global_BA_Tcw_.m, 128) || !bits(a.global_BA_Bef_Tcw_.m, b.global_BA_Bef_Tcw_.m, 128) ||
          a.n_BA_global_for_keyframe_ != b.n_BA_global_for_keyframe_) { std::printf("FAIL %s: global BA members of keyframe %d\n", what, i); return false; }
      std::map<int, int> wa, wb;
      for (auto& w : a.connected_keyframe_weights_) wa[A.index_of(w.first)] = w.second;
      for (auto& w : b.connected_keyframe_weights_) wb[B.index_of(w.first)] = w.second;
      if (wa != wb || a.ordered_weights_ != b.ordered_weights_ || a.ordered_connected_keyframes_.size() != b.ordered_connected_keyframes_.size()) {
        std::printf("FAIL %s: connections of keyframe %d\n", what, i); return false;
      }
      for (size_t j = 0; j < a.ordered_connected_keyframes_.size(); j++)
        if (A.index_of(a.ordered_connected_keyframes_[j]) != B.index_of(b.ordered_connected_keyframes_[j])) { std::printf("FAIL %s: ordered list of keyframe %d\n", what, i); return false; }
      if (A.index_of(a.parent_) != B.index_of(b.parent_) || a.is_first_connection_ != b.is_first_connection_) { std::printf("FAIL %s: parent of keyframe %d\n", what, i); return false; }
      std::set<int> ca, cb;
      for (McKeyFrame* c : a.childrens_) ca.insert(A.index_of(c));
      for (McKeyFrame* c : b.childrens_) cb.insert(B.index_of(c));
      if (ca != cb) { std::printf("FAIL %s: children of keyframe %d\n", what, i); return false; }
    }
    for (size_t p = 0; p < A.mps.size(); p++) {
      McMapPoint &a = A.mps[p], &b = B.mps[p];
      if (!bits(a.world_pose_.v, b.world_pose_.v, 24)) { std::printf("FAIL %s: position of point %zu (%.17g %.17g)\n", what, p, a.world_pose_[0], b.world_pose_[0]); return false; }
      if (!bits(a.normal_vector_.v, b.normal_vector_.v, 24) || !bits(&a.min_distance_, &b.min_distance_, 4) || !bits(&a.max_distance_, &b.max_distance_, 4)) {
        std::printf("FAIL %s: normal / depth of point %zu\n", what, p); return false;
      }
      if (a.corrected_by_keyframe_ != b.corrected_by_keyframe_ || a.corrected_reference_ != b.corrected_reference_) { std::printf("FAIL %s: stamps of point %zu\n", what, p); return false; }
    }
    return true;
  }
  static bool same_sim3(McScene& A, McKeyFrameAndSim3& sa, McScene& B, McKeyFrameAndSim3& sb, const char* what) {
    if (sa.size() != sb.size()) { std::printf("FAIL %s: %zu vs %zu entries\n", what, sa.size(), sb.size()); return false; }
    auto ia = sa.begin(); auto ib = sb.begin();                      // (each map in ITS iteration order: the pointer orders of the two copies agree)
    for (; ia != sa.end(); ++ia, ++ib)
      if (A.index_of(ia->first) != B.index_of(ib->first) || !bits(ia->second.d, ib->second.d, 56)) { std::printf("FAIL %s: entry of keyframe %d\n", what, A.index_of(ia->first)); return false; }
    return true;
  }
};
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::McTypes> Ops;

struct Counts { int gba_points = 0, gba_reached = 0, loop_points = 0, loop_contested = 0; };

static Sim3d loop_scw() {
  Sim3d S;
  const double q[4] = {0.05, -0.08, 0.03, 1.0}, s = std::sqrt(1.03 / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]));
  for (int k = 0; k < 4; k++) S.d[k] = q[k] * s;
  S.d[4] = 0.4; S.d[5] = -0.7; S.d[6] = 0.2;
  return S;
}

// current_connected_keyframes_ of keyframe `cur`: its covisible keyframes in their order, then itself (src/LoopClosing.cc:431-433)
static std::vector<McKeyFrame*> group_of(McScene& S, int cur) {
  std::vector<McKeyFrame*> g = S.kf(cur).GetVectorCovisibleKeyFrames();
  g.push_back(&S.kf(cur));
  return g;
}

static void count_state(McScene& S, int cur, const std::vector<McKeyFrame*>& group, const std::vector<Vector3d>& before, Counts* c, bool loop) {
  if (!loop) {
    for (size_t p = 0; p < S.mps.size(); p++) c->gba_points += !bits(S.mps[p].world_pose_.v, before[p].v, 24);
    for (McKeyFrame& k : S.store) c->gba_reached += bits(k.Tcw_.m, k.global_BA_Tcw_.m, 128);
    return;
  }
  for (size_t p = 0; p < S.mps.size(); p++) {
    if (bits(S.mps[p].world_pose_.v, before[p].v, 24)) continue;
    c->loop_points++;
    int holders = 0;
    for (McKeyFrame* k : group) holders += std::find(k->map_points_.begin(), k->map_points_.end(), &S.mps[p]) != k->map_points_.end();
    c->loop_contested += holders >= 2;
  }
  (void)cur;
}

static std::vector<Vector3d> positions(McScene& S) { std::vector<Vector3d> x; for (McMapPoint& m : S.mps) x.push_back(m.world_pose_); return x; }

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

static int time_mode(const std::string& which, int a1, int a2, int a3) {
  { std::unique_ptr<McScene> W(new McScene); W->build(5, 16, 200, 3, 3, 9); Ops::PropagateGlobalBA(&W->map, LOOP_KF); }      // (the first call pays for the runtime's start)
  double best_host = 1e30, best_drop = 1e30;
  for (int rep = 0; rep < 5; rep++) {
    std::unique_ptr<McScene> A(new McScene), B(new McScene);
    if (which == "gba") {
      A->build(21, a1, a2, 4, a3, 1u << 30); B->build(21, a1, a2, 4, a3, 1u << 30);
      auto t0 = std::chrono::steady_clock::now();
      PropagateGlobalBAHost(&B->map, LOOP_KF);
      best_host = std::min(best_host, ms_since(t0));
      t0 = std::chrono::steady_clock::now();
      Ops::PropagateGlobalBA(&A->map, LOOP_KF);
      best_drop = std::min(best_drop, ms_since(t0));
      if (!McCompare::same(*A, *B, "timed write-back")) return 1;
    } else {
      // a1 connected keyframes of about a2 slots each over a3 points: with four observers per point on average, a3 * 4 / a2 keyframes; the
      // group is the a1 - 1 keyframes around the current one, then the current one
      const int n_kf = std::max(a3 * 4 / std::max(a2, 1), a1 + 8), cur = n_kf / 2;
      A->build(22, n_kf, a3, a1 / 2, 3, (unsigned long)cur); B->build(22, n_kf, a3, a1 / 2, 3, (unsigned long)cur);
      std::vector<McKeyFrame*> ga, gb;
      for (int i = cur - a1 / 2; i < cur - a1 / 2 + a1; i++) if (i != cur) { ga.push_back(&A->kf(i)); gb.push_back(&B->kf(i)); }
      ga.resize(a1 - 1); gb.resize(a1 - 1);
      ga.push_back(&A->kf(cur)); gb.push_back(&B->kf(cur));
      McKeyFrameAndSim3 ca, na, cb, nb;
      auto t0 = std::chrono::steady_clock::now();
      CorrectLoopHost(&B->kf(cur), gb, loop_scw(), cb, nb);
      best_host = std::min(best_host, ms_since(t0));
      t0 = std::chrono::steady_clock::now();
      Ops::CorrectLoopPoses(&A->kf(cur), ga, loop_scw(), ca, na);
      best_drop = std::min(best_drop, ms_since(t0));
      if (!McCompare::same(*A, *B, "timed correction")) return 1;
    }
  }
  std::printf("TIME host_loop_ms %.3f dropin_ms %.3f\n", best_host, best_drop);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && std::string(argv[1]) == "time") return time_mode(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
  const bool host_only = argc == 2 && std::string(argv[1]) == "host";
  const int n_kf = 48, cur = 20;
  std::unique_ptr<McScene> A(new McScene), B(new McScene);
  A->build(8, n_kf, 1500, 4, 9, (unsigned long)cur); B->build(8, n_kf, 1500, 4, 9, (unsigned long)cur);
  bool shuffled = false;
  for (int i = 0; i + 1 < n_kf; i++) shuffled |= &A->kf(i) > &A->kf(i + 1);
  if (!shuffled) { std::printf("FAIL the keyframes lie in index order\n"); return 1; }
  if (!McCompare::same(*A, *B, "before")) return 1;
  Counts cb, ca;
  // 1. the global-BA write-back
  std::vector<Vector3d> before = positions(*B);
  PropagateGlobalBAHost(&B->map, LOOP_KF);
  count_state(*B, cur, {}, before, &cb, false);
  // 2. CorrectLoop on the moved map
  std::vector<McKeyFrame*> gb = group_of(*B, cur);
  McKeyFrameAndSim3 corr_b, non_b, corr_a, non_a;
  before = positions(*B);
  CorrectLoopHost(&B->kf(cur), gb, loop_scw(), corr_b, non_b);
  count_state(*B, cur, gb, before, &cb, true);
  if (host_only) { std::printf("HOST %d %d %d %d\n", cb.gba_points, cb.gba_reached, cb.loop_points, cb.loop_contested); return 0; }
  before = positions(*A);
  const int moved_gba = Ops::PropagateGlobalBA(&A->map, LOOP_KF);
  count_state(*A, cur, {}, before, &ca, false);
  {
    // (compare the write-back alone against a third copy, so that a difference is reported where it arises)
    std::unique_ptr<McScene> C(new McScene);
    C->build(8, n_kf, 1500, 4, 9, (unsigned long)cur);
    PropagateGlobalBAHost(&C->map, LOOP_KF);
    if (!McCompare::same(*A, *C, "after the write-back")) return 1;
  }
  std::vector<McKeyFrame*> ga = group_of(*A, cur);
  if (ga.size() != gb.size() || ga.size() < 4) { std::printf("FAIL the group has %zu keyframes\n", ga.size()); return 1; }
  before = positions(*A);
  const int moved_loop = Ops::CorrectLoopPoses(&A->kf(cur), ga, loop_scw(), corr_a, non_a);
  count_state(*A, cur, ga, before, &ca, true);
  if (!McCompare::same(*A, *B, "after the correction")) return 1;
  if (!McCompare::same_sim3(*A, corr_a, *B, corr_b, "corrected Sim3") || !McCompare::same_sim3(*A, non_a, *B, non_b, "non-corrected Sim3")) return 1;
  if (moved_loop != cb.loop_points || ca.loop_points != cb.loop_points || ca.gba_points != cb.gba_points || moved_gba < ca.gba_points) {
    std::printf("FAIL counts: drop-in %d / %d points, host %d / %d\n", moved_gba, moved_loop, cb.gba_points, cb.loop_points); return 1;
  }
  std::printf("OK %d %d %d %d\n", ca.gba_points, ca.gba_reached, ca.loop_points, ca.loop_contested);
  return 0;
}
