// Drop-in case of FrameOpsT::SetBadFlags (csrc/compat/orbslam_dropin.h; HIP library underneath) over the mock data model of
// tests/cpp/mock_badflag.h: two copies of one map (BfScene::build with one seed, the keyframes shuffled in memory so that pointer order
// is not index order).  On one the mock's reference-shaped SetBadFlag() runs on the targets one after the other; on the other the
// drop-in's single library call.  Afterwards the WHOLE map state must be equal: every keyframe's map, ordered lists, parent, children,
// bad and to-be-erased flags, Tcp (to the bit) and slots, every point's observations, count, reference keyframe and bad flag, and what
// was erased from the map and the keyframe database.  Then a keyframe listed twice (-1, nothing changed).
// Prints "OK <keyframes gone> <points turned bad> <keyframes re-parented>" on success; with the argument `host` only the host loop runs
// (no library call) and its own counts are printed as "HOST <...> <...> <...>".
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_badflag_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
// With arguments `time <n_kf> <n_targets> <points per keyframe>`: builds a map of that size (compile with -O2), times the host loop and
// the drop-in call (flattening + packed upload + kernels + download + write-back) on fresh copies, checks them equal, and prints
// "TIME host_loop_ms <x> dropin_ms <y>" (the medians of `reps` runs, default 5: `time <n_kf> <n_targets> <per_kf> <reps>`).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_badflag.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;

// the whole state of map A equals that of map B (same shape, compared by index)
struct BfCompare {
  static int pt_index(BfScene& S, const BfMapPoint* p) { return p ? (int)(p - S.mps.data()) : -1; }
  static bool same(BfScene& A, BfScene& B, const char* what) {
    const int n = (int)A.place.size();
    for (int i = 0; i < n; i++) {
      BfKeyFrame &a = A.kf(i), &b = B.kf(i);
      std::map<int, int> wa, wb;
      for (auto& w : a.connected_keyframe_weights_) wa[A.index_of(w.first)] = w.second;
      for (auto& w : b.connected_keyframe_weights_) wb[B.index_of(w.first)] = w.second;
      if (wa != wb) { std::printf("FAIL %s: map of keyframe %d (%zu vs %zu entries)\n", what, i, wa.size(), wb.size()); return false; }
      if (a.ordered_weights_ != b.ordered_weights_ || a.ordered_connected_keyframes_.size() != b.ordered_connected_keyframes_.size() ||
          a.ordered_weights_.size() != a.ordered_connected_keyframes_.size()) { std::printf("FAIL %s: ordered weights of keyframe %d\n", what, i); return false; }
      for (size_t j = 0; j < a.ordered_connected_keyframes_.size(); j++)
        if (A.index_of(a.ordered_connected_keyframes_[j]) != B.index_of(b.ordered_connected_keyframes_[j])) { std::printf("FAIL %s: ordered list of keyframe %d at %zu\n", what, i, j); return false; }
      if ((a.parent_ ? A.index_of(a.parent_) : -1) != (b.parent_ ? B.index_of(b.parent_) : -1)) { std::printf("FAIL %s: parent of keyframe %d\n", what, i); return false; }
      std::set<int> ca, cb;
      for (BfKeyFrame* c : a.childrens_) ca.insert(A.index_of(c));
      for (BfKeyFrame* c : b.childrens_) cb.insert(B.index_of(c));
      if (ca != cb) { std::printf("FAIL %s: children of keyframe %d\n", what, i); return false; }
      if (a.is_bad_ != b.is_bad_ || a.do_to_be_erased_ != b.do_to_be_erased_) { std::printf("FAIL %s: flags of keyframe %d\n", what, i); return false; }
      if (std::memcmp(a.Tcp_.m, b.Tcp_.m, sizeof(a.Tcp_.m)) != 0) { std::printf("FAIL %s: Tcp of keyframe %d\n", what, i); return false; }
      if (a.map_points_.size() != b.map_points_.size()) { std::printf("FAIL %s: slots of keyframe %d\n", what, i); return false; }
      for (size_t s = 0; s < a.map_points_.size(); s++)
        if (pt_index(A, a.map_points_[s]) != pt_index(B, b.map_points_[s])) { std::printf("FAIL %s: slot %zu of keyframe %d\n", what, s, i); return false; }
      if (A.map.erased_keyframes.count(&a) != B.map.erased_keyframes.count(&b) || A.db.erased.count(&a) != B.db.erased.count(&b)) { std::printf("FAIL %s: erase calls of keyframe %d\n", what, i); return false; }
    }
    for (size_t p = 0; p < A.mps.size(); p++) {
      BfMapPoint &a = A.mps[p], &b = B.mps[p];
      std::map<int, size_t> oa, ob;
      for (auto& o : a.observations_) oa[A.index_of(o.first)] = o.second;
      for (auto& o : b.observations_) ob[B.index_of(o.first)] = o.second;
      if (oa != ob || a.n_observations_ != b.n_observations_ || a.is_bad_ != b.is_bad_ || A.index_of(a.reference_keyframe_) != B.index_of(b.reference_keyframe_) ||
          A.map.erased_points.count(&a) != B.map.erased_points.count(&b)) { std::printf("FAIL %s: point %zu\n", what, p); return false; }
    }
    return true;
  }
  static int bad_points(BfScene& S) { int n = 0; for (BfMapPoint& p : S.mps) n += p.is_bad_; return n; }
  static std::vector<int> parents(BfScene& S) { std::vector<int> v; for (size_t i = 0; i < S.place.size(); i++) v.push_back(S.kf((int)i).parent_ ? S.index_of(S.kf((int)i).parent_) : -1); return v; }
};
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::BfTypes> Ops;

// n_tgt keyframes in a shuffled order; the first has children, and one of them follows it directly
static std::vector<BfKeyFrame*> targets(BfScene& S, int n_tgt, unsigned seed) {
  std::mt19937 rng(seed);
  const int n = (int)S.place.size();
  std::vector<int> order;
  for (int i = 1; i < n; i++) order.push_back(i);
  std::shuffle(order.begin(), order.end(), rng);
  std::vector<BfKeyFrame*> t;
  for (int i : order) {
    if ((int)t.size() >= n_tgt) break;
    BfKeyFrame* k = &S.kf(i);
    if (std::find(t.begin(), t.end(), k) != t.end()) continue;
    t.push_back(k);
    if (t.size() == 1 && (int)t.size() < n_tgt)
      for (int c = 1; c < n; c++)
        if (BfCompare::parents(S)[c] == i) { t.push_back(&S.kf(c)); break; }
  }
  return t;
}

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static int time_mode(int n_kf, int n_tgt, int per_kf, int reps) {
  std::unique_ptr<BfScene> W(new BfScene);
  W->build(5, 16, 40, 3);
  Ops::SetBadFlags(targets(*W, 2, 1));                             // (the first call pays for the runtime's start)
  std::vector<double> host, drop;
  for (int rep = 0; rep < reps; rep++) {
    std::unique_ptr<BfScene> A(new BfScene), B(new BfScene);
    A->build(21, n_kf, per_kf, 4); B->build(21, n_kf, per_kf, 4);
    std::vector<BfKeyFrame*> ta = targets(*A, n_tgt, 3), tb = targets(*B, n_tgt, 3);
    auto t0 = std::chrono::steady_clock::now();
    for (BfKeyFrame* k : tb) k->SetBadFlag();
    host.push_back(ms_since(t0));
    t0 = std::chrono::steady_clock::now();
    Ops::SetBadFlags(ta);
    drop.push_back(ms_since(t0));
    if (!BfCompare::same(*A, *B, "timed")) return 1;
  }
  std::printf("TIME host_loop_ms %.4f dropin_ms %.4f\n", median(host), median(drop));
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 5 && std::string(argv[1]) == "time") return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), argc > 5 ? std::atoi(argv[5]) : 5);
  // 60 keyframes, 9 of them targets in a shuffled order
  std::unique_ptr<BfScene> A(new BfScene), B(new BfScene);
  A->build(8, 60, 60, 3); B->build(8, 60, 60, 3);
  bool shuffled = false;
  for (int i = 0; i + 1 < 60; i++) shuffled |= &A->kf(i) > &A->kf(i + 1);
  if (!shuffled) { std::printf("FAIL the keyframes lie in index order\n"); return 1; }
  if (!BfCompare::same(*A, *B, "before")) return 1;
  const std::vector<int> parents_before = BfCompare::parents(*B);
  std::vector<BfKeyFrame*> ta = targets(*A, 9, 2), tb = targets(*B, 9, 2);
  for (BfKeyFrame* k : tb) k->SetBadFlag();
  const std::vector<int> parents_after = BfCompare::parents(*B);
  int moved = 0;
  for (size_t i = 0; i < parents_after.size(); i++) moved += parents_after[i] != parents_before[i];
  const int gone = (int)B->map.erased_keyframes.size(), bad_points = BfCompare::bad_points(*B);
  if (argc == 2 && std::string(argv[1]) == "host") { std::printf("HOST %d %d %d\n", gone, bad_points, moved); return 0; }
  const int n_bad = Ops::SetBadFlags(ta);
  if (n_bad != gone) { std::printf("FAIL %d keyframes went bad, the host loop removed %d\n", n_bad, gone); return 1; }
  if (!BfCompare::same(*A, *B, "after the list")) return 1;
  // a single keyframe, as a call site that culls one at a time makes it
  for (int i : {11, 27}) {
    if (A->kf(i).isBad()) continue;
    B->kf(i).SetBadFlag();
    std::vector<BfKeyFrame*> one(1, &A->kf(i));
    if (Ops::SetBadFlags(one) < 0) { std::printf("FAIL single keyframe %d refused\n", i); return 1; }
    if (!BfCompare::same(*A, *B, "after a single keyframe")) return 1;
  }
  // a keyframe listed twice: refused, nothing changed
  std::vector<BfKeyFrame*> twice;
  for (int i = 1; i < 60 && twice.size() < 2; i++) if (!A->kf(i).isBad()) twice.push_back(&A->kf(i));
  twice.push_back(twice[0]);
  if (Ops::SetBadFlags(twice) != -1) { std::printf("FAIL a list naming a keyframe twice was accepted\n"); return 1; }
  if (!BfCompare::same(*A, *B, "after the refused list")) return 1;
  std::printf("OK %d %d %d\n", n_bad, bad_points, moved);
  return 0;
}
