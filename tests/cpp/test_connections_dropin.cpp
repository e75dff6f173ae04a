// Drop-in case of FrameOpsT::UpdateConnections (csrc/compat/orbslam_dropin.h; HIP library underneath) over the mock data model of
// tests/cpp/mock_connections.h: two copies of one map with stale tables (ConnScene::build with one seed, the keyframes shuffled in
// memory so that pointer order is not index order).  On one the host loop of LoopClosing.cc:551-573 runs, with the mock's
// reference-shaped UpdateConnections / AddConnection; on the other the drop-in's single library call.  Afterwards every keyframe's map,
// ordered lists, parent, children and first-connection flag must be equal, and so must loop_connections.  Then a single keyframe as
// the one-element list (the LocalMapping call site), and a keyframe listed twice (-1, nothing changed).
// Prints "OK <keyframes written> <links found> <parents set>" on success; with the argument `host` only the host loop runs (no library
// call) and its own counts are printed as "HOST <keyframes written> <links found> <parents set>".
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_connections_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
// With arguments `time <n_kf> <n_targets> <points per keyframe>`: builds a map of that size (compile with -O2), times the host loop and
// the drop-in call (flattening + packed upload + kernels + download + write-back) on fresh copies, checks them equal, and prints
// "TIME host_loop_ms <x> dropin_ms <y> slots <n>" (the best of five).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_connections.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;

// the covisibility state of map A equals that of map B (same shape, compared by index)
struct ConnCompare {
  static bool same(ConnScene& A, ConnScene& B, const char* what) {
    const int n = (int)A.place.size();
    for (int i = 0; i < n; i++) {
      ConnKeyFrame &a = A.kf(i), &b = B.kf(i);
      std::map<int, int> wa, wb;
      for (auto& w : a.connected_keyframe_weights_) wa[A.index_of(w.first)] = w.second;
      for (auto& w : b.connected_keyframe_weights_) wb[B.index_of(w.first)] = w.second;
      if (wa != wb) { std::printf("FAIL %s: map of keyframe %d (%zu vs %zu entries)\n", what, i, wa.size(), wb.size()); return false; }
      if (a.ordered_weights_ != b.ordered_weights_ || a.ordered_connected_keyframes_.size() != b.ordered_connected_keyframes_.size() ||
          a.ordered_weights_.size() != a.ordered_connected_keyframes_.size()) { std::printf("FAIL %s: ordered weights of keyframe %d\n", what, i); return false; }
      for (size_t j = 0; j < a.ordered_connected_keyframes_.size(); j++)
        if (A.index_of(a.ordered_connected_keyframes_[j]) != B.index_of(b.ordered_connected_keyframes_[j])) { std::printf("FAIL %s: ordered list of keyframe %d at %zu\n", what, i, j); return false; }
      if ((a.parent_ ? A.index_of(a.parent_) : -1) != (b.parent_ ? B.index_of(b.parent_) : -1)) { std::printf("FAIL %s: parent of keyframe %d\n", what, i); return false; }
      if (a.is_first_connection_ != b.is_first_connection_) { std::printf("FAIL %s: first-connection flag of keyframe %d\n", what, i); return false; }
      std::set<int> ca, cb;
      for (ConnKeyFrame* c : a.childrens_) ca.insert(A.index_of(c));
      for (ConnKeyFrame* c : b.childrens_) cb.insert(B.index_of(c));
      if (ca != cb) { std::printf("FAIL %s: children of keyframe %d\n", what, i); return false; }
    }
    return true;
  }
  static int parents(ConnScene& S) { int n = 0; for (ConnKeyFrame& k : S.store) n += k.parent_ != nullptr; return n; }
  static int written(ConnScene& S) { int n = 0; for (ConnKeyFrame& k : S.store) n += k.n_writes_ > 0; return n; }
  static void reset_writes(ConnScene& S) { for (ConnKeyFrame& k : S.store) k.n_writes_ = 0; }
};
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::ConnTypes> Ops;
typedef std::map<ConnKeyFrame*, std::set<ConnKeyFrame*> > Links;

static bool same_links(ConnScene& A, Links& la, ConnScene& B, Links& lb, size_t* total) {
  std::map<int, std::vector<int> > a, b;                          // (each set in ITS iteration order: the pointer orders of the two copies agree)
  for (auto& l : la) for (ConnKeyFrame* k : l.second) a[A.index_of(l.first)].push_back(A.index_of(k));
  for (auto& l : lb) for (ConnKeyFrame* k : l.second) b[B.index_of(l.first)].push_back(B.index_of(k));
  *total = 0;
  for (auto& l : a) *total += l.second.size();
  if (la.size() != lb.size() || a != b) { std::printf("FAIL loop_connections differ\n"); return false; }
  return true;
}

static std::vector<ConnKeyFrame*> targets(ConnScene& S, int n_tgt, unsigned seed) {
  std::mt19937 rng(seed);
  const int n = (int)S.place.size();
  std::vector<int> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  std::shuffle(order.begin(), order.end(), rng);
  // the two sparse keyframes and their neighbour always take part
  for (int want : {n - 2, n - 1, 0}) { auto it = std::find(order.begin(), order.end(), want); std::iter_swap(it, order.begin() + (want == 0 ? 2 : n - 1 - want)); }
  std::vector<ConnKeyFrame*> t;
  for (int i = 0; i < n_tgt && i < n; i++) t.push_back(&S.kf(order[i]));
  return t;
}

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

static int time_mode(int n_kf, int n_tgt, int per_kf) {
  std::unique_ptr<ConnScene> W(new ConnScene);
  W->build(5, 16, 40, 3);
  { Links l; Ops::UpdateConnections(targets(*W, 8, 1), &l); }      // (the first call pays for the runtime's start)
  double best_host = 1e30, best_drop = 1e30;
  size_t slots = 0;
  for (int rep = 0; rep < 5; rep++) {
    std::unique_ptr<ConnScene> A(new ConnScene), B(new ConnScene);
    A->build(21, n_kf, per_kf, 4); B->build(21, n_kf, per_kf, 4);
    std::vector<ConnKeyFrame*> ta = targets(*A, n_tgt, 3), tb = targets(*B, n_tgt, 3);
    slots = 0;
    for (ConnKeyFrame* k : ta) slots += k->map_points_.size();
    Links la, lb;
    auto t0 = std::chrono::steady_clock::now();
    UpdateConnectionsHost(tb, lb);
    best_host = std::min(best_host, ms_since(t0));
    t0 = std::chrono::steady_clock::now();
    Ops::UpdateConnections(ta, &la);
    best_drop = std::min(best_drop, ms_since(t0));
    size_t n_links = 0;
    if (!ConnCompare::same(*A, *B, "timed") || !same_links(*A, la, *B, lb, &n_links)) return 1;
  }
  std::printf("TIME host_loop_ms %.3f dropin_ms %.3f slots %zu\n", best_host, best_drop, slots);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "time") return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  // 40 keyframes, 25 of them targets in a shuffled order
  std::unique_ptr<ConnScene> A(new ConnScene), B(new ConnScene);
  A->build(8, 40, 60, 3); B->build(8, 40, 60, 3);
  bool shuffled = false;
  for (int i = 0; i + 1 < 40; i++) shuffled |= &A->kf(i) > &A->kf(i + 1);
  if (!shuffled) { std::printf("FAIL the keyframes lie in index order\n"); return 1; }
  // part of the map has been through UpdateConnections before (true weights beside the stale ones), the same on both copies
  for (int i = 1; i < 40; i += 4) { A->kf(i).UpdateConnections(); B->kf(i).UpdateConnections(); }
  if (!ConnCompare::same(*A, *B, "before")) return 1;
  const int parents_before = ConnCompare::parents(*A);
  std::vector<ConnKeyFrame*> ta = targets(*A, 25, 2), tb = targets(*B, 25, 2);
  Links la, lb;
  ConnCompare::reset_writes(*B);
  UpdateConnectionsHost(tb, lb);
  if (argc == 2 && std::string(argv[1]) == "host") {
    size_t n = 0;
    for (auto& l : lb) n += l.second.size();
    std::printf("HOST %d %zu %d\n", ConnCompare::written(*B), n, ConnCompare::parents(*B) - parents_before);
    return 0;
  }
  const int written = Ops::UpdateConnections(ta, &la);
  if (written != ConnCompare::written(*B)) { std::printf("FAIL %d keyframes written, the host loop wrote %d\n", written, ConnCompare::written(*B)); return 1; }
  if (!ConnCompare::same(*A, *B, "after the list")) return 1;
  size_t n_links = 0;
  if (!same_links(*A, la, *B, lb, &n_links)) return 1;
  const int parents_set = ConnCompare::parents(*A) - parents_before;
  // the LocalMapping call site: one keyframe, no links
  for (int i : {3, 38, 39}) {
    B->kf(i).UpdateConnections();
    std::vector<ConnKeyFrame*> one(1, &A->kf(i));
    if (Ops::UpdateConnections(one) < 0) { std::printf("FAIL single keyframe %d refused\n", i); return 1; }
    if (!ConnCompare::same(*A, *B, "after a single keyframe")) return 1;
  }
  // a keyframe listed twice: refused, nothing changed
  std::vector<ConnKeyFrame*> twice = {&A->kf(5), &A->kf(6), &A->kf(5)};
  if (Ops::UpdateConnections(twice) != -1) { std::printf("FAIL a list naming a keyframe twice was accepted\n"); return 1; }
  if (!ConnCompare::same(*A, *B, "after the refused list")) return 1;
  std::printf("OK %d %zu %d\n", written, n_links, parents_set);
  return 0;
}
