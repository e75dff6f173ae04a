// Drop-in case of FrameOpsT::AssembleEssentialGraph, ApplyEssentialGraph and OptimizeEssentialGraph (csrc/compat/orbslam_dropin.h; HIP library
// underneath) over the mock data model of tests/cpp/mock_essgraph.h: two copies of one seeded map whose keyframes and points are shuffled in
// memory, so that pointer order - the order of the reference's std::set / std::map containers - is not id order.
//   1. Copy A runs CeresOptimizerT::OptimizeEssentialGraph, the host graph walk as it stands; copy B runs FrameOpsT::OptimizeEssentialGraph.
//      The class is not touched: this program defines ba_optimize_essential_graph itself, so both calls hand their problem to the recorder
//      below, which answers both with the same synthetic result (every free tangent moved a little).  The two recorded problems must name
//      the same vertices and the same edges in the same order, with the tangents and Sji within 1e-12.
//   2. Both write-backs then got one lie_opt: the complete map state - poses, centres, positions - must agree within 1e-12 (normals to 1e-9,
//      depth ranges to float rounding), and the same points must have been moved.
//   3. mock::Types, a data model without the members these entries read, still instantiates FrameOpsT.
// Prints "OK <vertices> <edges> <loop connection edges> <points moved>".
//   g++ -O1 -std=c++17 -ffp-contract=off -I include -I tests/cpp tests/cpp/test_essgraph_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_essgraph.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
template struct ORB_SLAM2::FrameOpsT<mock::Types>;                  // (3.)

// ---- the recorder: what either caller hands to the solver, and one answer for both
struct Recorded { std::vector<double> lie, S; std::vector<uint8_t> fixed; std::vector<int32_t> ej, ei; };
static std::vector<Recorded> g_calls;
extern "C" int ba_optimize_essential_graph(double* lie7, const uint8_t* kf_fixed, int n_kf, const int32_t* edge_j, const int32_t* edge_i, const double* edge_Sji, int n_edges,
                                           int max_iterations, const volatile uint8_t* stop_flag, ba_summary* summary) {
  (void)max_iterations; (void)stop_flag; (void)summary;
  Recorded r;
  r.lie.assign(lie7, lie7 + 7 * (size_t)n_kf); r.fixed.assign(kf_fixed, kf_fixed + n_kf);
  r.ej.assign(edge_j, edge_j + n_edges); r.ei.assign(edge_i, edge_i + n_edges); r.S.assign(edge_Sji, edge_Sji + 7 * (size_t)n_edges);
  g_calls.push_back(r);
  std::mt19937 rng(99);
  std::normal_distribution<double> G(0.0, 1.0);
  for (int v = 0; v < n_kf; v++)
    for (int q = 0; q < 7; q++) { const double d = G(rng) * (q < 3 ? 0.05 : q < 6 ? 0.01 : 0.02); if (!kf_fixed[v]) lie7[7 * (size_t)v + q] += d; }
  return 0;
}

namespace mock {

static Matrix4d make_pose(double ax, double ay, double az, const Vector3d& t) {
  const double cx = std::cos(ax), sx = std::sin(ax), cy = std::cos(ay), sy = std::sin(ay), cz = std::cos(az), sz = std::sin(az);
  Matrix4d T;
  T(0, 0) = cy * cz; T(0, 1) = sx * sy * cz - cx * sz; T(0, 2) = cx * sy * cz + sx * sz;
  T(1, 0) = cy * sz; T(1, 1) = sx * sy * sz + cx * cz; T(1, 2) = cx * sy * sz - sx * cz;
  T(2, 0) = -sy; T(2, 1) = sx * cy; T(2, 2) = cx * cy;
  for (int i = 0; i < 3; i++) T(i, 3) = t[i];
  return T;
}

struct EgScene {
  std::vector<EgKeyFrame> store; std::vector<EgMapPoint> pstore; std::vector<int> place, pplace; EgMap map;
  std::map<EgKeyFrame*, Sim3d> corrected, non_corrected; std::map<EgKeyFrame*, std::set<EgKeyFrame*> > loop_connections;
  int loop = 0, cur = 0;
  EgKeyFrame& kf(int i) { return store[place[i]]; }
  EgMapPoint& mp(int p) { return pstore[pplace[p]]; }
  // n_kf keyframes on a circle (keyframe i has id i, a chain of parents with a few re-hung, a few bad), ordered lists whose weights straddle
  // 100 or pass it wholly, loop edges, a group of n_group keyframes ending in the current one with corrected Sim3s of scale 0.95-1.05, loop
  // connections with entries below 100, bad entries and the exempt (current, loop) pair; n_mp points, a third already corrected
  void build(unsigned seed, int n_kf, int n_mp, int n_group) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> G(0.0, 1.0);
    store = std::vector<EgKeyFrame>(n_kf); pstore = std::vector<EgMapPoint>(n_mp); place.resize(n_kf); pplace.resize(n_mp);
    for (int i = 0; i < n_kf; i++) place[i] = i;
    for (int p = 0; p < n_mp; p++) pplace[p] = p;
    std::shuffle(place.begin(), place.end(), rng); std::shuffle(pplace.begin(), pplace.end(), rng);
    std::vector<float> sf(8);
    for (int l = 0; l < 8; l++) sf[l] = (float)std::pow(1.2, l);
    loop = 2; cur = n_kf - 1;
    for (int i = 0; i < n_kf; i++) {
      EgKeyFrame& k = kf(i);
      const double a = 6.2831853 * i / n_kf;
      k.id_ = (unsigned long)i; k.scale_factors_ = sf; k.undistort_keypoints_.resize(8);
      for (int s = 0; s < 8; s++) k.undistort_keypoints_[s].octave = (int)(rng() % 8);
      k.SetPose(make_pose(0.3 + 0.1 * G(rng), -a + 0.4, 0.25 + 0.1 * G(rng), Vector3d(20 * std::cos(a) + G(rng), G(rng), 20 * std::sin(a) + 5)));
      k.is_bad_ = i != cur && i != loop && i > 3 && rng() % 12 == 0;
      map.keyframes_.insert(&k);
    }
    for (int i = 1; i < n_kf; i++) {
      const int par = (rng() % 10 == 0 && i > 4) ? i - 3 : i - 1;
      kf(i).parent_ = &kf(par); kf(par).children_.insert(&kf(i));
    }
    for (int e = 0; e < n_kf / 8; e++) {
      const int a = (int)(rng() % n_kf), b = (int)(rng() % n_kf);
      if (a != b) { kf(a).loop_edges_.insert(&kf(b)); kf(b).loop_edges_.insert(&kf(a)); }
    }
    std::vector<std::map<int, int> > w(n_kf);
    const int choices[7] = {15, 40, 99, 100, 101, 130, 250};
    for (int i = 0; i < n_kf; i++)
      for (int c = 0; c < 5; c++) {
        const int j = (int)(rng() % n_kf);
        if (j != i && !w[i].count(j)) { w[i][j] = w[j][i] = choices[rng() % 7]; }
      }
    for (int i = 0; i < n_kf; i += 9) for (auto& e : w[i]) { e.second = std::max(e.second, 100); w[e.first][i] = e.second; }       // lists that pass wholly
    for (int i = 0; i < n_kf; i++) {
      EgKeyFrame& k = kf(i);
      std::vector<std::pair<int, int> > by;
      for (auto& e : w[i]) { k.connected_keyframe_weights_[&kf(e.first)] = e.second; by.push_back(std::make_pair(-e.second, e.first)); }
      std::sort(by.begin(), by.end());
      for (auto& e : by) { k.ordered_connected_keyframes_.push_back(&kf(e.second)); k.ordered_weights_.push_back(-e.first); }
    }
    for (int g = 0; g < n_group; g++) {
      const int i = g == n_group - 1 ? cur : n_kf - 2 - 2 * g;
      EgKeyFrame& k = kf(i);
      if (k.is_bad_) continue;
      double T[16], p7[7];
      for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[4 * r + c] = k.Tcw_(r, c);
      ba_matrix4d_to_pose7(T, p7);
      Sim3d n, c;
      const double s = 0.95 + 0.1 * U(rng), rs = std::sqrt(s);
      for (int q = 0; q < 4; q++) { n.d[q] = p7[3 + q]; c.d[q] = p7[3 + q] * rs; }
      for (int q = 0; q < 3; q++) { n.d[4 + q] = p7[q]; c.d[4 + q] = p7[q] * s + 0.1 * G(rng); }
      non_corrected[&k] = n; corrected[&k] = c;
      std::set<EgKeyFrame*>& links = loop_connections[&k];
      for (int e = 0; e < 4; e++) links.insert(&kf((int)(rng() % n_kf)));
      int t = 0;
      for (auto& e : w[i]) if (t++ < 3) links.insert(&kf(e.first));
      links.erase(&k);
      if (i == cur) links.insert(&kf(loop));
    }
    for (int p = 0; p < n_mp; p++) {
      EgMapPoint& m = mp(p);
      const int r = (int)(rng() % n_kf);
      const Vector3d O = kf(r).GetCameraCenter();
      m.world_pose_ = Vector3d(O[0] + 2 * G(rng), O[1] + 2 * G(rng), O[2] + 6 + 2 * U(rng));
      m.normal_vector_ = Vector3d(-7, -7, -7); m.min_distance_ = -7; m.max_distance_ = -7;
      m.is_bad_ = rng() % 20 == 0;
      const int n_obs = (int)(rng() % 5);
      for (int o = 0; o < n_obs; o++) m.observations_[&kf((r + o * 3) % n_kf)] = (size_t)(rng() % 8);
      if (rng() % 30 != 0) { m.reference_keyframe_ = &kf(r); if (n_obs == 0 && rng() % 2) m.observations_[&kf(r)] = 1; }
      if (!m.reference_keyframe_) m.observations_.clear();
      if (rng() % 3 == 0) { m.corrected_by_keyframe_ = (unsigned long)cur; m.corrected_reference_ = (unsigned long)(n_kf - 2 - 2 * (int)(rng() % (n_group - 1))); }
      map.map_points_.insert(&m);
    }
  }
};

}  // namespace mock

static int fail(const char* what, long at = -1, double a = 0, double b = 0) { std::printf("FAIL %s at %ld: %.17g vs %.17g\n", what, at, a, b); return 1; }

// `time <n_keyframes> <n_points> <group>` (compile with -O2): the host walk and the drop-in on fresh copies of a map of that size, the solve
// itself answered by the recorder; prints "TIME host_walk_ms <x> dropin_ms <y> vertices <a> edges <b>" (the best of five)
static int time_mode(int n_kf, int n_mp, int n_group) {
  using namespace mock;
  double best[2] = {1e30, 1e30};
  const bool fix_scale = false;
  for (int rep = 0; rep < 5; rep++)
    for (int which = 0; which < 2; which++) {
      EgScene S; S.build(23, n_kf, n_mp, n_group);
      g_calls.clear();
      const auto t0 = std::chrono::steady_clock::now();
      if (which == 0) ORB_SLAM2::CeresOptimizerT<EgTypes>::OptimizeEssentialGraph(&S.map, &S.kf(S.loop), &S.kf(S.cur), S.non_corrected, S.corrected, S.loop_connections, fix_scale);
      else ORB_SLAM2::FrameOpsT<EgTypes>::OptimizeEssentialGraph(&S.map, &S.kf(S.loop), &S.kf(S.cur), S.non_corrected, S.corrected, S.loop_connections);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      best[which] = std::min(best[which], ms);
    }
  std::printf("TIME host_walk_ms %.3f dropin_ms %.3f vertices %d edges %d\n", best[0], best[1], (int)g_calls[0].fixed.size(), (int)g_calls[0].ej.size());
  return 0;
}

int main(int argc, char** argv) {
  using namespace mock;
  typedef ORB_SLAM2::CeresOptimizerT<EgTypes> Ceres;
  typedef ORB_SLAM2::FrameOpsT<EgTypes> Ops;
  if (argc == 5 && std::strcmp(argv[1], "time") == 0) return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  const int n_kf = 90, n_mp = 600, n_group = 7;
  EgScene A, B;
  A.build(17, n_kf, n_mp, n_group); B.build(17, n_kf, n_mp, n_group);
  for (int i = 0; i + 1 < n_kf; i++)                                  // the two copies lie in memory in the same order
    if ((&A.kf(i) < &A.kf(i + 1)) != (&B.kf(i) < &B.kf(i + 1))) return fail("pointer order of the copies");
  bool shuffled = false;
  for (int i = 0; i + 1 < n_kf; i++) shuffled = shuffled || &A.kf(i) > &A.kf(i + 1);
  if (!shuffled) return fail("the keyframes are not shuffled in memory");
  const bool fix_scale = false;
  Ceres::OptimizeEssentialGraph(&A.map, &A.kf(A.loop), &A.kf(A.cur), A.non_corrected, A.corrected, A.loop_connections, fix_scale);
  const int n_edges = Ops::OptimizeEssentialGraph(&B.map, &B.kf(B.loop), &B.kf(B.cur), B.non_corrected, B.corrected, B.loop_connections);
  if (g_calls.size() != 2) return fail("the solver was not called once by each", (long)g_calls.size());
  const Recorded &a = g_calls[0], &b = g_calls[1];
  if (a.fixed != b.fixed) return fail("vertices / fixed flags");
  if (a.ej != b.ej || a.ei != b.ei) {
    for (size_t e = 0; e < std::min(a.ej.size(), b.ej.size()); e++) if (a.ej[e] != b.ej[e] || a.ei[e] != b.ei[e]) return fail("edge", (long)e, a.ej[e] * 1000 + a.ei[e], b.ej[e] * 1000 + b.ei[e]);
    return fail("number of edges", -1, (double)a.ej.size(), (double)b.ej.size());
  }
  if ((int)b.ej.size() != n_edges) return fail("returned edge count");
  for (size_t q = 0; q < a.lie.size(); q++) if (!(std::fabs(a.lie[q] - b.lie[q]) <= 1e-12 * std::max(1.0, std::fabs(a.lie[q])))) return fail("lie7", (long)q, a.lie[q], b.lie[q]);
  for (size_t q = 0; q < a.S.size(); q++) if (!(std::fabs(a.S[q] - b.S[q]) <= 1e-12 * std::max(1.0, std::fabs(a.S[q])))) return fail("Sji", (long)q, a.S[q], b.S[q]);
  int n_loop_conn = 0;
  {                                                                   // the leading edges that end in a target of loop_connections, as long as they do
    std::vector<EgKeyFrame*> all = B.map.GetAllKeyFrames(), vtx;
    for (EgKeyFrame* k : all) if (!k->isBad()) vtx.push_back(k);
    size_t e = 0;
    for (auto& t : B.loop_connections) for (; e < b.ei.size() && vtx[b.ei[e]] == t.first && t.second.count(vtx[b.ej[e]]) && n_loop_conn == (int)e; e++) n_loop_conn++;
  }
  int moved = 0, poses = 0;
  for (int i = 0; i < n_kf; i++) {
    EgKeyFrame &x = A.kf(i), &y = B.kf(i);
    if (x.is_bad_) { for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) if (y.Tcw_(r, c) != x.Tcw_(r, c)) return fail("a bad keyframe moved", i); continue; }
    poses++;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 4; c++) if (!(std::fabs(x.Tcw_(r, c) - y.Tcw_(r, c)) <= 1e-12 * std::max(1.0, std::fabs(x.Tcw_(r, c))))) return fail("Tcw", i, x.Tcw_(r, c), y.Tcw_(r, c));
      if (!(std::fabs(x.Ow_[r] - y.Ow_[r]) <= 1e-12 * std::max(1.0, std::fabs(x.Ow_[r])))) return fail("centre", i, x.Ow_[r], y.Ow_[r]);
    }
  }
  EgScene C; C.build(17, n_kf, n_mp, n_group);                        // the map at entry
  for (int p = 0; p < n_mp; p++) {
    EgMapPoint &x = A.mp(p), &y = B.mp(p), &z = C.mp(p);
    bool mv = false;
    for (int k = 0; k < 3; k++) {
      if (!(std::fabs(x.world_pose_[k] - y.world_pose_[k]) <= 1e-12 * std::max(1.0, std::fabs(x.world_pose_[k])))) return fail("X", p, x.world_pose_[k], y.world_pose_[k]);
      mv = mv || y.world_pose_[k] != z.world_pose_[k];
    }
    moved += mv ? 1 : 0;
    // the host walk calls UpdateNormalAndDepth on every point it moves; a point without observations or reference keyframe keeps its normal
    for (int k = 0; k < 3; k++) if (!(std::fabs(x.normal_vector_[k] - y.normal_vector_[k]) <= 1e-9)) return fail("normal", p, x.normal_vector_[k], y.normal_vector_[k]);
    if (!(std::fabs(x.max_distance_ - y.max_distance_) <= 1e-5f * std::max(1.0f, std::fabs(x.max_distance_)))) return fail("max_distance", p, x.max_distance_, y.max_distance_);
    if (!(std::fabs(x.min_distance_ - y.min_distance_) <= 1e-5f * std::max(1.0f, std::fabs(x.min_distance_)))) return fail("min_distance", p, x.min_distance_, y.min_distance_);
  }
  if (moved < n_mp / 2 || poses < n_kf / 2 || n_loop_conn < 3 || (int)b.ej.size() < n_kf) return fail("weak case", moved, poses, (double)b.ej.size());
  std::printf("OK %d %d %d %d\n", (int)b.fixed.size(), (int)b.ej.size(), n_loop_conn, moved);
  return 0;
}
