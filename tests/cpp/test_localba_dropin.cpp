// Drop-in case of FrameOpsT::AssembleLocalBA, ApplyLocalBA and LocalBundleAdjustment (csrc/compat/orbslam_dropin.h; HIP library underneath)
// over the mock data model of tests/cpp/mock_localba.h: copies of one seeded map (LbScene::build with one seed; keyframes AND points shuffled
// in memory, so that pointer order - the order of the reference's std::map containers - is not index order).
//   1. AssembleLocalBA against the reference-shaped loop of src/CeresOptimizer.cc:346-406, :423-506 on a second copy, field for field.
//   2. ApplyLocalBA, fed a synthetic result (seeded pose and point perturbations, seeded erase flags), against the literal :573-598 loop on
//      that copy: the WHOLE map state must be equal bit for bit - poses, inverse poses, centres, slots, positions, normals, depth ranges,
//      observations, Observations(), reference keyframes, bad flags.
//   3. LocalBundleAdjustment with the stop flag preset leaves a map as it was; without it, it returns 0 and the map is still consistent.
//   4. A map that is not consistent: -1, untouched.
// Prints "OK <cameras> <local points> <rows> <rows erased> <points turned bad>"; with the argument `host` only the host loops run (no
// library call beyond the host-only pose codec) and print "HOST" with the same five counts.
//   g++ -O1 -std=c++17 -ffp-contract=off -I include -I tests/cpp tests/cpp/test_localba_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
// With the arguments `time <n_keyframes> <n_points> <half window>`: builds a map of that size (compile with -O2), times the two host loops
// and the two drop-in calls on fresh copies, checks them equal, and prints "TIME host_loop_ms <x> dropin_ms <y> cameras <a> points <b> rows <c>" (the best of five).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_localba.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;

struct LbScene {
  std::vector<LbKeyFrame> store; std::vector<LbMapPoint> pstore; std::vector<int> place, pplace, at_place, at_pplace; LbMap map; int cur = 0;
  LbKeyFrame& kf(int i) { return store[place[i]]; }
  LbMapPoint& mp(int p) { return pstore[pplace[p]]; }
  int index_of(const LbKeyFrame* k) const { return k ? at_place[k - store.data()] : -1; }
  int index_of(const LbMapPoint* m) const { return m ? at_pplace[m - pstore.data()] : -1; }
  // n_kf keyframes on a line looking down z with small rotations, n_mp points in front of them, each seen from 1-7 keyframes of a window
  // around its place (its keypoint = its projection plus half a pixel of noise, a few gross outliers); null slots; a tenth of the keyframes
  // bad (still in the lists, as a keyframe is between SetBadFlag and its erasure); a few bad points (no observations, no reference keyframe,
  // half of them still in one slot); the current
  // keyframe in the middle, its covisible list = the keyframes within `half` of it, shuffled, one of them bad, one named twice
  void build(unsigned seed, int n_kf, int n_mp, int half) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> G(0.0, 1.0);
    store = std::vector<LbKeyFrame>(n_kf); place.resize(n_kf); pstore = std::vector<LbMapPoint>(n_mp); pplace.resize(n_mp);
    for (int i = 0; i < n_kf; i++) place[i] = i;
    for (int p = 0; p < n_mp; p++) pplace[p] = p;
    std::shuffle(place.begin(), place.end(), rng); std::shuffle(pplace.begin(), pplace.end(), rng);
    at_place.resize(n_kf); at_pplace.resize(n_mp);
    for (int i = 0; i < n_kf; i++) at_place[place[i]] = i;
    for (int p = 0; p < n_mp; p++) at_pplace[pplace[p]] = p;
    std::vector<float> sf(8), isg(8);
    for (int l = 0; l < 8; l++) { sf[l] = (float)std::pow(1.2, l); isg[l] = 1.0f / (sf[l] * sf[l]); }
    cur = n_kf / 2;
    for (int i = 0; i < n_kf; i++) {
      LbKeyFrame& k = kf(i);
      k.id_ = (unsigned long)((i * 7 + 3) % n_kf); k.scale_factors_ = sf; k.inv_level_sigma2s_ = isg;
      k.fx_ = 458.654f; k.fy_ = 457.296f; k.cx_ = 367.215f; k.cy_ = 248.375f;
      k.SetPose(make_pose(0.02 * G(rng), 0.02 * G(rng), Vector3d(0.25 * i, 0.03 * G(rng), 0.03 * G(rng))));
      k.is_bad_ = i != cur && rng() % 10 == 0;
    }
    kf(std::max(0, cur - half)).is_bad_ = true;
    for (int p = 0; p < n_mp; p++) {
      LbMapPoint& m = mp(p);
      const double at = U(rng) * n_kf;
      m.world_pose_ = Vector3d(0.25 * at + 0.8 * G(rng), 0.8 * G(rng), 5.0 + 3.0 * U(rng));
      m.normal_vector_ = Vector3d(-7, -7, -7); m.min_distance_ = -7; m.max_distance_ = -7;
      if (rng() % 25 == 0) {                                            // (half of them caught inside SetBadFlag: observations cleared, one slot not yet emptied)
        m.is_bad_ = true;
        if (rng() % 2) { LbKeyFrame& K = kf((int)at); K.map_points_.push_back(&m); K.undistort_keypoints_.push_back(KeyPoint()); }
        continue;
      }
      std::vector<int> cand;
      for (int k = std::max(0, (int)at - 4); k < std::min(n_kf, (int)at + 5); k++) cand.push_back(k);
      std::shuffle(cand.begin(), cand.end(), rng);
      const int n = std::min((int)cand.size(), 1 + (int)(rng() % 7));
      for (int j = 0; j < n; j++) {
        LbKeyFrame& K = kf(cand[j]);
        if (rng() % 8 == 0) { K.map_points_.push_back(nullptr); K.undistort_keypoints_.push_back(KeyPoint()); }
        double xc[3];
        for (int r = 0; r < 3; r++) xc[r] = ((K.Tcw_(r, 0) * m.world_pose_[0] + K.Tcw_(r, 1) * m.world_pose_[1]) + K.Tcw_(r, 2) * m.world_pose_[2]) + K.Tcw_(r, 3);
        KeyPoint kp; kp.octave = (int)(rng() % 4);
        kp.pt.x = (float)(K.fx_ * xc[0] / xc[2] + K.cx_ + 0.5 * G(rng) + (rng() % 40 == 0 ? 30.0 : 0.0)); kp.pt.y = (float)(K.fy_ * xc[1] / xc[2] + K.cy_ + 0.5 * G(rng));
        K.map_points_.push_back(&m); K.undistort_keypoints_.push_back(kp);
        m.observations_[&K] = K.map_points_.size() - 1;
      }
      m.n_observations_ = n;
      m.reference_keyframe_ = &kf(cand[rng() % n]);
      m.world_pose_ = Vector3d(m.world_pose_[0] + 0.02 * G(rng), m.world_pose_[1] + 0.02 * G(rng), m.world_pose_[2] + 0.02 * G(rng));
    }
    std::vector<int> nb;
    for (int i = std::max(0, cur - half); i < std::min(n_kf, cur + half + 1); i++) if (i != cur) nb.push_back(i);
    std::shuffle(nb.begin(), nb.end(), rng);
    nb.push_back(nb[1]);
    for (int i : nb) kf(cur).covisible_.push_back(&kf(i));
  }
  // keyframe k holds p in slot i iff p's observations contain (k, i); a bad point still in a slot is exempt
  bool consistent() {
    for (LbMapPoint& m : pstore)
      for (auto& o : m.observations_) if (o.second >= o.first->map_points_.size() || o.first->map_points_[o.second] != &m) return false;
    for (LbKeyFrame& k : store)
      for (size_t s = 0; s < k.map_points_.size(); s++) {
        LbMapPoint* m = k.map_points_[s];
        if (m && !m->is_bad_ && !(m->observations_.count(&k) && m->observations_[&k] == s)) return false;
      }
    return true;
  }
};

static bool bits(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

static bool same(LbScene& A, LbScene& B, const char* what) {
  for (size_t i = 0; i < A.place.size(); i++) {
    LbKeyFrame &a = A.kf((int)i), &b = B.kf((int)i);
    if (!bits(a.Tcw_.m, b.Tcw_.m, 128) || !bits(a.Twc_.m, b.Twc_.m, 128) || !bits(a.Ow_.v, b.Ow_.v, 24)) { std::printf("FAIL %s: pose of keyframe %zu\n", what, i); return false; }
    if (a.map_points_.size() != b.map_points_.size()) { std::printf("FAIL %s: slots of keyframe %zu\n", what, i); return false; }
    for (size_t s = 0; s < a.map_points_.size(); s++)
      if (A.index_of(a.map_points_[s]) != B.index_of(b.map_points_[s])) { std::printf("FAIL %s: slot %zu of keyframe %zu\n", what, s, i); return false; }
  }
  for (size_t p = 0; p < A.pplace.size(); p++) {
    LbMapPoint &a = A.mp((int)p), &b = B.mp((int)p);
    if (!bits(a.world_pose_.v, b.world_pose_.v, 24)) { std::printf("FAIL %s: position of point %zu\n", what, p); return false; }
    if (!bits(a.normal_vector_.v, b.normal_vector_.v, 24) || !bits(&a.min_distance_, &b.min_distance_, 4) || !bits(&a.max_distance_, &b.max_distance_, 4)) {
      std::printf("FAIL %s: normal / depth of point %zu\n", what, p); return false;
    }
    if (a.is_bad_ != b.is_bad_ || a.n_observations_ != b.n_observations_ || A.index_of(a.reference_keyframe_) != B.index_of(b.reference_keyframe_)) {
      std::printf("FAIL %s: flag / Observations() / reference keyframe of point %zu (%d %d, %d %d, %d %d)\n", what, p, (int)a.is_bad_, (int)b.is_bad_, a.n_observations_,
                  b.n_observations_, A.index_of(a.reference_keyframe_), B.index_of(b.reference_keyframe_));
      return false;
    }
    std::map<int, size_t> oa, ob;
    for (auto& o : a.observations_) oa[A.index_of(o.first)] = o.second;
    for (auto& o : b.observations_) ob[B.index_of(o.first)] = o.second;
    if (oa != ob) { std::printf("FAIL %s: observations of point %zu\n", what, p); return false; }
  }
  return true;
}
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::FrameOpsT<mock::LbTypes> Ops;
typedef Ops::LocalBAProblemT<LbKeyFrame, LbMapPoint> DropinProblem;

static bool same_problem(LbScene& A, DropinProblem& a, LbScene& B, LbProblem& b) {
  const size_t ncam = b.cams.size(), npl = b.pts.size(), nol = b.edges.size();
  if ((size_t)a.counts[0] != ncam || (size_t)a.counts[2] != npl || (size_t)a.counts[3] != nol || (size_t)a.counts[1] != b.local_kfs.size()) {
    std::printf("FAIL counts %d %d %d %d vs %zu %zu %zu %zu\n", a.counts[0], a.counts[1], a.counts[2], a.counts[3], ncam, b.local_kfs.size(), npl, nol); return false;
  }
  for (size_t c = 0; c < ncam; c++)
    if (A.index_of(a.kfs[a.cam_kf[c]]) != B.index_of(b.cams[c]) || a.cam_fixed[c] != b.cam_fixed[c] || a.cam_local[c] != b.cam_local[c]) { std::printf("FAIL camera %zu\n", c); return false; }
  if (!bits(a.K4.data(), b.K4.data(), 32 * ncam) || !bits(a.poses7.data(), b.poses7.data(), 56 * ncam)) { std::printf("FAIL K4 / poses7\n"); return false; }
  for (size_t j = 0; j < npl; j++) if (A.index_of(a.pts[a.lpt_pt[j]]) != B.index_of(b.pts[j])) { std::printf("FAIL point %zu\n", j); return false; }
  if (!bits(a.pts3.data(), b.pts3.data(), 24 * npl)) { std::printf("FAIL pts3\n"); return false; }
  if (!bits(a.lobs_cam.data(), b.obs_cam.data(), 4 * nol) || !bits(a.lobs_pt.data(), b.obs_pt.data(), 4 * nol) || !bits(a.lobs_uv.data(), b.obs_uv.data(), 16 * nol) ||
      !bits(a.lobs_inv_sigma2.data(), b.obs_isg.data(), 4 * nol)) { std::printf("FAIL rows\n"); return false; }
  for (size_t i = 0; i < nol; i++) {
    const int e = a.lobs_src[i];
    if (A.index_of(a.kfs[a.obs_kf[e]]) != B.index_of(b.edges[i].first) || a.lpt_pt[a.lobs_pt[i]] < 0 || !(a.obs_off[a.lpt_pt[a.lobs_pt[i]]] <= e && e < a.obs_off[a.lpt_pt[a.lobs_pt[i]] + 1])) {
      std::printf("FAIL lobs_src of row %zu\n", i); return false;
    }
  }
  return true;
}

// a synthetic result of the solve: seeded perturbations of the assembled poses and points, erase flags on a fifth of the rows
static void synthetic_result(const LbProblem& P, std::vector<double>* poses7, std::vector<double>* pts3, std::vector<uint8_t>* erase) {
  std::mt19937 rng(99);
  std::normal_distribution<double> G(0.0, 1.0);
  *poses7 = P.poses7; *pts3 = P.pts3;
  for (size_t c = 0; c < P.cams.size(); c++) {
    const double s = 0.5 + (rng() % 100) / 50.0;
    for (int k = 0; k < 3; k++) (*poses7)[7 * c + k] += 0.05 * G(rng);
    for (int k = 3; k < 7; k++) (*poses7)[7 * c + k] = ((*poses7)[7 * c + k] + 0.01 * G(rng)) * s;
  }
  for (double& v : *pts3) v += 0.05 * G(rng);
  erase->assign(std::max<size_t>(P.edges.size(), 1), 0);
  for (size_t i = 0; i < P.edges.size(); i++) (*erase)[i] = rng() % 5 == 0;
}

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

static int time_mode(int n_kf, int n_mp, int half) {
  { std::unique_ptr<LbScene> W(new LbScene); W->build(5, 16, 200, 3); DropinProblem P; Ops::AssembleLocalBA(&W->kf(W->cur), &P); }      // (the first call pays for the runtime's start)
  double best_host = 1e30, best_drop = 1e30;
  int sizes[3] = {0, 0, 0};
  for (int rep = 0; rep < 5; rep++) {
    std::unique_ptr<LbScene> A(new LbScene), B(new LbScene);
    A->build(21, n_kf, n_mp, half); B->build(21, n_kf, n_mp, half);
    LbProblem pb; DropinProblem pa;
    std::vector<double> poses7, pts3; std::vector<uint8_t> erase;
    auto t0 = std::chrono::steady_clock::now();
    AssembleHost(&B->kf(B->cur), &pb);
    double host = ms_since(t0);
    synthetic_result(pb, &poses7, &pts3, &erase);
    t0 = std::chrono::steady_clock::now();
    ApplyHost(&pb, poses7.data(), pts3.data(), erase.data());
    best_host = std::min(best_host, host + ms_since(t0));
    t0 = std::chrono::steady_clock::now();
    if (Ops::AssembleLocalBA(&A->kf(A->cur), &pa) < 0) { std::printf("FAIL the timed map is not consistent\n"); return 1; }
    Ops::ApplyLocalBA(&pa, poses7.data(), pts3.data(), erase.data());
    best_drop = std::min(best_drop, ms_since(t0));
    if (!same(*A, *B, "timed")) return 1;
    sizes[0] = pa.counts[0]; sizes[1] = pa.counts[2]; sizes[2] = pa.counts[3];
  }
  std::printf("TIME host_loop_ms %.3f dropin_ms %.3f cameras %d points %d rows %d\n", best_host, best_drop, sizes[0], sizes[1], sizes[2]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "time") return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  const bool host_only = argc == 2 && std::string(argv[1]) == "host";
  const unsigned seed = 8; const int n_kf = 40, n_mp = 1500, half = 6;
  std::unique_ptr<LbScene> A(new LbScene), B(new LbScene);
  A->build(seed, n_kf, n_mp, half); B->build(seed, n_kf, n_mp, half);
  bool shuffled = false;
  for (int i = 0; i + 1 < n_kf; i++) shuffled |= &A->kf(i) > &A->kf(i + 1);
  if (!shuffled || !A->consistent() || !same(*A, *B, "before")) { std::printf("FAIL the map as built\n"); return 1; }
  // 1. the assembled problem
  LbProblem pb;
  AssembleHost(&B->kf(B->cur), &pb);
  std::vector<double> poses7, pts3; std::vector<uint8_t> erase;
  synthetic_result(pb, &poses7, &pts3, &erase);
  int n_erase = 0, n_bad_before = 0, n_bad_after = 0;
  for (size_t i = 0; i < pb.edges.size(); i++) n_erase += erase[i];
  for (LbMapPoint& m : B->pstore) n_bad_before += m.is_bad_;
  // 2. the write-back on the host
  ApplyHost(&pb, poses7.data(), pts3.data(), erase.data());
  for (LbMapPoint& m : B->pstore) n_bad_after += m.is_bad_;
  if (!B->consistent()) { std::printf("FAIL the host loop left the map inconsistent\n"); return 1; }
  if (host_only) { std::printf("HOST %zu %zu %zu %d %d\n", pb.cams.size(), pb.pts.size(), pb.edges.size(), n_erase, n_bad_after - n_bad_before); return 0; }
  DropinProblem pa;
  if (Ops::AssembleLocalBA(&A->kf(A->cur), &pa) < 0) { std::printf("FAIL AssembleLocalBA calls the map inconsistent\n"); return 1; }
  {
    std::unique_ptr<LbScene> C(new LbScene);                          // (the assembly changes nothing the comparison sees)
    C->build(seed, n_kf, n_mp, half);
    LbProblem pc;
    AssembleHost(&C->kf(C->cur), &pc);
    if (!same(*A, *C, "after the assembly") || !same_problem(*A, pa, *C, pc)) return 1;
  }
  std::vector<LbMapPoint*> turned_bad;
  Ops::ApplyLocalBA(&pa, poses7.data(), pts3.data(), erase.data(), &turned_bad);
  if (!same(*A, *B, "after the write-back")) return 1;
  if ((int)turned_bad.size() != n_bad_after - n_bad_before) { std::printf("FAIL %zu points reported as turned bad, %d did\n", turned_bad.size(), n_bad_after - n_bad_before); return 1; }
  for (LbMapPoint* m : turned_bad) if (!m->is_bad_ || B->mp(A->index_of(m)).observations_.size() != 0) { std::printf("FAIL a point reported as turned bad is not\n"); return 1; }
  // 3. the stop flag, then a whole call
  {
    std::unique_ptr<LbScene> C(new LbScene), D(new LbScene);
    C->build(seed, n_kf, n_mp, half); D->build(seed, n_kf, n_mp, half);
    bool stop = true;
    if (Ops::LocalBundleAdjustment(&C->kf(C->cur), &stop, &C->map) != 0 || !same(*C, *D, "with the stop flag up")) { std::printf("FAIL stop flag\n"); return 1; }
    stop = false;
    std::vector<LbMapPoint*> gone;
    int was_bad = 0, is_bad = 0;
    for (LbMapPoint& m : C->pstore) was_bad += m.is_bad_;
    if (Ops::LocalBundleAdjustment(&C->kf(C->cur), &stop, &C->map, &gone) != 0 || !C->consistent()) { std::printf("FAIL the whole call\n"); return 1; }
    for (LbMapPoint& m : C->pstore) is_bad += m.is_bad_;
    if ((int)gone.size() != is_bad - was_bad) { std::printf("FAIL the whole call reports %zu points turned bad, %d did\n", gone.size(), is_bad - was_bad); return 1; }
    if (bits(C->kf(C->cur).Tcw_.m, D->kf(D->cur).Tcw_.m, 128)) { std::printf("FAIL the whole call left the current keyframe's pose\n"); return 1; }
  }
  // 4. an inconsistent map: a slot of the current keyframe holds a point that lists another slot of it
  {
    std::unique_ptr<LbScene> C(new LbScene), D(new LbScene);
    C->build(seed, n_kf, n_mp, half); D->build(seed, n_kf, n_mp, half);
    for (LbScene* S : {C.get(), D.get()}) {
      std::vector<LbMapPoint*>& slots = S->kf(S->cur).map_points_;
      size_t first = slots.size();
      for (size_t s = 0; s < slots.size(); s++) if (slots[s]) { if (first == slots.size()) first = s; else { slots[first] = slots[s]; break; } }
    }
    bool stop = false;
    DropinProblem pc;
    if (Ops::AssembleLocalBA(&C->kf(C->cur), &pc) != -1 || Ops::LocalBundleAdjustment(&C->kf(C->cur), &stop, &C->map) != -1 || !same(*C, *D, "inconsistent map")) {
      std::printf("FAIL an inconsistent map is not refused\n"); return 1;
    }
  }
  std::printf("OK %zu %zu %zu %d %d\n", pb.cams.size(), pb.pts.size(), pb.edges.size(), n_erase, n_bad_after - n_bad_before);
  return 0;
}
