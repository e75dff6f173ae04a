// Drop-in case of FrameOpsT::RelocalizationRefine (csrc/compat/orbslam_dropin.h; orbt_relocalization_refine underneath) over the mock
// data model of tests/cpp/mock_orbslam.h.  The current frame is extracted on the device from a synthetic image (the call needs the
// frame an extracting orbt_* call left there) and copied into a mock Frame; every candidate keyframe holds the same features with map
// points at 18 m in front of them, so the true pose is the identity and the PnP poses are small motions away from it.  On that frame
//   (1) a host loop of the reference's shape (src/Tracking.cc:1040-1127, restated: for every candidate with a pose the slots and `found`
//       from the inliers, then the existing drop-ins CeresOptimizer::PoseOptimization and ORBmatcher::SearchByProjection(Frame&,
//       KeyFrame*, found, th, ORBdist) with the narrow search inside the `ip` loop, break at the first nGood >= 50) runs and its result is
//       recorded; is_outliers_ is cleared per candidate (the drop-in writes every flag; the reference's left-overs sit on empty slots);
//   (2) the frame is put back and FrameOpsT::RelocalizationRefine runs.
// Tcw_, map_points_, is_outliers_ and the returned index must be equal, for a round whose match sits in the middle and for one without.
// The candidates include one without a pose, a point held at two keyframe features, and an inlier point the keyframe does not hold.
// Prints "OK <rounds> <first match of round 1> <first match of round 2> <slots filled> <candidates refined>" on success.
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_reloc_refine_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <memory>
#include <random>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_dropin.h"
#include "mock_orbslam.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
using namespace mock;
typedef ORB_SLAM2::ORBmatcherT<mock::Types> ORBmatcher;
typedef ORB_SLAM2::CeresOptimizerT<mock::Types> CeresOptimizer;
typedef ORB_SLAM2::FrameOpsT<mock::Types> FrameOps;

static const int W = 640, H = 480;
static const float K4[4] = {517.3f, 516.5f, 318.6f, 255.3f};

static bool is_identity(const Matrix4d& T) { for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) if (T(r, c) != (r == c ? 1.0 : 0.0)) return false; return true; }

// the loop of src/Tracking.cc:1040-1127 for one pass of the `while`, over the existing drop-ins
static int host_loop(Frame& F, const std::vector<KeyFrame*>& kfs, const std::vector<std::vector<MapPoint*> >& matches, const std::vector<Matrix4d>& poses,
                     const std::vector<std::vector<bool> >& inliers, int* refined) {
  ORBmatcher matcher2(0.9, true);
  for (size_t i = 0; i < kfs.size(); i++) {
    if (is_identity(poses[i])) continue;
    (*refined)++;
    F.Tcw_ = poses[i];
    std::set<MapPoint*> found;
    for (int j = 0; j < F.N_; j++) {
      if (inliers[i][j]) { F.map_points_[j] = matches[i][j]; found.insert(matches[i][j]); }
      else F.map_points_[j] = nullptr;
    }
    std::fill(F.is_outliers_.begin(), F.is_outliers_.end(), false);
    int nGood = CeresOptimizer::PoseOptimization(&F);
    if (nGood < 10) continue;
    for (int io = 0; io < F.N_; io++) if (F.is_outliers_[io]) F.map_points_[io] = nullptr;
    if (nGood < 50) {
      int nadditional = matcher2.SearchByProjection(F, kfs[i], found, 10, 100);
      if (nadditional + nGood >= 50) {
        nGood = CeresOptimizer::PoseOptimization(&F);
        if (nGood > 30 && nGood < 50) {
          found.clear();
          for (int ip = 0; ip < F.N_; ip++) {
            if (F.map_points_[ip]) found.insert(F.map_points_[ip]);
            nadditional = matcher2.SearchByProjection(F, kfs[i], found, 3, 64);
          }
          if (nGood + nadditional >= 50) {
            nGood = CeresOptimizer::PoseOptimization(&F);
            for (int io = 0; io < F.N_; io++) if (F.is_outliers_[io]) F.map_points_[io] = nullptr;
          }
        }
      }
    }
    if (nGood >= 50) return (int)i;
  }
  return -1;
}

int main() {
  // the image: random blocks on a grey ground
  std::mt19937 rng(7);
  std::vector<uint8_t> img((size_t)W * H, 110);
  for (int b = 0; b < 900; b++) {
    const int x0 = (int)(rng() % (W - 8)), y0 = (int)(rng() % (H - 8)), w = 6 + (int)(rng() % 40), h = 6 + (int)(rng() % 40);
    const uint8_t v = (uint8_t)(30 + rng() % 200);
    for (int y = y0; y < std::min(H, y0 + h); y++) for (int x = x0; x < std::min(W, x0 + w); x++) img[(size_t)y * W + x] = v;
  }
  orbx_ctx* ex = nullptr;
  if (orbx_create(1000, 1.2f, 8, 20, 7, 0, &ex) != 0) { std::printf("FAIL orbx_create: %s\n", orbhip_last_error()); return 1; }
  const int cap = orbx_max_keypoints(ex);
  std::vector<orbx_keypoint> kps((size_t)cap); std::vector<uint8_t> desc((size_t)cap * 32), outl((size_t)cap); std::vector<int32_t> owner((size_t)cap);
  const float bounds[4] = {0.f, (float)W, 0.f, (float)H};
  const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  orbt_result tr;
  if (orbt_track_with_motion_model(ex, img.data(), W, H, W, K4, bounds, I12, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 15.f, 1, kps.data(), desc.data(), cap, nullptr,
                                   owner.data(), outl.data(), &tr) != 0) { std::printf("FAIL extraction: %s\n", orbhip_last_error()); return 1; }
  const int N = tr.n_keypoints;
  if (N < 600) { std::printf("FAIL only %d keypoints\n", N); return 1; }
  float scale[16], sigma2[16], inv_sigma2[16];
  orbx_get_tables(ex, scale, nullptr, sigma2, inv_sigma2, nullptr);
  Frame::fx_ = K4[0]; Frame::fy_ = K4[1]; Frame::cx_ = K4[2]; Frame::cy_ = K4[3];
  Frame::min_x_ = 0; Frame::max_x_ = (float)W; Frame::min_y_ = 0; Frame::max_y_ = (float)H;
  auto fill = [&](GridOwner& g) {
    g.N_ = N; g.keypoints_.resize(N); g.descriptors_ = Mat(N); g.map_points_.assign(N, nullptr);
    for (int i = 0; i < N; i++) {
      KeyPoint& k = g.keypoints_[i];
      k.pt.x = kps[i].x; k.pt.y = kps[i].y; k.size = kps[i].size; k.angle = kps[i].angle; k.response = kps[i].response; k.octave = kps[i].octave;
      std::memcpy(g.descriptors_.ptr(i), &desc[32 * (size_t)i], 32);
    }
    g.undistort_keypoints_ = g.keypoints_;
    g.scale_factors_.assign(scale, scale + 8); g.level_sigma2s_.assign(sigma2, sigma2 + 8); g.inv_level_sigma2s_.assign(inv_sigma2, inv_sigma2 + 8);
    g.build_grid(0, (float)W, 0, (float)H);
  };
  Frame F; fill(F); F.is_outliers_.assign(N, false);
  // the candidates: {correct inliers, wrong inliers, fraction of the features that hold a point, pose (0: none)}
  struct Spec { int n_correct, n_wrong; double points; double motion; };
  const Spec round1[] = {{20, 8, 0.0, 0.02}, {40, 0, 0.5, 0.0}, {6, 12, 0.5, 0.02}, {25, 8, 0.6, 0.02}, {120, 10, 0.5, 0.01}};
  const Spec round2[] = {{20, 8, 0.0, 0.02}, {6, 12, 0.5, 0.02}, {2, 0, 0.5, 0.01}, {30, 20, 0.012, 0.02}};
  std::vector<std::unique_ptr<KeyFrame> > kf_store; std::vector<std::unique_ptr<MapPoint> > mp_store;
  int firsts[2] = {-9, -9}, filled = 0, refined = 0, rounds = 0;
  for (int round = 0; round < 2; round++) {
    const Spec* specs = round == 0 ? round1 : round2; const int nc = round == 0 ? 5 : 4;
    std::vector<KeyFrame*> kfs; std::vector<std::vector<MapPoint*> > matches; std::vector<Matrix4d> poses; std::vector<std::vector<bool> > inliers;
    for (int c = 0; c < nc; c++) {
      const Spec& s = specs[c];
      std::mt19937 r(100 * round + c + 1); std::uniform_real_distribution<double> U(0, 1); std::normal_distribution<double> G(0, 1);
      kf_store.emplace_back(new KeyFrame); KeyFrame* kf = kf_store.back().get(); fill(*kf);
      std::vector<int> perm(N); for (int i = 0; i < N; i++) perm[i] = i; std::shuffle(perm.begin(), perm.end(), r);
      auto point_of = [&](int i) {
        if (kf->map_points_[i]) return kf->map_points_[i];
        mp_store.emplace_back(new MapPoint); MapPoint* mp = mp_store.back().get();
        const KeyPoint& k = kf->undistort_keypoints_[i];
        const double z = 18.0 * (1.0 + 0.002 * G(r));
        mp->world_pose_ = Vector3d((k.pt.x - K4[2]) / K4[0] * z, (k.pt.y - K4[3]) / K4[1] * z, z);
        mp->descriptor_ = kf->descriptors_.row(i);
        mp->max_distance_ = (float)(mp->world_pose_.norm() * scale[k.octave] * 0.95); mp->min_distance_ = mp->max_distance_ / scale[7];
        mp->n_observations_ = 1;
        kf->map_points_[i] = mp;
        return mp;
      };
      std::vector<MapPoint*> m(N, nullptr); std::vector<bool> inl(N, false);
      int at = 0;
      for (int k = 0; k < s.n_correct; k++, at++) { const int f = perm[at]; m[f] = point_of(f); inl[f] = true; }
      for (int k = 0; k < s.n_wrong; k++, at += 2) { const int f = perm[at]; m[f] = point_of(perm[at + 1]); inl[f] = true; }      // the point of another feature
      for (int i = at; i < N; i++) if (U(r) < s.points) point_of(perm[i]);
      // matches that are not inliers (masked out, :1070), a point at two keyframe features, an inlier the keyframe does not hold
      for (int k = 0; k < 10; k++) { const int f = perm[N - 1 - k]; if (!m[f]) m[f] = point_of(f); }
      if (s.n_correct > 3) {
        kf->map_points_[perm[N - 20]] = m[perm[0]];
        mp_store.emplace_back(new MapPoint(*m[perm[1]])); kf->map_points_[perm[1]] = nullptr; m[perm[1]] = mp_store.back().get();
      }
      Matrix4d T;
      if (s.motion > 0) { T = make_pose(0.05 * s.motion * G(r), 0.05 * s.motion * G(r), Vector3d(s.motion * G(r), s.motion * G(r), s.motion * G(r))); }
      kfs.push_back(kf); matches.push_back(m); poses.push_back(T); inliers.push_back(inl);
    }
    const std::vector<MapPoint*> slots0 = F.map_points_; const std::vector<bool> flags0 = F.is_outliers_; const Matrix4d T0 = F.Tcw_;
    const int want = host_loop(F, kfs, matches, poses, inliers, &refined);
    const std::vector<MapPoint*> want_slots = F.map_points_; const std::vector<bool> want_flags = F.is_outliers_; const Matrix4d want_T = F.Tcw_;
    F.map_points_ = slots0; F.is_outliers_ = flags0; F.Tcw_ = T0;
    const int got = FrameOps::RelocalizationRefine(ex, F, kfs, matches, poses, inliers);
    if (got != want) { std::printf("FAIL round %d: first match %d, the host loop says %d\n", round, got, want); return 1; }
    if (F.map_points_ != want_slots) { int d = 0; for (int f = 0; f < N; f++) d += F.map_points_[f] != want_slots[f]; std::printf("FAIL round %d: %d slots differ\n", round, d); return 1; }
    if (F.is_outliers_ != want_flags) { std::printf("FAIL round %d: is_outliers_\n", round); return 1; }
    if (std::memcmp(F.Tcw_.m, want_T.m, sizeof(want_T.m)) != 0) { std::printf("FAIL round %d: Tcw_\n", round); return 1; }
    firsts[round] = got; rounds++;
    for (int f = 0; f < N; f++) filled += F.map_points_[f] ? 1 : 0;
  }
  orbx_destroy(ex);
  std::printf("OK %d %d %d %d %d\n", rounds, firsts[0], firsts[1], filled, refined);
  return 0;
}
