// Drop-in case of PnPsolverT (csrc/compat/orbslam_pnpsolver.h; HIP library underneath) over the mock data model and a scripted RNG
// with DUtils::Random's interface.  Reads one relocalisation candidate (written by tests/test_gpu_pnp_dropin.py) and makes the calls
// of Tracking::Relocalization - SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), then iterate(5, ...) again and again, REJECTING
// every returned pose, until bNoMore, then twice more (a solver called after exhaustion runs 5 more iterations).  A second pass
// makes the same sequence with the library called directly - the compaction of src/PnPsolver.cc:79-102, the draw of :189-202 on the
// same generator, the bookkeeping of :183 - and every call must agree bit for bit: pose, bNoMore, the scattered mask, nInliers.
// Prints one "CALL status consumed iterations bNoMore nInliers" line per call and "OK" at the end.
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_pnpsolver_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_pnpsolver.h"
#include "mock_pnp.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
uint64_t ScriptedRandom::state = 0;

typedef ORB_SLAM2::PnPsolverT<mock::Types, ScriptedRandom> PnPsolver;

struct Call { double T[16]; bool no_more; std::vector<bool> inl; int n_inl; };

static int fail(const char* what) { std::printf("FAIL %s\n", what); return 1; }

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: test_pnpsolver_dropin scene.bin");
  PnpScene S;
  if (!S.read(argv[1])) return fail("cannot read the scene");
  const int max_calls = 80;
  // ---- pass 1: the drop-in
  std::vector<Call> a;
  ScriptedRandom::Reset(7);
  {
    PnPsolver solver(S.frame, S.matches);
    solver.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    int after = 0;
    while ((int)a.size() < max_calls && after < 2) {
      Call c;
      bool no_more; int n_inl;
      mock::Matrix4d T = solver.iterate(5, no_more, c.inl, n_inl);
      for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) c.T[4 * r + k] = T(r, k);
      c.no_more = no_more; c.n_inl = n_inl;
      std::printf("CALL %d %d %d %d %d\n", solver.last_result().status, solver.last_result().consumed, solver.iterations(), (int)no_more, n_inl);
      a.push_back(c);
      if (no_more) after++;
      if (solver.params().n < solver.params().min_inliers) break;          // too few points: nothing more to see
    }
  }
  // ---- pass 2: the library called directly
  ScriptedRandom::Reset(7);
  std::vector<float> p3d, p2d, max_err; std::vector<size_t> kpi;
  for (size_t i = 0; i < S.matches.size(); i++) {
    mock::MapPoint* p = S.matches[i];
    if (!p || p->isBad()) continue;
    const mock::KeyPoint& kp = S.frame.undistort_keypoints_[i];
    p2d.push_back(kp.pt.x); p2d.push_back(kp.pt.y);
    max_err.push_back(S.frame.level_sigma2s_[kp.octave] * 5.991f);
    const mock::Vector3d X = p->GetWorldPos();
    p3d.push_back((float)X[0]); p3d.push_back((float)X[1]); p3d.push_back((float)X[2]);
    kpi.push_back(i);
  }
  const int N = (int)kpi.size();
  const float K4[4] = {mock::Frame::fx_, mock::Frame::fy_, mock::Frame::cx_, mock::Frame::cy_};
  orbt_pnp_params pr;
  if (orbt_pnp_ransac_params(N, 0.99, 10, 300, 4, 0.5f, &pr)) return fail("orbt_pnp_ransac_params");
  int mnIterations = 0, best_count = 0;
  std::vector<uint8_t> best_mask((size_t)N, 0), inl((size_t)N, 0);
  double best_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (size_t k = 0; k < a.size(); k++) {
    Call c; c.no_more = false; c.n_inl = 0;
    const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(c.T, ident, sizeof ident);
    if (N < pr.min_inliers) c.no_more = true;
    else {
      const int n_sets = pr.max_iterations - mnIterations > 5 ? pr.max_iterations - mnIterations : 5;
      std::vector<int32_t> sets(4 * (size_t)n_sets);
      for (int s = 0; s < n_sets; s++) {
        std::vector<int> avail(N);
        for (int i = 0; i < N; i++) avail[i] = i;
        for (int j = 0; j < 4; j++) {
          const int r = ScriptedRandom::RandomInt(0, (int)avail.size() - 1);
          sets[4 * (size_t)s + j] = avail[r]; avail[r] = avail.back(); avail.pop_back();
        }
      }
      orbt_pnp_result res;
      if (orbt_pnp_iterate(p3d.data(), p2d.data(), max_err.data(), N, K4,
                           pr.min_inliers, sets.data(), n_sets, &best_count, best_mask.data(), best_T, &res, inl.data(), nullptr))
        return fail(orbhip_last_error());
      mnIterations += res.consumed;
      c.no_more = res.status != ORBT_PNP_REFINED;
      if (res.status == ORBT_PNP_REFINED || res.status == ORBT_PNP_EXHAUSTED_BEST) {
        std::memcpy(c.T, res.Tcw, sizeof c.T);
        c.n_inl = res.n_inliers;
        c.inl.assign(S.matches.size(), false);
        for (int i = 0; i < N; i++) if (inl[i]) c.inl[kpi[i]] = true;
      }
    }
    if (std::memcmp(c.T, a[k].T, sizeof c.T) != 0) return fail("the pose differs from the library's");
    if (c.no_more != a[k].no_more || c.n_inl != a[k].n_inl || c.inl != a[k].inl) return fail("bNoMore, nInliers or the mask differ from the library's");
  }
  std::printf("OK\n");
  return 0;
}
