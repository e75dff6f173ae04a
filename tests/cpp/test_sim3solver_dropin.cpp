// Drop-in case of Sim3SolverT (csrc/compat/orbslam_sim3solver.h; HIP library underneath) over the mock data model and a scripted RNG
// with DUtils::Random's interface.  Reads one loop candidate (written by tests/test_gpu_sim3solver_dropin.py) and makes the calls of
// LoopClosing::ComputeSim3 - SetRansacParameters(0.99, 20, 300), then iterate(5, ...) again and again, REJECTING every returned pose,
// until is_no_more, then twice more (a solver at its bound consumes nothing).  A second pass makes the same sequence with the library
// called directly - the compaction of src/Sim3Solver.cc:73-104, the draw of :169-182 on the same generator, the bookkeeping of
// :164-165 and :209 - and every call must agree bit for bit: pose, is_no_more, the scattered mask, n_inliers, R, t, scale.
// Prints "N n n_slots", one "CALL status consumed iterations is_no_more n_inliers" line per call and "OK" at the end.
//   g++ -O1 -std=c++17 -I include -I tests/cpp tests/cpp/test_sim3solver_dropin.cpp -o /tmp/t ceres_mono_orb_slam2_amd/lib/liborbslam_hip.so
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_sim3solver.h"
#include "mock_sim3.h"

namespace mock {
unsigned long MapPoint::next_id_ = 0, KeyFrame::next_id_ = 0;
std::mutex MapPoint::global_mutex_;
float Frame::fx_, Frame::fy_, Frame::cx_, Frame::cy_, Frame::min_x_, Frame::max_x_, Frame::min_y_, Frame::max_y_;
}  // namespace mock
uint64_t Sim3ScriptedRandom::state = 0;

typedef ORB_SLAM2::Sim3SolverT<mock::Types, Sim3ScriptedRandom> Sim3Solver;

struct Call { double T[16], R[9], t[3]; float s; bool no_more; std::vector<bool> inl; int n_inl; };

static int fail(const char* what) { std::printf("FAIL %s\n", what); return 1; }

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: test_sim3solver_dropin scene.bin");
  Sim3Scene S;
  if (!S.read(argv[1])) return fail("cannot read the scene");
  const int max_calls = 200;
  // ---- pass 1: the drop-in
  std::vector<Call> a;
  std::vector<size_t> dropin_indices;
  Sim3ScriptedRandom::Reset(7);
  {
    Sim3Solver* pSolver = new Sim3Solver(&S.kf1, &S.kf2, S.matches12, S.fix_scale != 0);
    pSolver->SetRansacParameters(0.99, 20, 300);
    dropin_indices = pSolver->matched_indices();
    std::printf("N %d %d\n", (int)dropin_indices.size(), (int)S.matches12.size());
    int after = 0;
    while ((int)a.size() < max_calls && after < 3) {
      Call c;
      bool is_no_more; int n_inliers;
      mock::Matrix4d Scm = pSolver->iterate(5, is_no_more, c.inl, n_inliers);
      for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) c.T[4 * r + k] = Scm(r, k);
      const mock::Matrix3d R = pSolver->GetEstimatedRotation();
      const mock::Vector3d t = pSolver->GetEstimatedTranslation();
      for (int r = 0; r < 3; r++) { for (int k = 0; k < 3; k++) c.R[3 * r + k] = R(r, k); c.t[r] = t[r]; }
      c.s = pSolver->GetEstimatedScale();
      c.no_more = is_no_more; c.n_inl = n_inliers;
      const bool few = pSolver->params().n < pSolver->params().min_inliers;
      std::printf("CALL %d %d %d %d %d\n", few ? -1 : pSolver->last_result().status, few ? 0 : pSolver->last_result().consumed, pSolver->iterations(),
                  (int)is_no_more, n_inliers);
      if ((int)c.inl.size() != (int)S.matches12.size()) return fail("is_inliers does not have N1 entries");
      a.push_back(c);
      if (is_no_more) after++;
      if (few) break;                                              // too few correspondences: nothing more to see
    }
    delete pSolver;
  }
  // ---- pass 2: the library called directly
  Sim3ScriptedRandom::Reset(7);
  std::vector<double> X1c, X2c; std::vector<float> e1, e2; std::vector<size_t> idx;
  std::vector<mock::MapPoint*> in1 = S.kf1.GetMapPointMatches();
  const mock::Matrix3d R1 = S.kf1.GetRotation(), R2 = S.kf2.GetRotation();
  const mock::Vector3d t1 = S.kf1.GetTranslation(), t2 = S.kf2.GetTranslation();
  for (size_t i = 0; i < S.matches12.size(); i++) {
    mock::MapPoint* p2 = S.matches12[i];
    mock::MapPoint* p1 = in1[i];
    if (!p2 || !p1 || p1->isBad() || p2->isBad()) continue;
    const int i1 = p1->GetIndexInKeyFrame(&S.kf1), i2 = p2->GetIndexInKeyFrame(&S.kf2);
    if (i1 < 0 || i2 < 0) continue;
    e1.push_back((float)(size_t)(9.210 * S.kf1.level_sigma2s_[S.kf1.undistort_keypoints_[i1].octave]));
    e2.push_back((float)(size_t)(9.210 * S.kf2.level_sigma2s_[S.kf2.undistort_keypoints_[i2].octave]));
    const mock::Vector3d A = p1->GetWorldPos(), B = p2->GetWorldPos();
    for (int r = 0; r < 3; r++) {
      X1c.push_back(((R1(r, 0) * A[0] + R1(r, 1) * A[1]) + R1(r, 2) * A[2]) + t1[r]);
      X2c.push_back(((R2(r, 0) * B[0] + R2(r, 1) * B[1]) + R2(r, 2) * B[2]) + t2[r]);
    }
    idx.push_back(i);
  }
  if (idx != dropin_indices) return fail("matched_indices_1_ differ from the constructor's skip rules");
  const int N = (int)idx.size();
  const float K1[4] = {S.kf1.fx_, S.kf1.fy_, S.kf1.cx_, S.kf1.cy_}, K2[4] = {S.kf2.fx_, S.kf2.fy_, S.kf2.cx_, S.kf2.cy_};
  orbt_sim3_params pr;
  if (orbt_sim3_ransac_params(N, 0.99, 20, 300, &pr)) return fail("orbt_sim3_ransac_params");
  int n_iterations = 0, best_count = 0;
  std::vector<uint8_t> best_mask((size_t)N, 0), inl((size_t)N, 0);
  double best_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, best_t[3] = {0, 0, 0};
  float best_s = 1.0f;
  const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (size_t k = 0; k < a.size(); k++) {
    Call c; c.no_more = false; c.n_inl = 0;
    std::memcpy(c.T, ident, sizeof ident);
    c.inl.assign(S.matches12.size(), false);
    if (N < pr.min_inliers) c.no_more = true;
    else {
      int n_sets = pr.max_iterations - n_iterations < 5 ? pr.max_iterations - n_iterations : 5;
      if (n_sets < 0) n_sets = 0;
      std::vector<int32_t> sets(3 * (size_t)n_sets + 3);
      for (int s = 0; s < n_sets; s++) {
        std::vector<int> avail(N);
        for (int i = 0; i < N; i++) avail[i] = i;
        for (int j = 0; j < 3; j++) {
          const int r = Sim3ScriptedRandom::RandomInt(0, (int)avail.size() - 1);
          sets[3 * (size_t)s + j] = avail[r]; avail[r] = avail.back(); avail.pop_back();
        }
      }
      orbt_sim3_result res;
      if (orbt_sim3_iterate(X1c.data(), X2c.data(), e1.data(), e2.data(), N, K1, K2, S.fix_scale != 0, pr.min_inliers, sets.data(), n_sets, &best_count,
                            best_mask.data(), best_R, best_t, &best_s, &res, inl.data(), nullptr))
        return fail(orbhip_last_error());
      n_iterations += res.consumed;
      if (res.status == ORBT_SIM3_FOUND) {
        std::memcpy(c.T, res.T12, sizeof c.T);
        c.n_inl = res.n_inliers;
        for (int i = 0; i < N; i++) if (inl[i]) c.inl[idx[i]] = true;
      } else if (n_iterations >= pr.max_iterations) c.no_more = true;
    }
    if (std::memcmp(c.T, a[k].T, sizeof c.T) != 0) return fail("the pose differs from the library's");
    if (c.no_more != a[k].no_more || c.n_inl != a[k].n_inl || c.inl != a[k].inl) return fail("is_no_more, n_inliers or the mask differ from the library's");
    if (std::memcmp(best_R, a[k].R, sizeof best_R) != 0 || std::memcmp(best_t, a[k].t, sizeof best_t) != 0 || std::memcmp(&best_s, &a[k].s, 4) != 0)
      return fail("GetEstimatedRotation / Translation / Scale differ from the library's state");
  }
  std::printf("OK\n");
  return 0;
}
