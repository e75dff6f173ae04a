// ============================================================================
// orbslam_dropin.h -- ORB_SLAM2::ORBmatcher and ORB_SLAM2::CeresOptimizer with the REFERENCE's member-function
// signatures (reference include/ORBmatcher.h:36-97, include/CeresOptimizer.h:351-376), implemented over the C ABI of
// include/orbslam_hip.h.  The call sites in Tracking / LocalMapping / LoopClosing compile unchanged:
//
//     ORBmatcher matcher(0.9, true);
//     int nmatches = matcher.SearchByProjection(current_frame_, last_frame_, th);       // src/Tracking.cc:632
//     CeresOptimizer::PoseOptimization(&current_frame_);                                // src/Tracking.cc:646
//     CeresOptimizer::LocalBundleAdjustment(current_keyframe_, &is_abort_BA_, map_);    // src/LocalMapping.cc:89
//
// The classes are templates over a `Types` bundle naming the reference's own data model (Frame, KeyFrame, MapPoint, Map,
// the Eigen fixed-size types, cv::Mat / cv::KeyPoint / cv::Point2f).  Inside the reference tree
//     #define ORBSLAM_DROPIN_REFERENCE_TYPES       (before including this header; needs Frame.h, KeyFrame.h, MapPoint.h, Map.h)
// instantiates them as ORB_SLAM2::ORBmatcher / ORB_SLAM2::CeresOptimizer; tests/cpp/ instantiates them over mock structs
// that copy the member names of include/Frame.h, KeyFrame.h, MapPoint.h, Map.h.
//
// What runs where: every method walks the pointer graph exactly as the reference does (which map points, validity tests,
// projection geometry with the reference's float / double mix, the mutations Replace / AddObservation / SetPose /
// EraseObservation under the reference's lock scopes) and hands the data-parallel part - frame grid, window candidates,
// Hamming distances; residuals, Jacobians, Schur complement, MFMA Cholesky - to the HIP library in ONE call per method.
// Only element access is used on the math types (M(i, j), v[i]); nothing here needs Eigen to compile.
// ============================================================================
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/orbslam_hip.h"

namespace ORB_SLAM2 {
namespace dropin {

inline void check(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + " failed: " + orbhip_last_error());
}

struct P3 { double x, y, z; };
template <class V> inline P3 p3(const V& v) { return {v[0], v[1], v[2]}; }
// R (3x3 block of any matrix type, row r0 / col c0) * p + t, plain left-to-right double arithmetic
template <class M> inline P3 rot(const M& R, const P3& p) {
  return {R(0, 0) * p.x + R(0, 1) * p.y + R(0, 2) * p.z, R(1, 0) * p.x + R(1, 1) * p.y + R(1, 2) * p.z, R(2, 0) * p.x + R(2, 1) * p.y + R(2, 2) * p.z};
}
inline P3 add(const P3& a, const P3& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline P3 sub(const P3& a, const P3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline double dot(const P3& a, const P3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline double norm(const P3& a) { return std::sqrt(dot(a, a)); }
struct R33 { double m[3][3]; double operator()(int r, int c) const { return m[r][c]; } };
template <class M> inline R33 block33(const M& T) { R33 R; for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.m[r][c] = T(r, c); return R; }
template <class M> inline P3 col3(const M& T) { return {T(0, 3), T(1, 3), T(2, 3)}; }
inline P3 rot_t(const R33& R, const P3& p) {   // R^T p
  return {R.m[0][0] * p.x + R.m[1][0] * p.y + R.m[2][0] * p.z, R.m[0][1] * p.x + R.m[1][1] * p.y + R.m[2][1] * p.z, R.m[0][2] * p.x + R.m[1][2] * p.y + R.m[2][2] * p.z};
}

// flattened view of one frame / keyframe: what the C ABI takes
struct Flat {
  std::vector<float> kps4; const uint8_t* desc = nullptr; int n = 0; float bounds[4] = {0, 0, 0, 0};
  std::vector<uint8_t> desc_store;
};
template <class F> inline void flatten(const F& f, Flat* o) {          // Frame& or KeyFrame&
  o->n = (int)f.undistort_keypoints_.size();
  o->kps4.resize(4 * (size_t)o->n);
  for (int i = 0; i < o->n; i++) {
    const auto& kp = f.undistort_keypoints_[i];
    o->kps4[4 * i] = kp.pt.x; o->kps4[4 * i + 1] = kp.pt.y; o->kps4[4 * i + 2] = (float)kp.octave; o->kps4[4 * i + 3] = kp.angle;
  }
  o->desc_store.resize(32 * (size_t)o->n);                               // (cv::Mat rows may be padded: copy row by row)
  for (int i = 0; i < o->n; i++) std::memcpy(&o->desc_store[32 * (size_t)i], f.descriptors_.ptr(i), 32);
  o->desc = o->desc_store.data();
  o->bounds[0] = (float)f.min_x_; o->bounds[1] = (float)f.max_x_; o->bounds[2] = (float)f.min_y_; o->bounds[3] = (float)f.max_y_;
}
// DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned int>>) -> ascending node ids + CSR lists
struct FlatFV { std::vector<uint32_t> node, off{0}, idx; };
template <class FV> inline void flatten_fv(const FV& fv, FlatFV* o) {
  for (auto it = fv.begin(); it != fv.end(); ++it) {
    o->node.push_back((uint32_t)it->first);
    for (auto v : it->second) o->idx.push_back((uint32_t)v);
    o->off.push_back((uint32_t)o->idx.size());
  }
}
// per-query arrays of the projection engine
struct Queries {
  std::vector<float> uv, radius, angle; std::vector<int32_t> lo, hi, pred; std::vector<uint8_t> valid, desc;
  explicit Queries(size_t n) : uv(2 * n, 0.f), radius(n, 0.f), angle(n, 0.f), lo(n, -1), hi(n, -1), pred(n, -1), valid(n, 0), desc(32 * n, 0) {}
  template <class MatT> void set_desc(size_t q, const MatT& d) { std::memcpy(&desc[32 * q], d.ptr(0), 32); }
};
// an owned copy of row r: m.row(r).clone() for cv::Mat (row() shares the keyframe's storage), m.row(r) where row() already copies
template <class M> inline auto row_copy(const M& m, int r, int) -> decltype(m.row(r).clone()) { return m.row(r).clone(); }
template <class M> inline M row_copy(const M& m, int r, long) { return m.row(r); }

}  // namespace dropin

// ============================================================================================== ORBmatcher
template <class Types>
class ORBmatcherT {
 public:
  typedef typename Types::Frame Frame;
  typedef typename Types::KeyFrame KeyFrame;
  typedef typename Types::MapPoint MapPoint;
  typedef typename Types::Map Map;
  typedef typename Types::Matrix3d Matrix3d;
  typedef typename Types::Matrix4d Matrix4d;
  typedef typename Types::Vector3d Vector3d;
  typedef typename Types::Mat Mat;
  typedef typename Types::Point2f Point2f;

  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;        // src/ORBmatcher.cc:35-37

  ORBmatcherT(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

  // src/ORBmatcher.cc:1422-1437
  static int DescriptorDistance(const Mat& a, const Mat& b) { return orbm_descriptor_distance(a.ptr(0), b.ptr(0)); }

  // ---- Tracking::SearchLocalPoints (src/Tracking.cc:834), src/ORBmatcher.cc:42-119 -------------------------------------
  int SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th = 3) {
    using namespace dropin;
    const bool bFactor = th != 1.0;
    const size_t nq = vpMapPoints.size();
    Queries Q(nq);
    for (size_t iMP = 0; iMP < nq; iMP++) {
      MapPoint* pMP = vpMapPoints[iMP];
      if (!pMP->is_track_in_view_) continue;
      if (pMP->isBad()) continue;
      const int nPredictedLevel = pMP->track_scale_level_;
      float r = RadiusByViewingCos(pMP->track_view_cos_);
      if (bFactor) r *= th;
      Q.valid[iMP] = pMP->Observations() > 0 ? 1 : 3;          // (3: once assigned, the feature stays open for later points, ":83-84")
      Q.uv[2 * iMP] = pMP->track_proj_x_; Q.uv[2 * iMP + 1] = pMP->track_proj_y_;
      Q.radius[iMP] = r * F.scale_factors_[nPredictedLevel];
      Q.lo[iMP] = nPredictedLevel - 1; Q.hi[iMP] = nPredictedLevel;
      Q.set_desc(iMP, pMP->GetDescriptor());
    }
    Flat T; flatten(F, &T);
    std::vector<uint8_t> taken(T.n, 0);                       // F.map_points_[idx] holds a point with observations (":83-84")
    for (int i = 0; i < T.n; i++) taken[i] = (F.map_points_[i] && F.map_points_[i]->Observations() > 0) ? 1 : 0;
    std::vector<int32_t> match(nq ? nq : 1, -1);
    int nmatches = 0;
    check(orbm_search_by_projection(T.kps4.data(), T.desc, T.n, T.bounds, Q.uv.data(), Q.radius.data(), Q.lo.data(), Q.hi.data(), nullptr, Q.desc.data(),
                                    Q.valid.data(), nullptr, (int)nq, nullptr, 0.f, taken.data(), 1, mfNNratio, TH_HIGH, 0, match.data(), nullptr, &nmatches),
          "orbm_search_by_projection");
    for (size_t iMP = 0; iMP < nq; iMP++) if (match[iMP] >= 0) F.map_points_[match[iMP]] = vpMapPoints[iMP];
    return nmatches;
  }

  // ---- Tracking::TrackWithMotionModel (src/Tracking.cc:632,638), src/ORBmatcher.cc:1161-1271 ---------------------------
  int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th) {
    using namespace dropin;
    const R33 Rcw = block33(CurrentFrame.Tcw_); const P3 tcw = col3(CurrentFrame.Tcw_);
    const size_t nq = (size_t)LastFrame.N_;
    Queries Q(nq);
    for (size_t i = 0; i < nq; i++) {
      MapPoint* map_point = LastFrame.map_points_[i];
      if (!map_point || LastFrame.is_outliers_[i]) continue;
      const P3 x3Dc = add(rot(Rcw, p3(map_point->GetWorldPos())), tcw);
      const float xc = x3Dc.x, yc = x3Dc.y;
      const float invzc = 1.0 / x3Dc.z;
      if (invzc < 0) continue;
      const float u = CurrentFrame.fx_ * xc * invzc + CurrentFrame.cx_;
      const float v = CurrentFrame.fy_ * yc * invzc + CurrentFrame.cy_;
      if (u < CurrentFrame.min_x_ || u > CurrentFrame.max_x_) continue;
      if (v < CurrentFrame.min_y_ || v > CurrentFrame.max_y_) continue;
      const int nLastOctave = LastFrame.keypoints_[i].octave;
      Q.valid[i] = map_point->Observations() > 0 ? 1 : 3;      // (":1220-1221" looks at the point assigned earlier in this loop, too)
      Q.uv[2 * i] = u; Q.uv[2 * i + 1] = v;
      Q.radius[i] = th * CurrentFrame.scale_factors_[nLastOctave];
      Q.lo[i] = nLastOctave - 1; Q.hi[i] = nLastOctave + 1;
      Q.angle[i] = LastFrame.undistort_keypoints_[i].angle;
      Q.set_desc(i, map_point->GetDescriptor());
    }
    Flat T; flatten(CurrentFrame, &T);
    std::vector<uint8_t> taken(T.n, 0);
    for (int i = 0; i < T.n; i++) taken[i] = (CurrentFrame.map_points_[i] && CurrentFrame.map_points_[i]->Observations() > 0) ? 1 : 0;
    std::vector<int32_t> match(nq ? nq : 1, -1);
    int nmatches = 0;
    check(orbm_search_by_projection(T.kps4.data(), T.desc, T.n, T.bounds, Q.uv.data(), Q.radius.data(), Q.lo.data(), Q.hi.data(), nullptr, Q.desc.data(),
                                    Q.valid.data(), Q.angle.data(), (int)nq, nullptr, 0.f, taken.data(), 0, mfNNratio, TH_HIGH, mbCheckOrientation ? 1 : 0,
                                    match.data(), nullptr, &nmatches), "orbm_search_by_projection");
    // the reference assigns in query order (":1232") and then resets the slots of the removed rotation bins (":1260-1264"):
    // a slot that held a point without observations, or that two queries shared, ends as nullptr when ANY of its matches is removed
    for (size_t i = 0; i < nq; i++) {
      if (match[i] >= 0) CurrentFrame.map_points_[match[i]] = LastFrame.map_points_[i];
      else if (match[i] <= -2) CurrentFrame.map_points_[-2 - match[i]] = LastFrame.map_points_[i];
    }
    for (size_t i = 0; i < nq; i++) if (match[i] <= -2) CurrentFrame.map_points_[-2 - match[i]] = static_cast<MapPoint*>(nullptr);
    return nmatches;
  }

  // ---- Tracking::Relocalization (src/Tracking.cc:1085,1101), src/ORBmatcher.cc:1273-1384 -------------------------------
  int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, const float th, const int ORBdist) {
    using namespace dropin;
    const R33 Rcw = block33(CurrentFrame.Tcw_); const P3 tcw = col3(CurrentFrame.Tcw_);
    const P3 Rt = rot_t(Rcw, tcw); const P3 Ow = {-Rt.x, -Rt.y, -Rt.z};
    const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
    const size_t nq = vpMPs.size();
    Queries Q(nq);
    for (size_t i = 0; i < nq; i++) {
      MapPoint* pMP = vpMPs[i];
      if (!pMP || pMP->isBad() || sAlreadyFound.count(pMP)) continue;
      const P3 x3Dw = p3(pMP->GetWorldPos());
      const P3 x3Dc = add(rot(Rcw, x3Dw), tcw);
      const float xc = x3Dc.x, yc = x3Dc.y;
      const float invzc = 1.0 / x3Dc.z;
      const float u = CurrentFrame.fx_ * xc * invzc + CurrentFrame.cx_;
      const float v = CurrentFrame.fy_ * yc * invzc + CurrentFrame.cy_;
      if (u < CurrentFrame.min_x_ || u > CurrentFrame.max_x_) continue;
      if (v < CurrentFrame.min_y_ || v > CurrentFrame.max_y_) continue;
      float dist3D = norm(sub(x3Dw, Ow));
      const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
      if (dist3D < minDistance || dist3D > maxDistance) continue;
      const int nPredictedLevel = pMP->PredictScale(dist3D, &CurrentFrame);
      Q.valid[i] = 1; Q.uv[2 * i] = u; Q.uv[2 * i + 1] = v;
      Q.radius[i] = th * CurrentFrame.scale_factors_[nPredictedLevel];
      Q.lo[i] = nPredictedLevel - 1; Q.hi[i] = nPredictedLevel + 1;
      Q.angle[i] = pKF->undistort_keypoints_[i].angle;
      Q.set_desc(i, pMP->GetDescriptor());
    }
    Flat T; flatten(CurrentFrame, &T);
    std::vector<uint8_t> taken(T.n, 0);
    for (int i = 0; i < T.n; i++) taken[i] = CurrentFrame.map_points_[i] ? 1 : 0;          // (":1336": any map point closes the feature)
    std::vector<int32_t> match(nq ? nq : 1, -1);
    int nmatches = 0;
    check(orbm_search_by_projection(T.kps4.data(), T.desc, T.n, T.bounds, Q.uv.data(), Q.radius.data(), Q.lo.data(), Q.hi.data(), nullptr, Q.desc.data(),
                                    Q.valid.data(), Q.angle.data(), (int)nq, nullptr, 0.f, taken.data(), 0, mfNNratio, ORBdist, mbCheckOrientation ? 1 : 0,
                                    match.data(), nullptr, &nmatches), "orbm_search_by_projection");
    // (every candidate slot was empty, ":1336", so a removed match leaves nullptr behind: assign only the kept ones)
    for (size_t i = 0; i < nq; i++) if (match[i] >= 0) CurrentFrame.map_points_[match[i]] = vpMPs[i];
    return nmatches;
  }

  // ---- LoopClosing::ComputeSim3 (src/LoopClosing.cc:374), src/ORBmatcher.cc:258-361 ------------------------------------
  int SearchByProjection(KeyFrame* pKF, const Matrix4d& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th) {
    using namespace dropin;
    Sim3Cam C = decompose(Scw);
    std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPoint*>(nullptr));
    const size_t nq = vpPoints.size();
    Queries Q(nq);
    for (size_t iMP = 0; iMP < nq; iMP++) {
      MapPoint* pMP = vpPoints[iMP];
      if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
      float u, v, dist; int level;
      if (!project_with_gates(pKF, C, pMP, 0.0, true, &u, &v, &dist, &level)) continue;
      Q.valid[iMP] = 1; Q.uv[2 * iMP] = u; Q.uv[2 * iMP + 1] = v;
      Q.radius[iMP] = th * pKF->scale_factors_[level];
      Q.pred[iMP] = level;
      Q.set_desc(iMP, pMP->GetDescriptor());
    }
    Flat T; flatten(*pKF, &T);
    std::vector<uint8_t> taken(T.n, 0);
    for (int i = 0; i < T.n && i < (int)vpMatched.size(); i++) taken[i] = vpMatched[i] ? 1 : 0;
    std::vector<int32_t> match(nq ? nq : 1, -1);
    int nmatches = 0;
    check(orbm_search_by_projection(T.kps4.data(), T.desc, T.n, T.bounds, Q.uv.data(), Q.radius.data(), nullptr, nullptr, Q.pred.data(), Q.desc.data(),
                                    Q.valid.data(), nullptr, (int)nq, nullptr, 0.f, taken.data(), 0, mfNNratio, TH_LOW, 0, match.data(), nullptr, &nmatches),
          "orbm_search_by_projection");
    for (size_t iMP = 0; iMP < nq; iMP++) if (match[iMP] >= 0) vpMatched[match[iMP]] = vpPoints[iMP];
    return nmatches;
  }

  // ---- Tracking::TrackReferenceKeyFrame / Relocalization (src/Tracking.cc:576,1019), src/ORBmatcher.cc:151-256 ----------
  int SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) {
    using namespace dropin;
    const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
    vpMapPointMatches = std::vector<MapPoint*>(F.N_, static_cast<MapPoint*>(nullptr));
    Flat A, B; flatten(*pKF, &A); flatten(F, &B);
    std::vector<uint8_t> valid1(A.n, 0);
    std::vector<float> a1(A.n), a2(B.n);
    for (int i = 0; i < A.n; i++) { MapPoint* p = i < (int)vpMapPointsKF.size() ? vpMapPointsKF[i] : nullptr; valid1[i] = (p && !p->isBad()) ? 1 : 0; a1[i] = pKF->undistort_keypoints_[i].angle; }
    for (int i = 0; i < B.n; i++) a2[i] = F.keypoints_[i].angle;                         // (":221": the frame's raw keypoint angle)
    FlatFV f1, f2; flatten_fv(pKF->feature_vector_, &f1); flatten_fv(F.feature_vector_, &f2);
    std::vector<int32_t> m12(A.n ? A.n : 1, -1);
    int nmatches = 0;
    check(orbm_search_by_bow(A.desc, A.n, valid1.data(), a1.data(), B.desc, B.n, nullptr, a2.data(), f1.node.data(), f1.off.data(), f1.idx.data(), (int)f1.node.size(),
                             f2.node.data(), f2.off.data(), f2.idx.data(), (int)f2.node.size(), mfNNratio, TH_LOW, 0, mbCheckOrientation ? 1 : 0, m12.data(), &nmatches),
          "orbm_search_by_bow");
    for (int i = 0; i < A.n; i++) if (m12[i] >= 0) vpMapPointMatches[m12[i]] = vpMapPointsKF[i];
    return nmatches;
  }

  // ---- LoopClosing::ComputeSim3 (src/LoopClosing.cc:262), src/ORBmatcher.cc:470-580 ------------------------------------
  int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12) {
    using namespace dropin;
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    vpMatches12 = std::vector<MapPoint*>(vpMapPoints1.size(), static_cast<MapPoint*>(nullptr));
    Flat A, B; flatten(*pKF1, &A); flatten(*pKF2, &B);
    std::vector<uint8_t> valid1(A.n, 0), valid2(B.n, 0);
    std::vector<float> a1(A.n), a2(B.n);
    for (int i = 0; i < A.n; i++) { MapPoint* p = i < (int)vpMapPoints1.size() ? vpMapPoints1[i] : nullptr; valid1[i] = (p && !p->isBad()) ? 1 : 0; a1[i] = pKF1->undistort_keypoints_[i].angle; }
    for (int i = 0; i < B.n; i++) { MapPoint* p = i < (int)vpMapPoints2.size() ? vpMapPoints2[i] : nullptr; valid2[i] = (p && !p->isBad()) ? 1 : 0; a2[i] = pKF2->undistort_keypoints_[i].angle; }
    FlatFV f1, f2; flatten_fv(pKF1->feature_vector_, &f1); flatten_fv(pKF2->feature_vector_, &f2);
    std::vector<int32_t> m12(A.n ? A.n : 1, -1);
    int nmatches = 0;
    check(orbm_search_by_bow(A.desc, A.n, valid1.data(), a1.data(), B.desc, B.n, valid2.data(), a2.data(), f1.node.data(), f1.off.data(), f1.idx.data(),
                             (int)f1.node.size(), f2.node.data(), f2.off.data(), f2.idx.data(), (int)f2.node.size(), mfNNratio, TH_LOW, 1,
                             mbCheckOrientation ? 1 : 0, m12.data(), &nmatches), "orbm_search_by_bow");
    for (int i = 0; i < A.n && i < (int)vpMatches12.size(); i++) if (m12[i] >= 0) vpMatches12[i] = vpMapPoints2[m12[i]];
    return nmatches;
  }

  // ---- Tracking::MonocularInitialization (src/Tracking.cc:416), src/ORBmatcher.cc:363-468 ------------------------------
  int SearchForInitialization(Frame& F1, Frame& F2, std::vector<Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10) {
    using namespace dropin;
    Flat A, B; flatten(F1, &A); flatten(F2, &B);
    std::vector<float> pm(2 * (size_t)A.n);
    for (int i = 0; i < A.n; i++) { pm[2 * i] = vbPrevMatched[i].x; pm[2 * i + 1] = vbPrevMatched[i].y; }
    vnMatches12 = std::vector<int>(A.n, -1);
    std::vector<int32_t> m(A.n ? A.n : 1, -1);
    int nmatches = 0;
    check(orbm_search_for_initialization(A.kps4.data(), A.desc, A.n, B.kps4.data(), B.desc, B.n, B.bounds, pm.data(), windowSize, mfNNratio,
                                         mbCheckOrientation ? 1 : 0, m.data(), &nmatches), "orbm_search_for_initialization");
    for (int i = 0; i < A.n; i++) { vnMatches12[i] = m[i]; vbPrevMatched[i].x = pm[2 * i]; vbPrevMatched[i].y = pm[2 * i + 1]; }
    return nmatches;
  }

  // ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:250), src/ORBmatcher.cc:582-722 (monocular) ---------------
  int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Matrix3d& F12, std::vector<std::pair<size_t, size_t> >& vMatchedPairs, const bool bOnlyStereo) {
    using namespace dropin;
    vMatchedPairs.clear();
    if (bOnlyStereo) return 0;                                   // no feature of a monocular keyframe has a right coordinate (":626-629")
    // epipole in the second image (":589-596")
    const P3 Cw = p3(pKF1->GetCameraCenter());
    const Matrix3d R2w = pKF2->GetRotation();
    const P3 C2 = add(rot(R2w, Cw), p3(pKF2->GetTranslation()));
    const float invz = 1.0f / C2.z;
    const float ex = pKF2->fx_ * C2.x * invz + pKF2->cx_;
    const float ey = pKF2->fy_ * C2.y * invz + pKF2->cy_;
    Flat A, B; flatten(*pKF1, &A); flatten(*pKF2, &B);
    std::vector<uint8_t> um1(A.n), um2(B.n);
    for (int i = 0; i < A.n; i++) um1[i] = pKF1->GetMapPoint(i) ? 0 : 1;
    for (int i = 0; i < B.n; i++) um2[i] = pKF2->GetMapPoint(i) ? 0 : 1;
    FlatFV f1, f2; flatten_fv(pKF1->feature_vector_, &f1); flatten_fv(pKF2->feature_vector_, &f2);
    double F[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) F[3 * r + c] = F12(r, c);
    std::vector<int32_t> m12(A.n ? A.n : 1, -1);
    int nmatches = 0;
    check(orbm_search_for_triangulation(A.kps4.data(), A.desc, um1.data(), A.n, B.kps4.data(), B.desc, um2.data(), B.n, f1.node.data(), f1.off.data(), f1.idx.data(),
                                        (int)f1.node.size(), f2.node.data(), f2.off.data(), f2.idx.data(), (int)f2.node.size(), F, ex, ey,
                                        pKF2->scale_factors_.data(), pKF2->level_sigma2s_.data(), mbCheckOrientation ? 1 : 0, m12.data(), &nmatches),
          "orbm_search_for_triangulation");
    vMatchedPairs.reserve(nmatches);
    for (int i = 0; i < A.n; i++) if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
    return nmatches;
  }

  // ---- LoopClosing::ComputeSim3 (src/LoopClosing.cc:319), src/ORBmatcher.cc:956-1159 -----------------------------------
  int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const Matrix3d& R12, const Vector3d& t12, const float th) {
    using namespace dropin;
    const Matrix3d R1w = pKF1->GetRotation(), R2w = pKF2->GetRotation();
    const P3 t1w = p3(pKF1->GetTranslation()), t2w = p3(pKF2->GetTranslation());
    R33 sR12, sR21;                                              // sR12 = s12 * R12, sR21 = (1 / s12) * R12^T  (":973-975")
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { sR12.m[r][c] = s12 * R12(r, c); sR21.m[r][c] = (1.0 / s12) * R12(c, r); }
    const P3 t12p = p3(t12);
    const P3 t21r = rot(sR21, t12p); const P3 t21 = {-t21r.x, -t21r.y, -t21r.z};
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const int N1 = (int)vpMapPoints1.size(), N2 = (int)vpMapPoints2.size();
    std::vector<bool> vbAlreadyMatched1(N1, false), vbAlreadyMatched2(N2, false);
    for (int i = 0; i < N1; i++) {
      MapPoint* pMP = vpMatches12[i];
      if (pMP) {
        vbAlreadyMatched1[i] = true;
        const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
        if (idx2 >= 0 && idx2 < N2) vbAlreadyMatched2[idx2] = true;
      }
    }
    Flat A, B; flatten(*pKF1, &A); flatten(*pKF2, &B);
    Queries Q12(N1), Q21(N2);
    auto one_way = [&](const std::vector<MapPoint*>& pts, const std::vector<bool>& already, const Matrix3d& Raw, const P3& taw, const R33& sRba, const P3& tba,
                       KeyFrame* target, Queries& Q) {
      for (size_t i = 0; i < pts.size(); i++) {
        MapPoint* pMP = pts[i];
        if (!pMP || already[i]) continue;
        if (pMP->isBad()) continue;
        const P3 p3Dca = add(rot(Raw, p3(pMP->GetWorldPos())), taw);
        const P3 p3Dcb = add(rot(sRba, p3Dca), tba);
        if (p3Dcb.z < 0.0) continue;
        const float invz = 1.0 / p3Dcb.z;
        const float x = p3Dcb.x * invz, y = p3Dcb.y * invz;
        const float u = pKF1->fx_ * x + pKF1->cx_, v = pKF1->fy_ * y + pKF1->cy_;          // (both directions use keyframe 1's intrinsics, ":958-961")
        if (!target->IsInImage(u, v)) continue;
        const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
        const float dist3D = norm(p3Dcb);
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        const int nPredictedLevel = pMP->PredictScale(dist3D, target);
        Q.valid[i] = 1; Q.uv[2 * i] = u; Q.uv[2 * i + 1] = v;
        Q.radius[i] = th * target->scale_factors_[nPredictedLevel];
        Q.pred[i] = nPredictedLevel;
        Q.set_desc(i, pMP->GetDescriptor());
      }
    };
    one_way(vpMapPoints1, vbAlreadyMatched1, R1w, t1w, sR21, t21, pKF2, Q12);
    one_way(vpMapPoints2, vbAlreadyMatched2, R2w, t2w, sR12, t12p, pKF1, Q21);
    // the descriptor rows the C ABI searches with are the MAP POINTS' descriptors (":1036", ":1112"), not the keyframes' own
    std::vector<int32_t> m12(N1 ? N1 : 1, -1);
    int nFound = 0;
    check(orbm_search_by_sim3(A.kps4.data(), A.desc, N1, B.kps4.data(), B.desc, N2, A.bounds, B.bounds, Q12.uv.data(), Q12.radius.data(), Q12.pred.data(),
                              Q12.valid.data(), Q12.desc.data(), Q21.uv.data(), Q21.radius.data(), Q21.pred.data(), Q21.valid.data(), Q21.desc.data(),
                              m12.data(), &nFound), "orbm_search_by_sim3");
    for (int i1 = 0; i1 < N1; i1++) if (m12[i1] >= 0) vpMatches12[i1] = vpMapPoints2[m12[i1]];
    return nFound;
  }

  // ---- LocalMapping::SearchInNeighbors (src/LocalMapping.cc:441,472), src/ORBmatcher.cc:724-842 --------------------------
  int Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th = 3.0) {
    using namespace dropin;
    Sim3Cam C;
    C.R = block33(pKF->GetRotation()); C.t = p3(pKF->GetTranslation()); C.Ow = p3(pKF->GetCameraCenter());
    const size_t nq = vpMapPoints.size();
    Queries Q(nq);
    // candidate selection does not depend on the map mutations below (no `taken` state, ":775-811"): it is computed for
    // every non-null point first; validity (isBad / IsInKeyFrame) is evaluated in the sequential pass, where it can change
    for (size_t i = 0; i < nq; i++) {
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP) continue;
      float u, v, dist; int level;
      if (!project_with_gates(pKF, C, pMP, 0.0f, true, &u, &v, &dist, &level)) continue;
      Q.valid[i] = 1; Q.uv[2 * i] = u; Q.uv[2 * i + 1] = v;
      Q.radius[i] = th * pKF->scale_factors_[level];
      Q.pred[i] = level;
      Q.set_desc(i, pMP->GetDescriptor());
    }
    Flat T; flatten(*pKF, &T);
    std::vector<int32_t> match(nq ? nq : 1, -1);
    int n = 0;
    check(orbm_search_by_projection(T.kps4.data(), T.desc, T.n, T.bounds, Q.uv.data(), Q.radius.data(), nullptr, nullptr, Q.pred.data(), Q.desc.data(),
                                    Q.valid.data(), nullptr, (int)nq, pKF->inv_level_sigma2s_.data(), 5.99f, nullptr, 0, mfNNratio, TH_LOW, 0, match.data(), nullptr, &n),
          "orbm_search_by_projection");
    int nFused = 0;
    for (size_t i = 0; i < nq; i++) {
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP) continue;
      if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
      if (match[i] < 0) continue;
      const int bestIdx = match[i];
      MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
          else pMPinKF->Replace(pMP);
        }
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
    return nFused;
  }

  // ---- LocalMapping::SearchInNeighbors, the loop `for (target keyframes) matcher.Fuse(neighbor_keyframe, map_point_matches)`
  //      (src/LocalMapping.cc:437-442) with the candidate selection of ALL target keyframes in ONE call (orbl_fuse_batch, round 5).
  // The projection and its gates are evaluated per (keyframe, point) up front - they read only what no Fuse changes (poses,
  // positions, normals, distance bounds) - the validity tests (NULL / isBad / IsInKeyFrame) and the Replace / AddObservation
  // mutation run keyframe after keyframe in the reference's order.  What a mutation CAN change for a later keyframe is a point's
  // descriptor (MapPoint::Replace ends with ComputeDistinctiveDescriptors on the survivor, src/MapPoint.cc:230): a point whose
  // descriptor no longer equals the one the batch searched with is searched again, alone, for the keyframe at hand.
  // Returns the per-keyframe return values of Fuse.
  std::vector<int> Fuse(const std::vector<KeyFrame*>& targets, const std::vector<MapPoint*>& vpMapPoints, const float th = 3.0) {
    using namespace dropin;
    const size_t nt = targets.size(), nq = vpMapPoints.size();
    std::vector<int> ret(nt, 0);
    if (!nt || !nq) return ret;
    // orbl_fuse_batch takes ONE inv_level_sigma2 table; keyframes of differently configured extractors (the reference reads each
    // keyframe's own table, src/ORBmatcher.cc:789) keep the reference's loop of single calls
    for (size_t t = 1; t < nt; t++)
      if (targets[t]->inv_level_sigma2s_ != targets[0]->inv_level_sigma2s_) {
        for (size_t k = 0; k < nt; k++) ret[k] = Fuse(targets[k], vpMapPoints, th);
        return ret;
      }
    std::vector<float> uv(2 * nt * nq, 0.f), radius(nt * nq, 0.f); std::vector<int32_t> level(nt * nq, -1);
    std::vector<uint8_t> desc(32 * nq, 0);
    for (size_t i = 0; i < nq; i++) if (vpMapPoints[i]) std::memcpy(&desc[32 * i], vpMapPoints[i]->GetDescriptor().ptr(0), 32);
    std::vector<Flat> T(nt); std::vector<orbl_fuse_keyframe> kf(nt);
    for (size_t t = 0; t < nt; t++) {
      KeyFrame* pKF = targets[t];
      Sim3Cam C;
      C.R = block33(pKF->GetRotation()); C.t = p3(pKF->GetTranslation()); C.Ow = p3(pKF->GetCameraCenter());
      for (size_t i = 0; i < nq; i++) {
        MapPoint* pMP = vpMapPoints[i];
        if (!pMP) continue;
        float u, v, dist; int lv;
        if (!project_with_gates(pKF, C, pMP, 0.0f, true, &u, &v, &dist, &lv)) continue;
        const size_t e = t * nq + i;
        uv[2 * e] = u; uv[2 * e + 1] = v; radius[e] = th * pKF->scale_factors_[lv]; level[e] = lv;
      }
      flatten(*pKF, &T[t]);
      kf[t].kps = T[t].kps4.data(); kf[t].desc = T[t].desc; kf[t].n = T[t].n;
      for (int k = 0; k < 4; k++) kf[t].bounds[k] = T[t].bounds[k];
    }
    std::vector<int32_t> best_idx(nt * nq, -1), best_dist(nt * nq, 256);
    check(orbl_fuse_batch(kf.data(), (int)nt, uv.data(), radius.data(), level.data(), (int)nq, desc.data(), targets[0]->inv_level_sigma2s_.data(),
                          (int)targets[0]->inv_level_sigma2s_.size(), best_idx.data(), best_dist.data()), "orbl_fuse_batch");
    for (size_t t = 0; t < nt; t++) {
      KeyFrame* pKF = targets[t];
      int nFused = 0;
      for (size_t i = 0; i < nq; i++) {
        MapPoint* pMP = vpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        const size_t e = t * nq + i;
        if (level[e] < 0) continue;
        int bestIdx = best_idx[e], bestDist = best_dist[e];
        if (std::memcmp(&desc[32 * i], pMP->GetDescriptor().ptr(0), 32) != 0) {      // the descriptor changed since the batch: this point, this keyframe, again
          Queries Q(1);
          Q.valid[0] = 1; Q.uv[0] = uv[2 * e]; Q.uv[1] = uv[2 * e + 1]; Q.radius[0] = radius[e]; Q.pred[0] = level[e];
          Q.set_desc(0, pMP->GetDescriptor());
          int32_t m1 = -1, d1 = 256; int n1 = 0;
          check(orbm_search_by_projection(T[t].kps4.data(), T[t].desc, T[t].n, T[t].bounds, Q.uv.data(), Q.radius.data(), nullptr, nullptr, Q.pred.data(), Q.desc.data(),
                                          Q.valid.data(), nullptr, 1, pKF->inv_level_sigma2s_.data(), 5.99f, nullptr, 0, mfNNratio, 256, 0, &m1, &d1, &n1),
                "orbm_search_by_projection");
          bestIdx = m1; bestDist = d1;
        }
        if (bestIdx < 0 || bestDist > TH_LOW) continue;
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
          if (!pMPinKF->isBad()) {
            if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
            else pMPinKF->Replace(pMP);
          }
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
      }
      ret[t] = nFused;
    }
    return ret;
  }

  // ---- LoopClosing::SearchAndFuse (src/LoopClosing.cc:611), src/ORBmatcher.cc:844-954 ------------------------------------
  int Fuse(KeyFrame* pKF, Matrix4d Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint) {
    using namespace dropin;
    Sim3Cam C = decompose(Scw);
    const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();
    const size_t nq = vpPoints.size();
    Queries Q(nq);
    for (size_t iMP = 0; iMP < nq; iMP++) {
      MapPoint* pMP = vpPoints[iMP];
      if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
      float u, v, dist; int level;
      if (!project_with_gates(pKF, C, pMP, 0.0f, true, &u, &v, &dist, &level)) continue;
      Q.valid[iMP] = 1; Q.uv[2 * iMP] = u; Q.uv[2 * iMP + 1] = v;
      Q.radius[iMP] = th * pKF->scale_factors_[level];
      Q.pred[iMP] = level;
      Q.set_desc(iMP, pMP->GetDescriptor());
    }
    Flat T; flatten(*pKF, &T);
    std::vector<int32_t> match(nq ? nq : 1, -1);
    int n = 0;
    check(orbm_search_by_projection(T.kps4.data(), T.desc, T.n, T.bounds, Q.uv.data(), Q.radius.data(), nullptr, nullptr, Q.pred.data(), Q.desc.data(),
                                    Q.valid.data(), nullptr, (int)nq, nullptr, 0.f, nullptr, 0, mfNNratio, TH_LOW, 0, match.data(), nullptr, &n),
          "orbm_search_by_projection");
    int nFused = 0;
    for (size_t iMP = 0; iMP < nq; iMP++) {
      if (match[iMP] < 0) continue;
      MapPoint* pMP = vpPoints[iMP];
      MapPoint* pMPinKF = pKF->GetMapPoint(match[iMP]);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, match[iMP]);
        pKF->AddMapPoint(pMP, match[iMP]);
      }
      nFused++;
    }
    return nFused;
  }

  // ---- LoopClosing::SearchAndFuse, the whole loop (src/LoopClosing.cc:599-630):
  //        for (corrected keyframes) { matcher.Fuse(keyframe, Scw, loop_map_points_, 4, replace); lock map; for (i) if (replace[i]) replace[i]->Replace(loop_map_points_[i]); }
  //      with the candidate selection of ALL keyframes in ONE call (orbl_fuse_batch_sim3, round 6).  Projection and gates are evaluated per
  //      (keyframe, point) up front - they read what no Fuse / Replace changes (the corrected Sim(3), positions, normals, distance bounds) -;
  //      what a keyframe's turn CAN see of the turns before it is re-read when its turn comes: isBad (a loop point that was itself some
  //      keyframe's duplicate has been replaced), GetMapPoints() (Replace hands the replaced point's observations to the loop point: a
  //      later keyframe may already hold it), GetMapPoint(bestIdx), and the loop point's descriptor (Replace ends with
  //      ComputeDistinctiveDescriptors on the survivor, src/MapPoint.cc:230): a point whose descriptor no longer equals the one the
  //      batch searched with is searched again, alone, for the keyframe at hand.  `corrected` in the reference's iteration order
  //      (KeyFrameAndSim3 is a std::map ordered by keyframe pointer), Scw as Sophus::Sim3d::matrix().  Returns Fuse's value per keyframe.
  std::vector<int> SearchAndFuse(const std::vector<std::pair<KeyFrame*, Matrix4d>>& corrected, const std::vector<MapPoint*>& loop_map_points, Map* map, const float th = 4.0) {
    using namespace dropin;
    const size_t nt = corrected.size(), nq = loop_map_points.size();
    std::vector<int> ret(nt, 0);
    if (!nt || !nq) return ret;
    std::vector<float> uv(2 * nt * nq, 0.f), radius(nt * nq, 0.f); std::vector<int32_t> level(nt * nq, -1);
    std::vector<uint8_t> desc(32 * nq, 0);
    for (size_t i = 0; i < nq; i++) std::memcpy(&desc[32 * i], loop_map_points[i]->GetDescriptor().ptr(0), 32);
    std::vector<Flat> T(nt); std::vector<orbl_fuse_keyframe> kf(nt);
    int n_levels = 1;
    for (size_t t = 0; t < nt; t++) {
      KeyFrame* pKF = corrected[t].first;
      const Sim3Cam C = decompose(corrected[t].second);
      n_levels = std::max(n_levels, (int)pKF->scale_factors_.size());
      for (size_t i = 0; i < nq; i++) {
        float u, v, dist; int lv;
        if (!project_with_gates(pKF, C, loop_map_points[i], 0.0f, true, &u, &v, &dist, &lv)) continue;
        const size_t e = t * nq + i;
        uv[2 * e] = u; uv[2 * e + 1] = v; radius[e] = th * pKF->scale_factors_[lv]; level[e] = lv;
      }
      flatten(*pKF, &T[t]);
      kf[t].kps = T[t].kps4.data(); kf[t].desc = T[t].desc; kf[t].n = T[t].n;
      for (int k = 0; k < 4; k++) kf[t].bounds[k] = T[t].bounds[k];
    }
    std::vector<int32_t> best_idx(nt * nq, -1), best_dist(nt * nq, 256);
    check(orbl_fuse_batch_sim3(kf.data(), (int)nt, uv.data(), radius.data(), level.data(), (int)nq, desc.data(), n_levels, best_idx.data(), best_dist.data()),
          "orbl_fuse_batch_sim3");
    for (size_t t = 0; t < nt; t++) {
      KeyFrame* pKF = corrected[t].first;
      std::vector<MapPoint*> replace_map_points(nq, static_cast<MapPoint*>(nullptr));
      const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();
      int nFused = 0;
      for (size_t i = 0; i < nq; i++) {
        MapPoint* pMP = loop_map_points[i];
        if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
        const size_t e = t * nq + i;
        if (level[e] < 0) continue;
        int bestIdx = best_idx[e], bestDist = best_dist[e];
        if (std::memcmp(&desc[32 * i], pMP->GetDescriptor().ptr(0), 32) != 0) {      // the descriptor changed since the batch: this point, this keyframe, again
          Queries Q(1);
          Q.valid[0] = 1; Q.uv[0] = uv[2 * e]; Q.uv[1] = uv[2 * e + 1]; Q.radius[0] = radius[e]; Q.pred[0] = level[e];
          Q.set_desc(0, pMP->GetDescriptor());
          int32_t m1 = -1, d1 = 256; int n1 = 0;
          check(orbm_search_by_projection(T[t].kps4.data(), T[t].desc, T[t].n, T[t].bounds, Q.uv.data(), Q.radius.data(), nullptr, nullptr, Q.pred.data(), Q.desc.data(),
                                          Q.valid.data(), nullptr, 1, nullptr, 0.f, nullptr, 0, mfNNratio, 256, 0, &m1, &d1, &n1),
                "orbm_search_by_projection");
          bestIdx = m1; bestDist = d1;
        }
        if (bestIdx < 0 || bestDist > TH_LOW) continue;
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
          if (!pMPinKF->isBad()) replace_map_points[i] = pMPinKF;
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
      }
      ret[t] = nFused;
      std::unique_lock<std::mutex> lock(map->mutex_map_update_);     // "Get Map Mutex" (:617)
      for (size_t i = 0; i < nq; i++)
        if (replace_map_points[i]) replace_map_points[i]->Replace(loop_map_points[i]);
    }
    return ret;
  }

 protected:
  float RadiusByViewingCos(const float& viewCos) { return viewCos > 0.998 ? 2.5 : 4.0; }        // src/ORBmatcher.cc:121-126

  struct Sim3Cam { dropin::R33 R; dropin::P3 t, Ow; };
  // "Decompose Scw" (":269-274", ":854-859"): scw from the first row, Rcw = sRcw / scw, tcw = Scw.t / scw, Ow = -Rcw^T tcw
  static Sim3Cam decompose(const Matrix4d& Scw) {
    using namespace dropin;
    Sim3Cam C;
    const R33 sR = block33(Scw);
    const float scw = std::sqrt(sR.m[0][0] * sR.m[0][0] + sR.m[0][1] * sR.m[0][1] + sR.m[0][2] * sR.m[0][2]);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) C.R.m[r][c] = sR.m[r][c] / scw;
    const P3 st = col3(Scw);
    C.t = {st.x / scw, st.y / scw, st.z / scw};
    const P3 Rt = rot_t(C.R, C.t);
    C.Ow = {-Rt.x, -Rt.y, -Rt.z};
    return C;
  }
  // the gates shared by SearchByProjection(KeyFrame*, Scw, ...) and both Fuse overloads (":286-322", ":746-777", ":873-906"):
  // positive depth, inside the image, distance inside the scale-invariance region, viewing angle below 60 degrees
  static bool project_with_gates(KeyFrame* pKF, const Sim3Cam& C, MapPoint* pMP, double, bool viewing_gate, float* u_out, float* v_out, float* dist_out, int* level_out) {
    using namespace dropin;
    const P3 p3Dw = p3(pMP->GetWorldPos());
    const P3 p3Dc = add(rot(C.R, p3Dw), C.t);
    if (p3Dc.z < 0.0) return false;
    const float invz = 1 / p3Dc.z;
    const float x = p3Dc.x * invz, y = p3Dc.y * invz;
    const float u = pKF->fx_ * x + pKF->cx_, v = pKF->fy_ * y + pKF->cy_;
    if (!pKF->IsInImage(u, v)) return false;
    const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
    const P3 PO = sub(p3Dw, C.Ow);
    const float dist = norm(PO);
    if (dist < minDistance || dist > maxDistance) return false;
    if (viewing_gate && dot(PO, p3(pMP->GetNormal())) < 0.5 * dist) return false;
    *u_out = u; *v_out = v; *dist_out = dist;
    *level_out = pMP->PredictScale(dist, pKF);
    return true;
  }

  float mfNNratio;
  bool mbCheckOrientation;
};

// ============================================================================================== CeresOptimizer
template <class Types>
class CeresOptimizerT {
 public:
  typedef typename Types::Frame Frame;
  typedef typename Types::KeyFrame KeyFrame;
  typedef typename Types::MapPoint MapPoint;
  typedef typename Types::Map Map;
  typedef typename Types::Matrix3d Matrix3d;
  typedef typename Types::Matrix4d Matrix4d;
  typedef typename Types::Vector2d Vector2d;
  typedef typename Types::Vector3d Vector3d;
  typedef typename Types::Quaterniond Quaterniond;

  // MatEigenConverter::Matrix4dToMatrix_7_1 / Matrix_7_1_ToMatrix4d (src/MatEigenConverter.cc:66-85)
  static void Matrix4dToMatrix_7_1(const Matrix4d& pose, double out7[7]) {
    double T[16];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T[4 * r + c] = pose(r, c);
    dropin::check(ba_matrix4d_to_pose7(T, out7), "ba_matrix4d_to_pose7");
  }
  static Matrix4d Matrix_7_1_ToMatrix4d(const double in7[7]) {
    double T[16];
    dropin::check(ba_pose7_to_matrix4d(in7, T), "ba_pose7_to_matrix4d");
    Matrix4d pose;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) pose(r, c) = T[4 * r + c];
    return pose;
  }

  // src/CeresOptimizer.cc:227-241
  bool static CheckOutlier(Matrix3d K, Vector2d& observation, float inv_sigma, Vector3d& world_pose, Vector3d& tcw, Quaterniond& qcw, double thres) {
    const double K4[4] = {K(0, 0), K(1, 1), K(0, 2), K(1, 2)};
    const double pose7[7] = {tcw[0], tcw[1], tcw[2], qcw.x(), qcw.y(), qcw.z(), qcw.w()};
    const double X[3] = {world_pose[0], world_pose[1], world_pose[2]}, uv[2] = {observation[0], observation[1]};
    return ba_check_outlier(K4, pose7, X, uv, (double)inv_sigma, thres, nullptr) != 0;
  }

  // src/CeresOptimizer.cc:243-269
  int static CheckOutliers(Frame* frame, Vector3d& tcw, Quaterniond& qcw) {
    int n_bad = 0;
    const double K4[4] = {frame->fx_, frame->fy_, frame->cx_, frame->cy_};
    const double pose7[7] = {tcw[0], tcw[1], tcw[2], qcw.x(), qcw.y(), qcw.z(), qcw.w()};
    for (int i = 0; i < frame->N_; i++) {
      MapPoint* map_point = frame->map_points_[i];
      if (!map_point) continue;
      const Vector3d wp = map_point->GetWorldPos();
      const double X[3] = {wp[0], wp[1], wp[2]};
      const auto& kp = frame->undistort_keypoints_[i];
      const double uv[2] = {kp.pt.x, kp.pt.y};
      const float inv_sigma = frame->inv_level_sigma2s_[kp.octave];
      if (ba_check_outlier(K4, pose7, X, uv, (double)inv_sigma, 5.991, nullptr) != 0) { frame->is_outliers_[i] = true; n_bad++; }
      else frame->is_outliers_[i] = false;
    }
    return n_bad;
  }

  // ---- src/CeresOptimizer.cc:275-342 (Tracking.cc:587,646,684,1074,...) --------------------------------------------------
  int static PoseOptimization(Frame* frame) {
    const int N = frame->N_;
    double pose7[7];
    std::vector<double> Xw, uv; std::vector<float> isg; std::vector<int> slot;
    std::vector<uint8_t> outlier;
    int n_inliers = 0;
    {
      std::unique_lock<std::mutex> lock(MapPoint::global_mutex_);               // (":284")
      Matrix4dToMatrix_7_1(frame->Tcw_, pose7);                                 // frame_tcw, Eigen::Quaterniond(frame_R)
      const double K4[4] = {frame->fx_, frame->fy_, frame->cx_, frame->cy_};
      for (int i = 0; i < N; i++) {
        MapPoint* map_point = frame->map_points_[i];
        if (!map_point) continue;
        frame->is_outliers_[i] = false;
        const Vector3d p = map_point->GetWorldPos();
        const auto& kp = frame->undistort_keypoints_[i];
        Xw.push_back(p[0]); Xw.push_back(p[1]); Xw.push_back(p[2]);
        uv.push_back(kp.pt.x); uv.push_back(kp.pt.y);
        isg.push_back(frame->inv_level_sigma2s_[kp.octave]);
        slot.push_back(i);
      }
      const int n = (int)slot.size();
      if (n < 3) return 0;                                                      // (":330": pose untouched)
      outlier.assign(n, 0);
      dropin::check(ba_pose_optimization(K4, pose7, Xw.data(), uv.data(), isg.data(), n, outlier.data(), &n_inliers, nullptr), "ba_pose_optimization");
      for (int k = 0; k < n; k++) frame->is_outliers_[slot[k]] = outlier[k] != 0;       // CheckOutliers (":333")
    }
    frame->SetPose(Matrix_7_1_ToMatrix4d(pose7));                               // normalized q -> R (":336-340")
    return n_inliers;
  }

  // ---- src/CeresOptimizer.cc:49-57 (Tracking.cc:502, LoopClosing.cc:656) -------------------------------------------------
  void static GlobalBundleAdjustemnt(Map* map, int n_iterations = 200, bool* stop_flag = nullptr, const unsigned long n_loop_keyframe = 0,
                                     const bool is_robust = true) {
    std::vector<KeyFrame*> keyframes = map->GetAllKeyFrames();
    std::vector<MapPoint*> map_points = map->GetAllMapPoints();
    BundleAdjustment(keyframes, map_points, n_iterations, stop_flag, n_loop_keyframe, is_robust);
  }

  // ---- src/CeresOptimizer.cc:59-225 ---------------------------------------------------------------------------------------
  void static BundleAdjustment(const std::vector<KeyFrame*>& keyframes, const std::vector<MapPoint*>& map_points, int n_iterations = 200,
                               bool* stop_flag = nullptr, const unsigned long n_loop_keyframe = 0, const bool is_robust = true) {
    if (keyframes.empty()) return;
    unsigned long max_keyframe_id = 0;
    std::map<KeyFrame*, int> cam_of;                               // ided_keyframe_pose: non-bad keyframes
    std::vector<KeyFrame*> cams;
    std::vector<double> K4, poses7; std::vector<uint8_t> cam_fixed;
    // (cameras by keyframe id - Map::GetAllKeyFrames() hands over a std::set<KeyFrame*>'s pointer order, i.e. whatever the allocator did;
    // by id an odometry-like map gives a banded reduced system, which the library factors at the cost of the band: see LocalBundleAdjustment)
    std::vector<KeyFrame*> kf_by_id(keyframes);
    std::stable_sort(kf_by_id.begin(), kf_by_id.end(), [](const KeyFrame* a, const KeyFrame* b) { return a->id_ < b->id_; });
    for (size_t i = 0; i < kf_by_id.size(); i++) {
      KeyFrame* keyframe = kf_by_id[i];
      if (keyframe->isBad()) continue;
      if (cam_of.count(keyframe)) continue;
      double p7[7];
      Matrix4dToMatrix_7_1(keyframe->GetPose(), p7);
      cam_of[keyframe] = (int)cams.size(); cams.push_back(keyframe);
      poses7.insert(poses7.end(), p7, p7 + 7);
      const double k4[4] = {keyframe->fx_, keyframe->fy_, keyframe->cx_, keyframe->cy_};
      K4.insert(K4.end(), k4, k4 + 4);
      cam_fixed.push_back(keyframe->id_ == 0 ? 1 : 0);            // (":115-120")
      if (keyframe->id_ > max_keyframe_id) max_keyframe_id = keyframe->id_;
    }
    std::vector<int> pt_of(map_points.size(), -1);                 // -1: bad, or no edge (is_not_optimized_map_point)
    std::vector<double> pts3, obs_uv, obs_w; std::vector<int32_t> obs_cam, obs_pt; std::vector<uint8_t> obs_rob;
    for (size_t i = 0; i < map_points.size(); i++) {
      MapPoint* map_point = map_points[i];
      if (map_point->isBad()) continue;
      const Vector3d X = map_point->GetWorldPos();
      const std::map<KeyFrame*, size_t> observations = map_point->GetObservations();
      int n_edges = 0;
      const int pid = (int)(pts3.size() / 3);
      for (auto it = observations.begin(); it != observations.end(); ++it) {
        KeyFrame* keyframe = it->first;
        if (keyframe->isBad() || keyframe->id_ > max_keyframe_id) continue;
        auto c = cam_of.find(keyframe);
        if (c == cam_of.end()) continue;                           // (a keyframe outside `keyframes`: the reference would insert a zero pose here)
        n_edges++;
        const auto& kp = keyframe->undistort_keypoints_[it->second];
        obs_cam.push_back(c->second); obs_pt.push_back(pid);
        obs_uv.push_back(kp.pt.x); obs_uv.push_back(kp.pt.y);
        obs_w.push_back((double)keyframe->inv_level_sigma2s_[kp.octave]);        // sqrt_information = I * invSigma2 (F7)
        obs_rob.push_back(is_robust ? 1 : 0);
      }
      if (n_edges == 0) continue;                                  // (":170-172": RemoveParameterBlock of a never-added block; skipped)
      pt_of[i] = pid;
      pts3.push_back(X[0]); pts3.push_back(X[1]); pts3.push_back(X[2]);
    }
    ba_options o; o.max_iterations = n_iterations; o.huber_delta = std::sqrt(5.991); o.fix_points = 0;
    o.stop_flag = reinterpret_cast<const volatile uint8_t*>(stop_flag);
    dropin::check(ba_solve(K4.data(), poses7.data(), cam_fixed.data(), (int)cams.size(), pts3.data(), (int)(pts3.size() / 3), obs_cam.data(), obs_pt.data(),
                           obs_uv.data(), obs_w.data(), obs_rob.data(), (int)obs_cam.size(), &o, nullptr), "ba_solve");
    for (size_t c = 0; c < cams.size(); c++) {                     // (":194-209")
      KeyFrame* keyframe = cams[c];
      if (keyframe->isBad()) continue;
      const Matrix4d pose = Matrix_7_1_ToMatrix4d(&poses7[7 * c]);
      if (n_loop_keyframe == 0) keyframe->SetPose(pose);
      else { keyframe->global_BA_Tcw_ = pose; keyframe->n_BA_global_for_keyframe_ = n_loop_keyframe; }
    }
    for (size_t i = 0; i < map_points.size(); i++) {               // (":211-224")
      if (pt_of[i] < 0) continue;
      MapPoint* map_point = map_points[i];
      if (map_point->isBad()) continue;
      Vector3d X;
      for (int k = 0; k < 3; k++) X[k] = pts3[3 * (size_t)pt_of[i] + k];
      if (n_loop_keyframe == 0) { map_point->SetWorldPos(X); map_point->UpdateNormalAndDepth(); }
      else { map_point->global_BA_pose_ = X; map_point->n_BA_global_for_keyframe_ = n_loop_keyframe; }
    }
  }

  // ---- src/CeresOptimizer.cc:344-599 (LocalMapping.cc:89) -----------------------------------------------------------------
  void static LocalBundleAdjustment(KeyFrame* keyframe, bool* stop_flag, Map* map) {
    // local keyframes: the current one and its covisibles (":348-363")
    std::vector<KeyFrame*> local_kfs; std::map<KeyFrame*, int> cam_of;
    auto add_cam = [&](KeyFrame* kf, std::vector<KeyFrame*>& list) { if (!cam_of.count(kf)) { cam_of[kf] = -1; list.push_back(kf); } };
    add_cam(keyframe, local_kfs);
    keyframe->n_BA_local_for_keyframe_ = keyframe->id_;
    const std::vector<KeyFrame*> neighbor_keyframes = keyframe->GetVectorCovisibleKeyFrames();
    for (size_t i = 0; i < neighbor_keyframes.size(); i++) {
      KeyFrame* nb = neighbor_keyframes[i];
      nb->n_BA_local_for_keyframe_ = keyframe->id_;
      if (!nb->isBad()) add_cam(nb, local_kfs);
    }
    // local map points seen in local keyframes (":366-384"); std::map = the reference's container (and its iteration order)
    std::map<MapPoint*, int> pt_of;
    for (KeyFrame* kf : local_kfs) {
      const std::vector<MapPoint*> mps = kf->GetMapPointMatches();
      for (MapPoint* mp : mps)
        if (mp && !mp->isBad() && mp->n_BA_local_for_keyframe_ != keyframe->id_) { pt_of[mp] = -1; mp->n_BA_local_for_keyframe_ = keyframe->id_; }
    }
    // fixed keyframes: see local points, are not local (":388-406")
    std::map<KeyFrame*, int> fixed_set;
    for (auto it = pt_of.begin(); it != pt_of.end(); ++it) {
      const std::map<KeyFrame*, size_t> observations = it->first->GetObservations();
      for (auto ob = observations.begin(); ob != observations.end(); ++ob) {
        KeyFrame* kf = ob->first;
        if (kf->n_BA_local_for_keyframe_ != keyframe->id_ && kf->n_BA_fixed_for_keyframe_ != keyframe->id_) {
          kf->n_BA_fixed_for_keyframe_ = keyframe->id_;
          if (!kf->isBad()) fixed_set[kf] = -1;
        }
      }
    }
    // flatten: cameras = local (free unless id 0) then fixed; points in map order; one observation per (point, non-bad keyframe)
    std::vector<KeyFrame*> cams;
    std::vector<double> K4, poses7; std::vector<uint8_t> cam_fixed, cam_local;
    auto push_cam = [&](KeyFrame* kf, bool local) {
      double p7[7];
      Matrix4dToMatrix_7_1(kf->GetPose(), p7);
      cam_of[kf] = (int)cams.size(); cams.push_back(kf);
      poses7.insert(poses7.end(), p7, p7 + 7);
      const double k4[4] = {kf->fx_, kf->fy_, kf->cx_, kf->cy_};
      K4.insert(K4.end(), k4, k4 + 4);
      cam_local.push_back(local ? 1 : 0);
      cam_fixed.push_back((!local || kf->id_ == 0) ? 1 : 0);      // (":476-481", ":499-502")
    };
    // Camera ORDER (round 5).  The reference keeps the local keyframes in an unordered_map keyed by pointer (":348") and Ceres orders the
    // parameter blocks itself, so there is no order to reproduce; the library factors the reduced system in the order given and skips
    // the tiles outside its skyline (INTEGRATION.md "What the keyframe order means for the solver").  By keyframe id - the current
    // keyframe, which shares landmarks with every other one, is the newest and comes LAST - a window along an odometry chain is a band
    // with one dense block row; with the current keyframe first (rounds 1-4) the first block column was dense and so the whole envelope.
    // Deterministic whatever the allocator does; the results are the same to rounding.
    std::vector<KeyFrame*> by_id(local_kfs);
    std::stable_sort(by_id.begin(), by_id.end(), [](const KeyFrame* a, const KeyFrame* b) { return a->id_ < b->id_; });
    for (KeyFrame* kf : by_id) push_cam(kf, true);
    for (auto it = fixed_set.begin(); it != fixed_set.end(); ++it) push_cam(it->first, false);
    std::vector<MapPoint*> pts; std::vector<double> pts3, obs_uv; std::vector<float> obs_isg; std::vector<int32_t> obs_cam, obs_pt;
    std::vector<std::pair<KeyFrame*, MapPoint*>> obs_edge;
    for (auto it = pt_of.begin(); it != pt_of.end(); ++it) {
      MapPoint* mp = it->first;
      const Vector3d X = mp->GetWorldPos();
      it->second = (int)pts.size(); pts.push_back(mp);
      pts3.push_back(X[0]); pts3.push_back(X[1]); pts3.push_back(X[2]);
      const std::map<KeyFrame*, size_t> observations = mp->GetObservations();
      for (auto ob = observations.begin(); ob != observations.end(); ++ob) {
        KeyFrame* kf = ob->first;
        if (kf->isBad()) continue;
        auto c = cam_of.find(kf);
        if (c == cam_of.end() || c->second < 0) continue;          // neither local nor fixed (":465,:483": no residual is added)
        const auto& kp = kf->undistort_keypoints_[ob->second];
        obs_cam.push_back(c->second); obs_pt.push_back(it->second);
        obs_uv.push_back(kp.pt.x); obs_uv.push_back(kp.pt.y);
        obs_isg.push_back(kf->inv_level_sigma2s_[kp.octave]);
        obs_edge.push_back(std::make_pair(kf, mp));
      }
    }
    if (stop_flag && *stop_flag) return;                           // (":509-512")
    std::vector<uint8_t> erase(obs_cam.size() ? obs_cam.size() : 1, 0);
    int aborted = 0;
    dropin::check(ba_local_bundle_adjustment(K4.data(), poses7.data(), cam_fixed.data(), cam_local.data(), (int)cams.size(), pts3.data(), (int)pts.size(),
                                             obs_cam.data(), obs_pt.data(), obs_uv.data(), obs_isg.data(), (int)obs_cam.size(),
                                             reinterpret_cast<const volatile uint8_t*>(stop_flag), 1, erase.data(), &aborted, nullptr, nullptr),
                  "ba_local_bundle_adjustment");
    if (aborted) return;                                           // stop raised before pass 2: the reference returns without writing back
    std::unique_lock<std::mutex> lock(map->mutex_map_update_);     // (":573")
    for (size_t i = 0; i < obs_edge.size(); i++)
      if (erase[i]) { obs_edge[i].first->EraseMapPointMatch(obs_edge[i].second); obs_edge[i].second->EraseObservation(obs_edge[i].first); }
    for (KeyFrame* kf : local_kfs) kf->SetPose(Matrix_7_1_ToMatrix4d(&poses7[7 * (size_t)cam_of[kf]]));          // (":584-590"; the calls in the collection order, the poses from the cameras' places)
    for (size_t p = 0; p < pts.size(); p++) {                      // (":592-598")
      Vector3d X;
      for (int k = 0; k < 3; k++) X[k] = pts3[3 * p + k];
      pts[p]->SetWorldPos(X);
      pts[p]->UpdateNormalAndDepth();
    }
  }

  // ---- src/CeresOptimizer.cc:601-735 (LoopClosing.cc:324) ------------------------------------------------------------------
  // Sim3 = Sophus::Sim3d (or anything whose data() is its storage [qx, qy, qz, qw with |q|^2 = scale, tx, ty, tz]).
  typedef typename Types::Sim3 Sim3;
  typedef typename Types::KeyFrameAndSim3 KeyFrameAndSim3;

  int static OptimizeSim3(KeyFrame* keyframe_1, KeyFrame* keyframe_2, std::vector<MapPoint*>& matches12, Sim3& S12, const float th2, const bool bFixScale) {
    using namespace dropin;
    const double K1[4] = {keyframe_1->fx_, keyframe_1->fy_, keyframe_1->cx_, keyframe_1->cy_};      // keyframe->K_ (":607-608")
    const double K2[4] = {keyframe_2->fx_, keyframe_2->fy_, keyframe_2->cx_, keyframe_2->cy_};
    const Matrix3d R1cw = keyframe_1->GetRotation(), R2cw = keyframe_2->GetRotation();
    const P3 t1cw = p3(keyframe_1->GetTranslation()), t2cw = p3(keyframe_2->GetTranslation());
    const int N = (int)matches12.size();
    const std::vector<MapPoint*> map_points_1 = keyframe_1->GetMapPointMatches();
    std::vector<double> P3D2c, obs1, P3D1c, obs2; std::vector<float> w1, w2;
    for (int i = 0; i < N; i++) {                                      // (":633-692")
      if (!matches12[i]) continue;
      MapPoint* map_point_1 = map_points_1[i];
      MapPoint* map_point_2 = matches12[i];
      const int i2 = map_point_2->GetIndexInKeyFrame(keyframe_2);
      if (!map_point_1 || !map_point_2) continue;
      if (map_point_1->isBad() || map_point_2->isBad() || i2 < 0) continue;
      const auto& keypoint_1 = keyframe_1->undistort_keypoints_[i];
      const auto& keypoint_2 = keyframe_2->undistort_keypoints_[i2];
      const P3 c2 = add(rot(R2cw, p3(map_point_2->GetWorldPos())), t2cw);
      const P3 c1 = add(rot(R1cw, p3(map_point_1->GetWorldPos())), t1cw);
      P3D2c.push_back(c2.x); P3D2c.push_back(c2.y); P3D2c.push_back(c2.z); obs1.push_back(keypoint_1.pt.x); obs1.push_back(keypoint_1.pt.y);
      w1.push_back(keyframe_1->inv_level_sigma2s_[keypoint_1.octave]);
      P3D1c.push_back(c1.x); P3D1c.push_back(c1.y); P3D1c.push_back(c1.z); obs2.push_back(keypoint_2.pt.x); obs2.push_back(keypoint_2.pt.y);
      w2.push_back(keyframe_2->inv_level_sigma2s_[keypoint_2.octave]);
    }
    int n_inliers = 0;
    double s12[7];
    for (int k = 0; k < 7; k++) s12[k] = S12.data()[k];
    const double dummy[3] = {0, 0, 0}; const float fdummy[1] = {0};
    const int n = (int)w1.size();
    check(ba_optimize_sim3(K1, K2, s12, n ? P3D2c.data() : dummy, n ? obs1.data() : dummy, n ? w1.data() : fdummy, n ? P3D1c.data() : dummy, n ? obs2.data() : dummy,
                           n ? w2.data() : fdummy, n, (double)th2, bFixScale ? 1 : 0, nullptr, &n_inliers, nullptr), "ba_optimize_sim3");
    for (int k = 0; k < 7; k++) S12.data()[k] = s12[k];                // S12 = Sim3d::exp(sim12) (":696")
    return n_inliers;                                                  // 0 when fewer than 10 (":731")
  }

  // ---- src/CeresOptimizer.cc:737-957 (LoopClosing.cc:573) -----------------------------------------------------------------
  // The reference indexes its parameter blocks by keyframe id in arrays of max id + 1; here the non-bad keyframes of the map
  // are numbered densely in map order.  An edge to a keyframe without a block (bad, or not in the map: the reference would
  // read an uninitialised 7-vector there) is not added, and bad keyframes are not written back.
  void static OptimizeEssentialGraph(Map* map, KeyFrame* loop_keyframe, KeyFrame* current_keyframe, const KeyFrameAndSim3& keyframes_non_corrected_sim3,
                                     const KeyFrameAndSim3& keyframes_corrected_sim3, const std::map<KeyFrame*, std::set<KeyFrame*> >& loop_connections,
                                     const bool& is_fixed_scale) {
    (void)is_fixed_scale;                                              // (never read by the reference either)
    const int min_weight = 100;
    const std::vector<KeyFrame*> all_keyframes = map->GetAllKeyFrames();
    const std::vector<MapPoint*> all_map_points = map->GetAllMapPoints();
    std::unordered_map<KeyFrame*, int> vtx;
    std::vector<KeyFrame*> kfs;
    std::vector<double> lie; std::vector<uint8_t> fixed;
    for (size_t i = 0; i < all_keyframes.size(); i++) {                // (":769-793")
      KeyFrame* keyframe = all_keyframes[i];
      if (keyframe->isBad() || vtx.count(keyframe)) continue;
      double S[7], x[7];
      auto it = keyframes_corrected_sim3.find(keyframe);
      if (it != keyframes_corrected_sim3.end()) { for (int k = 0; k < 7; k++) S[k] = it->second.data()[k]; }
      else se3_as_sim3(keyframe->GetPose(), S);                        // Sim3d(RxSO3d(1.0, Rcw), tcw)
      dropin::check(ba_sim3_log(S, x), "ba_sim3_log");
      vtx[keyframe] = (int)kfs.size(); kfs.push_back(keyframe);
      lie.insert(lie.end(), x, x + 7);
      fixed.push_back(keyframe == loop_keyframe ? 1 : 0);
    }
    const int n_kf = (int)kfs.size();
    if (n_kf == 0) return;
    const std::vector<double> lie_orig = lie;
    std::vector<int32_t> edge_j, edge_i; std::vector<double> edge_S;
    auto exp_of = [&](int v, double* S) { dropin::check(ba_sim3_exp(&lie_orig[7 * (size_t)v], S), "ba_sim3_exp"); };
    auto add_edge = [&](int vj, int vi, const double* Sjw, const double* Swi) {
      double Sji[7];
      dropin::check(ba_sim3_mul(Sjw, Swi, Sji), "ba_sim3_mul");
      edge_j.push_back(vj); edge_i.push_back(vi); edge_S.insert(edge_S.end(), Sji, Sji + 7);
    };
    // the pose a keyframe enters "normal" edges with: its non-corrected Sim3 if it has one, else exp of its block (":826-833", ":842-847")
    auto world_pose = [&](KeyFrame* kf, int v, double* S) {
      auto it = keyframes_non_corrected_sim3.find(kf);
      if (it != keyframes_non_corrected_sim3.end()) { for (int k = 0; k < 7; k++) S[k] = it->second.data()[k]; }
      else exp_of(v, S);
    };
    std::set<std::pair<unsigned long, unsigned long> > inserted_edges;
    for (auto it = loop_connections.begin(); it != loop_connections.end(); ++it) {       // (":797-821")
      KeyFrame* keyframe = it->first;
      auto vi = vtx.find(keyframe);
      if (vi == vtx.end()) continue;
      const unsigned long id_i = keyframe->id_;
      double Siw[7], Swi[7];
      exp_of(vi->second, Siw);
      dropin::check(ba_sim3_inverse(Siw, Swi), "ba_sim3_inverse");
      for (auto jt = it->second.begin(); jt != it->second.end(); ++jt) {
        const unsigned long id_j = (*jt)->id_;
        if ((id_i != current_keyframe->id_ || id_j != loop_keyframe->id_) && keyframe->GetWeight(*jt) < min_weight) continue;
        auto vj = vtx.find(*jt);
        if (vj == vtx.end()) continue;
        double Sjw[7];
        exp_of(vj->second, Sjw);
        add_edge(vj->second, vi->second, Sjw, Swi);
        inserted_edges.insert(std::make_pair(std::min(id_i, id_j), std::max(id_i, id_j)));
      }
    }
    for (size_t i = 0; i < all_keyframes.size(); i++) {                // (":824-905")
      KeyFrame* keyframe = all_keyframes[i];
      auto vi = vtx.find(keyframe);
      if (vi == vtx.end() || kfs[vi->second] != keyframe) continue;
      double Siw[7], Swi[7];
      world_pose(keyframe, vi->second, Siw);
      dropin::check(ba_sim3_inverse(Siw, Swi), "ba_sim3_inverse");
      KeyFrame* parent_keyframe = keyframe->GetParent();
      if (parent_keyframe) {
        auto vj = vtx.find(parent_keyframe);
        if (vj != vtx.end()) { double Sjw[7]; world_pose(parent_keyframe, vj->second, Sjw); add_edge(vj->second, vi->second, Sjw, Swi); }
      }
      const std::set<KeyFrame*> loop_edges = keyframe->GetLoopEdges();
      for (auto lt = loop_edges.begin(); lt != loop_edges.end(); ++lt) {
        KeyFrame* local_loop_keyframe = *lt;
        if (local_loop_keyframe->id_ < keyframe->id_) {
          auto vl = vtx.find(local_loop_keyframe);
          if (vl == vtx.end()) continue;
          double Slw[7]; world_pose(local_loop_keyframe, vl->second, Slw); add_edge(vl->second, vi->second, Slw, Swi);
        }
      }
      const std::vector<KeyFrame*> connected_keyframes = keyframe->GetCovisiblesByWeight(min_weight);
      for (auto ct = connected_keyframes.begin(); ct != connected_keyframes.end(); ++ct) {
        KeyFrame* keyframe_n = *ct;
        if (keyframe_n && keyframe_n != parent_keyframe && !keyframe->hasChild(keyframe_n) && !loop_edges.count(keyframe_n)) {
          if (!keyframe_n->isBad() && keyframe_n->id_ < keyframe->id_) {
            if (inserted_edges.count(std::make_pair(std::min<unsigned long>(keyframe->id_, keyframe_n->id_), std::max<unsigned long>(keyframe->id_, keyframe_n->id_)))) continue;
            auto vn = vtx.find(keyframe_n);
            if (vn == vtx.end()) continue;
            double Snw[7]; world_pose(keyframe_n, vn->second, Snw); add_edge(vn->second, vi->second, Snw, Swi);
          }
        }
      }
    }
    const int32_t idummy[1] = {0}; const double ddummy[7] = {0, 0, 0, 1, 0, 0, 0};
    const int n_edges = (int)edge_j.size();
    dropin::check(ba_optimize_essential_graph(lie.data(), fixed.data(), n_kf, n_edges ? edge_j.data() : idummy, n_edges ? edge_i.data() : idummy,
                                              n_edges ? edge_S.data() : ddummy, n_edges, 100, nullptr, nullptr), "ba_optimize_essential_graph");
    // write-back (":908-956"): SE(3) recovery per keyframe, map points through their reference keyframe
    std::vector<MapPoint*> pts; std::vector<int32_t> pt_ref; std::vector<double> pts3;
    for (size_t i = 0; i < all_map_points.size(); i++) {
      MapPoint* map_point = all_map_points[i];
      if (map_point->isBad()) continue;
      KeyFrame* ref = nullptr;
      if (map_point->corrected_by_keyframe_ == current_keyframe->id_) {
        for (KeyFrame* k : kfs) if (k->id_ == (unsigned long)map_point->corrected_reference_) { ref = k; break; }
      } else ref = map_point->GetReferenceKeyFrame();
      auto vr = ref ? vtx.find(ref) : vtx.end();
      if (vr == vtx.end()) continue;                                   // (no block for the reference keyframe: left as it is)
      const Vector3d X = map_point->GetWorldPos();
      pts.push_back(map_point); pt_ref.push_back(vr->second); pts3.push_back(X[0]); pts3.push_back(X[1]); pts3.push_back(X[2]);
    }
    std::vector<double> Tiw(12 * (size_t)n_kf);
    dropin::check(ba_essential_graph_correct(lie_orig.data(), lie.data(), n_kf, Tiw.data(), pts.empty() ? idummy : pt_ref.data(), pts.empty() ? nullptr : pts3.data(), (int)pts.size()),
                  "ba_essential_graph_correct");
    std::unique_lock<std::mutex> lock(map->mutex_map_update_);         // (":911")
    for (int v = 0; v < n_kf; v++) {
      Matrix4d T;
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) T(r, c) = Tiw[12 * (size_t)v + 4 * r + c];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      kfs[v]->SetPose(T);
    }
    for (size_t p = 0; p < pts.size(); p++) {
      Vector3d X;
      for (int k = 0; k < 3; k++) X[k] = pts3[3 * p + k];
      pts[p]->SetWorldPos(X);
      pts[p]->UpdateNormalAndDepth();
    }
  }

  // Sophus::Sim3d(Sophus::RxSO3d(1.0, R), t) of a rigid pose, as 7 doubles (Eigen's matrix -> quaternion branches through the pose codec)
  static void se3_as_sim3(const Matrix4d& T, double S[7]) {
    double p7[7];
    Matrix4dToMatrix_7_1(T, p7);
    S[0] = p7[3]; S[1] = p7[4]; S[2] = p7[5]; S[3] = p7[6]; S[4] = p7[0]; S[5] = p7[1]; S[6] = p7[2];
  }
};

// ============================================================================================== Frame-side steps
// The bodies of the reference's member functions on either side of the matcher, over the same Types bundle: a maintainer
// replaces the body of Frame::ComputeBoW / KeyFrame::ComputeBoW / Frame::isInFrustum / Frame::GetFeaturesInArea /
// KeyFrame::GetFeaturesInArea by ONE call, and the per-match body of LocalMapping::CreateNewMapPoints by TriangulateMatches.
template <class Types>
struct FrameOpsT {
  typedef typename Types::Frame Frame;
  typedef typename Types::KeyFrame KeyFrame;
  typedef typename Types::MapPoint MapPoint;
  typedef typename Types::Matrix3d Matrix3d;
  typedef typename Types::Vector3d Vector3d;

  // Frame::ComputeBoW (src/Frame.cc:322-327: only when bow_vector_ is empty) and KeyFrame::ComputeBoW (src/KeyFrame.cc:107-117:
  // when either container is empty): orb_vocabulary_->transform(descriptors, bow_vector_, feature_vector_, 4)
  template <class F> static void ComputeBoW(F& f, orbv_ctx* orb_vocabulary, bool also_when_feature_vector_empty = false) {
    if (!(f.bow_vector_.empty() || (also_when_feature_vector_empty && f.feature_vector_.empty()))) return;
    const int n = (int)f.undistort_keypoints_.size();
    std::vector<uint8_t> desc(32 * (size_t)std::max(n, 1));
    for (int i = 0; i < n; i++) std::memcpy(&desc[32 * (size_t)i], f.descriptors_.ptr(i), 32);
    std::vector<uint32_t> bw(std::max(n, 1)), fn(std::max(n, 1)), fo(n + 2), fi(std::max(n, 1));
    std::vector<double> bv(std::max(n, 1));
    int nw = 0, nf = 0;
    dropin::check(orbv_transform(orb_vocabulary, desc.data(), n, 4, bw.data(), bv.data(), &nw, fn.data(), fo.data(), fi.data(), &nf), "orbv_transform");
    f.bow_vector_.clear(); f.feature_vector_.clear();
    for (int k = 0; k < nw; k++) f.bow_vector_.insert(f.bow_vector_.end(), std::make_pair(bw[k], bv[k]));
    for (int m = 0; m < nf; m++) {
      auto it = f.feature_vector_.insert(f.feature_vector_.end(), std::make_pair(fn[m], std::vector<unsigned int>()));
      it->second.assign(fi.begin() + fo[m], fi.begin() + fo[m + 1]);
    }
  }

  // Frame::isInFrustum (src/Frame.cc:191-241) for a LIST of map points - the loop of Tracking::SearchLocalPoints
  // (src/Tracking.cc:810-826) in one call: sets is_track_in_view_, track_proj_x_, track_proj_y_, track_scale_level_,
  // track_view_cos_ of every point exactly as the member function does and returns the per-point results.
  static std::vector<bool> isInFrustum(Frame& F, const std::vector<MapPoint*>& points, float viewingCosLimit) {
    using namespace dropin;
    const size_t n = points.size();
    std::vector<bool> res(n, false);
    if (!n) return res;
    double R[9], t[3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[3 * r + c] = F.Tcw_(r, c); t[r] = F.Tcw_(r, 3); }
    const float K4[4] = {F.fx_, F.fy_, F.cx_, F.cy_}, bounds[4] = {(float)F.min_x_, (float)F.max_x_, (float)F.min_y_, (float)F.max_y_};
    std::vector<double> P(3 * n), Pn(3 * n); std::vector<float> mn(n), mx(n);
    for (size_t i = 0; i < n; i++) {
      const Vector3d p = points[i]->GetWorldPos(), nn = points[i]->GetNormal();
      for (int k = 0; k < 3; k++) { P[3 * i + k] = p[k]; Pn[3 * i + k] = nn[k]; }
      mn[i] = points[i]->GetMinDistanceInvariance(); mx[i] = points[i]->GetMaxDistanceInvariance();
    }
    std::vector<uint8_t> in_view(n); std::vector<float> uv(2 * n), vc(n), dist(n);
    check(orbm_is_in_frustum_gates(R, t, K4, bounds, P.data(), Pn.data(), mn.data(), mx.data(), (int)n, viewingCosLimit, in_view.data(), uv.data(), vc.data(), dist.data()),
          "orbm_is_in_frustum_gates");
    for (size_t i = 0; i < n; i++) {
      MapPoint* mp = points[i];
      mp->is_track_in_view_ = false;                                   // (":192")
      if (!in_view[i]) continue;
      const int nPredictedLevel = mp->PredictScale(dist[i], &F);      // (":231")
      mp->is_track_in_view_ = true; mp->track_proj_x_ = uv[2 * i]; mp->track_proj_y_ = uv[2 * i + 1];
      mp->track_scale_level_ = nPredictedLevel; mp->track_view_cos_ = vc[i];
      res[i] = true;
    }
    return res;
  }
  static bool isInFrustum(Frame& F, MapPoint* map_point, float viewingCosLimit) { return isInFrustum(F, std::vector<MapPoint*>(1, map_point), viewingCosLimit)[0]; }

  // Frame::GetFeaturesInArea (src/Frame.cc:243-307) and KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:575-622, levels -1 / -1)
  template <class F> static std::vector<size_t> GetFeaturesInArea(const F& f, const float& x, const float& y, const float& r, const int minLevel = -1, const int maxLevel = -1) {
    dropin::Flat T; dropin::flatten(f, &T);
    const float q[2] = {x, y};
    const int32_t lo = minLevel, hi = maxLevel;
    std::vector<uint32_t> off(2, 0), idx((size_t)std::max(T.n, 1));
    int total = 0;
    dropin::check(orbm_features_in_area(T.kps4.data(), T.n, T.bounds, q, &r, &lo, &hi, 1, off.data(), idx.data(), (int)idx.size(), &total), "orbm_features_in_area");
    return std::vector<size_t>(idx.begin(), idx.begin() + total);
  }

  // Tracking::Relocalization, everything behind `Tcw = pSolver->iterate(...)` (src/Tracking.cc:1056-1126) for ALL candidates of one pass of
  // the `while` loop in ONE call (orbt_relocalization_refine) on the frame `extractor` left on the device for this thread
  // (orbt_relocalization_search_by_bow at the top of Relocalization): per candidate i that has a pose - poses[i] is not the identity,
  // :1059 - matches[i] = map_point_matches_vector[i] and inliers[i] = is_inliers of its PnP solver.  Returns the index of the first
  // candidate with nGood >= 50, where the reference breaks out (:1122-1125), and leaves Tcw_, map_points_ and is_outliers_ of
  // current_frame as that candidate's refinement leaves them; -1: no candidate matched, and the frame is left as the LAST refined
  // candidate leaves it (the reference went through all of them).  is_outliers_ is written for every feature (the reference keeps flags of
  // earlier candidates on slots that are empty now; nothing reads a flag of an empty slot).  The map points' min_distance_ /
  // max_distance_ are read directly: MapPoint.h declares `template <class> friend struct FrameOpsT;`.
  // (Matrix4d is a template parameter: a Types bundle without Tracking's matrix type can still instantiate the rest of FrameOpsT.)
  template <class Matrix4d>
  static int RelocalizationRefine(orbx_ctx* extractor, Frame& current_frame, const std::vector<KeyFrame*>& candidate_keyframes,
                                  const std::vector<std::vector<MapPoint*> >& matches, const std::vector<Matrix4d>& poses,
                                  const std::vector<std::vector<bool> >& inliers, bool check_orientation = true, bool narrow_in_loop = true) {
    using namespace dropin;
    const size_t nc = candidate_keyframes.size();
    if (matches.size() != nc || poses.size() != nc || inliers.size() != nc) throw std::runtime_error("FrameOpsT::RelocalizationRefine: one entry per candidate keyframe is needed");
    if (!nc) return -1;
    const int n_kp = current_frame.N_;
    struct Cand { std::vector<int32_t> pt, slot; std::vector<double> X; std::vector<uint8_t> desc; std::vector<float> mn, mx, ang; std::vector<MapPoint*> row; double T[12]; bool has_pose; };
    std::vector<Cand> C(nc);
    std::vector<orbt_reloc_refine_candidate> flat(nc);
    std::unordered_map<MapPoint*, int32_t> id_of;
    auto is_identity = [](const Matrix4d& T) { for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) if (T(r, c) != (r == c ? 1.0 : 0.0)) return false; return true; };
    for (size_t c = 0; c < nc; c++) {
      Cand& Q = C[c];
      KeyFrame* kf = candidate_keyframes[c];
      Q.has_pose = kf && !is_identity(poses[c]);
      if (kf) Q.row = kf->GetMapPointMatches();
      auto push = [&](MapPoint* mp, bool searchable, float angle) {      // one row of the keyframe side
        const bool usable = mp && !mp->isBad();
        int32_t id = -1;
        if (usable || (mp && !searchable)) { auto it = id_of.find(mp); id = it == id_of.end() ? (id_of[mp] = (int32_t)id_of.size()) : it->second; }
        Q.pt.push_back(id);
        const Vector3d p = mp ? mp->GetWorldPos() : Vector3d();
        for (int k = 0; k < 3; k++) Q.X.push_back(mp ? p[k] : 0.0);
        Q.desc.resize(Q.desc.size() + 32, 0);
        if (mp) { const auto d = mp->GetDescriptor(); std::memcpy(&Q.desc[Q.desc.size() - 32], d.ptr(0), 32); }
        // (a row that must not be searched - below - has an empty distance range: every distance is outside it)
        Q.mn.push_back(mp && searchable ? mp->min_distance_ : 0.f); Q.mx.push_back(mp && searchable ? mp->max_distance_ : 0.f);
        Q.ang.push_back(angle);
      };
      for (size_t i = 0; i < Q.row.size(); i++) push(Q.row[i], true, kf->undistort_keypoints_[i].angle);
      Q.slot.assign((size_t)std::max(n_kp, 1), -1);
      if (Q.has_pose) {
        std::unordered_map<MapPoint*, int32_t> at;                      // the first feature of the keyframe that holds the point
        for (size_t i = 0; i < Q.row.size(); i++) if (Q.row[i] && !Q.row[i]->isBad()) at.insert(std::make_pair(Q.row[i], (int32_t)i));
        for (int f = 0; f < n_kp && f < (int)matches[c].size() && f < (int)inliers[c].size(); f++) {
          MapPoint* mp = inliers[c][f] ? matches[c][f] : static_cast<MapPoint*>(nullptr);
          if (!mp) continue;
          auto it = at.find(mp);
          if (it == at.end()) {
            // an inlier point the keyframe does not hold (any more), or a bad one: it still is an observation of PoseOptimization and an
            // element of `found`, but SearchByProjection never walks it - a row of its own behind the keyframe's, closed to the search
            it = at.insert(std::make_pair(mp, (int32_t)Q.row.size())).first;
            Q.row.push_back(mp); push(mp, false, 0.f);
          }
          Q.slot[f] = it->second;
        }
        for (int r = 0; r < 3; r++) for (int k = 0; k < 4; k++) Q.T[4 * r + k] = poses[c](r, k);
      }
      orbt_reloc_refine_candidate& q = flat[c];
      q.pt = Q.pt.data(); q.Xw = Q.X.data(); q.desc = Q.desc.data(); q.min_dist = Q.mn.data(); q.max_dist = Q.mx.data(); q.angle = Q.ang.data();
      q.n = (int32_t)Q.pt.size(); q.reserved = 0; q.Tcw = Q.has_pose ? Q.T : nullptr; q.slot_kf = Q.has_pose ? Q.slot.data() : nullptr;
    }
    const float K4[4] = {current_frame.fx_, current_frame.fy_, current_frame.cx_, current_frame.cy_};
    const float bounds[4] = {(float)current_frame.min_x_, (float)current_frame.max_x_, (float)current_frame.min_y_, (float)current_frame.max_y_};
    std::vector<orbt_reloc_refine_result> res(nc);
    std::vector<int32_t> slot_out(nc * (size_t)std::max(n_kp, 1), -1); std::vector<uint8_t> outl(nc * (size_t)std::max(n_kp, 1), 0);
    int32_t first = -1;
    check(orbt_relocalization_refine(extractor, K4, bounds, current_frame.log_scale_factor_, flat.data(), (int)nc, n_kp, check_orientation ? 1 : 0, narrow_in_loop ? 1 : 0,
                                     res.data(), slot_out.data(), outl.data(), &first), "orbt_relocalization_refine");
    int take = first;
    if (take < 0) for (size_t c = 0; c < nc; c++) if (C[c].has_pose) take = (int)c;
    if (take < 0) return -1;                                              // nobody had a pose: the frame was not touched
    Matrix4d T;
    {
      double M[16];
      check(ba_pose7_to_matrix4d(res[take].pose7, M), "ba_pose7_to_matrix4d");
      for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) T(r, k) = M[4 * r + k];
    }
    // (a candidate whose first PoseOptimization had fewer than 3 correspondences leaves the PnP pose as it was: current_frame_.Tcw_ = Tcw, :1060)
    if (res[take].n_correspondences[0] < 3) current_frame.Tcw_ = poses[take]; else current_frame.SetPose(T);
    for (int f = 0; f < n_kp; f++) {
      const int32_t s = slot_out[(size_t)take * n_kp + f];
      current_frame.map_points_[f] = s >= 0 ? C[take].row[s] : static_cast<MapPoint*>(nullptr);
      current_frame.is_outliers_[f] = outl[(size_t)take * n_kp + f] != 0;
    }
    return first;
  }

  // LocalMapping::CreateNewMapPoints, the body of "Triangulate each match" (src/LocalMapping.cc:267-378) for all matches of one
  // neighbour keyframe: x3D[k] / ok[k] for matched_indices[k]; the caller keeps the MapPoint construction (":380-395").
  static void TriangulateMatches(KeyFrame* current_keyframe, KeyFrame* neighbor_keyframe, const std::vector<std::pair<size_t, size_t> >& matched_indices,
                                 const float ratioFactor, std::vector<Vector3d>* x3D, std::vector<bool>* ok) {
    const size_t n = matched_indices.size();
    x3D->assign(n, Vector3d()); ok->assign(n, false);
    if (!n) return;
    double T1[12], T2[12];
    const Matrix3d R1 = current_keyframe->GetRotation(), R2 = neighbor_keyframe->GetRotation();
    const Vector3d t1 = current_keyframe->GetTranslation(), t2 = neighbor_keyframe->GetTranslation();
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { T1[4 * r + c] = R1(r, c); T2[4 * r + c] = R2(r, c); } T1[4 * r + 3] = t1[r]; T2[4 * r + 3] = t2[r]; }
    const float K1[4] = {current_keyframe->fx_, current_keyframe->fy_, current_keyframe->cx_, current_keyframe->cy_};
    const float K2[4] = {neighbor_keyframe->fx_, neighbor_keyframe->fy_, neighbor_keyframe->cx_, neighbor_keyframe->cy_};
    std::vector<float> kp1(3 * n), kp2(3 * n);
    for (size_t k = 0; k < n; k++) {
      const auto& a = current_keyframe->undistort_keypoints_[matched_indices[k].first];
      const auto& b = neighbor_keyframe->undistort_keypoints_[matched_indices[k].second];
      kp1[3 * k] = a.pt.x; kp1[3 * k + 1] = a.pt.y; kp1[3 * k + 2] = (float)a.octave;
      kp2[3 * k] = b.pt.x; kp2[3 * k + 1] = b.pt.y; kp2[3 * k + 2] = (float)b.octave;
    }
    std::vector<double> X(3 * n); std::vector<uint8_t> good(n);
    dropin::check(orbm_triangulate_matches(T1, T2, K1, K2, kp1.data(), kp2.data(), (int)n, current_keyframe->level_sigma2s_.data(), current_keyframe->scale_factors_.data(),
                                           (int)current_keyframe->scale_factors_.size(), ratioFactor, X.data(), good.data()), "orbm_triangulate_matches");
    for (size_t k = 0; k < n; k++) { (*ok)[k] = good[k] != 0; for (int c = 0; c < 3; c++) (*x3D)[k][c] = X[3 * k + c]; }
  }

  // LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:196-396), everything between the baseline test and the MapPoint construction
  // for ALL neighbours in ONE call (orbl_create_new_map_points): per neighbour k the accepted triangulations {idx1, idx2, x3D} in
  // idx1 order - SearchForTriangulation with ORBmatcher(0.6, false) (:203, :250), the per-match body (:267-378), and the hand-over
  // between neighbours (a keypoint of the current keyframe that got a point is not searched again: AddMapPoint :383 /
  // src/ORBmatcher.cc:621-623).  `neighbours` = the keyframes that passed the baseline test (:231-244), F12s[k] =
  // ComputeF12(current_keyframe_, neighbours[k]) (:247); abort (nullable) = the flag CheckNewKeyFrames() reads (:227): looked at
  // before every neighbour after the first; *n_processed neighbours are complete.  The caller's loop over the result keeps the
  // reference's lines :380-393 (new MapPoint, AddObservation x 2, AddMapPoint x 2, ComputeDistinctiveDescriptors, UpdateNormalAndDepth).
  struct NewPoint { int idx1, idx2; Vector3d x3D; };
  static std::vector<std::vector<NewPoint> > CreateNewMapPoints(KeyFrame* current_keyframe, const std::vector<KeyFrame*>& neighbours, const std::vector<Matrix3d>& F12s,
                                                                const float ratioFactor, const volatile bool* abort = nullptr, int* n_processed = nullptr) {
    using namespace dropin;
    const size_t nn = neighbours.size();
    std::vector<std::vector<NewPoint> > out(nn);
    if (n_processed) *n_processed = 0;
    if (!nn) return out;
    Flat A; flatten(*current_keyframe, &A);
    FlatFV f1; flatten_fv(current_keyframe->feature_vector_, &f1);
    std::vector<uint8_t> um1((size_t)std::max(A.n, 1));
    for (int i = 0; i < A.n; i++) um1[i] = current_keyframe->GetMapPoint(i) ? 0 : 1;
    double T1[12];
    const Matrix3d R1 = current_keyframe->GetRotation(); const Vector3d t1 = current_keyframe->GetTranslation();
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T1[4 * r + c] = R1(r, c); T1[4 * r + 3] = t1[r]; }
    const float K1[4] = {current_keyframe->fx_, current_keyframe->fy_, current_keyframe->cx_, current_keyframe->cy_};
    const P3 Cw = p3(current_keyframe->GetCameraCenter());
    std::vector<Flat> B(nn); std::vector<FlatFV> f2(nn); std::vector<std::vector<uint8_t> > um2(nn);
    std::vector<orbl_keyframe> nb(nn);
    for (size_t k = 0; k < nn; k++) {
      KeyFrame* o = neighbours[k];
      flatten(*o, &B[k]); flatten_fv(o->feature_vector_, &f2[k]);
      um2[k].resize((size_t)std::max(B[k].n, 1));
      for (int i = 0; i < B[k].n; i++) um2[k][i] = o->GetMapPoint(i) ? 0 : 1;
      orbl_keyframe& q = nb[k];
      q.kps = B[k].kps4.data(); q.desc = B[k].desc; q.unmapped = um2[k].data(); q.n = B[k].n;
      q.fv_node = f2[k].node.data(); q.fv_off = f2[k].off.data(); q.fv_idx = f2[k].idx.data(); q.fv_n = (int)f2[k].node.size();
      const Matrix3d R2 = o->GetRotation(); const Vector3d t2 = o->GetTranslation();
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { q.Tcw[4 * r + c] = R2(r, c); q.F12[3 * r + c] = F12s[k](r, c); } q.Tcw[4 * r + 3] = t2[r]; }
      q.K4[0] = o->fx_; q.K4[1] = o->fy_; q.K4[2] = o->cx_; q.K4[3] = o->cy_;
      // epipole in the neighbour's image (src/ORBmatcher.cc:589-596)
      const P3 C2 = add(rot(R2, Cw), p3(t2));
      const float invz = 1.0f / C2.z;
      q.ex = o->fx_ * C2.x * invz + o->cx_; q.ey = o->fy_ * C2.y * invz + o->cy_;
    }
    std::vector<int32_t> m12(nn * (size_t)std::max(A.n, 1)); std::vector<uint8_t> ok(nn * (size_t)std::max(A.n, 1)); std::vector<double> X(3 * nn * (size_t)std::max(A.n, 1));
    // (a bool the reference's thread sets is read as a byte: sizeof(bool) == 1 on every ABI this builds for)
    static_assert(sizeof(bool) == 1, "the abort flag is read as one byte");
    int npr = 0;
    check(orbl_create_new_map_points(A.kps4.data(), A.desc, um1.data(), A.n, f1.node.data(), f1.off.data(), f1.idx.data(), (int)f1.node.size(), T1, K1, nb.data(), (int)nn,
                                     current_keyframe->scale_factors_.data(), current_keyframe->level_sigma2s_.data(), (int)current_keyframe->scale_factors_.size(), ratioFactor,
                                     (const volatile uint8_t*)abort, m12.data(), ok.data(), X.data(), &npr), "orbl_create_new_map_points");
    if (n_processed) *n_processed = npr;
    for (size_t k = 0; k < (size_t)npr; k++)
      for (int i = 0; i < A.n; i++) {
        const size_t e = k * (size_t)A.n + i;
        if (!ok[e]) continue;
        NewPoint np; np.idx1 = i; np.idx2 = m12[e];
        for (int c = 0; c < 3; c++) np.x3D[c] = X[3 * e + c];
        out[k].push_back(np);
      }
    return out;
  }

  // MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:256-315, what & ORBL_MP_DESC) and MapPoint::UpdateNormalAndDepth
  // (:335-378, what & ORBL_MP_NORMAL_DEPTH) for a LIST of points in ONE library call (orbl_update_map_points): the loops of
  // LocalMapping.cc:141-152, :386-388 (after the loop over the new points), :476-485 and the LocalBA write-back
  // (src/CeresOptimizer.cc:590-598).  Per point the snapshot of the reference's methods - is_bad_, observations_ (std::map order),
  // reference_keyframe_, world_pose_ under mutex_features_ (+ mutex_pose_ for the normal) - then keyframe->isBad() for the
  // descriptor part only, GetCameraCenter(), and the octave of undistort_keypoints_[observations[reference_keyframe]] (operator[]
  // on the local copy: index 0 when the reference keyframe is not in the list).  The results are written back under the
  // reference's lock scopes: descriptor_ under mutex_features_ (:311-314), max / min_distance_ and normal_vector_ under mutex_pose_
  // (:373-377).  Inside the reference tree these members are protected: MapPoint.h declares `template <class> friend struct
  // FrameOpsT;`; the mutexes are taken when the type has them.  One call per distinct scale-factor table
  // of the reference keyframes (every keyframe copies the one extractor's: one call).  NULL entries are skipped.
  static void UpdateMapPoints(const std::vector<MapPoint*>& points, int what) {
    const bool desc = (what & ORBL_MP_DESC) != 0, nd = (what & ORBL_MP_NORMAL_DEPTH) != 0;
    if (points.empty() || !(desc || nd)) return;
    struct Snap { bool bad = true; std::vector<std::pair<KeyFrame*, size_t> > obs; KeyFrame* ref = nullptr; double X[3] = {0, 0, 0}; int level = 0; };
    std::vector<Snap> S(points.size());
    std::vector<std::vector<float> > tables;                   // distinct scale-factor tables, and the points of each
    std::vector<std::vector<size_t> > members(1);
    for (size_t i = 0; i < points.size(); i++) {
      MapPoint* mp = points[i];
      Snap& s = S[i];
      if (!mp) { members[0].push_back(i); continue; }           // (NULL entries of GetMapPointMatches(): skipped, as :479)
      {
        std::unique_lock<std::mutex> lock1 = lock_features(mp, 0);
        std::unique_lock<std::mutex> lock2 = nd ? lock_pose(mp, 0) : std::unique_lock<std::mutex>();
        s.bad = mp->is_bad_;
        if (!s.bad) {
          s.obs.assign(mp->observations_.begin(), mp->observations_.end());
          if (nd) { s.ref = mp->reference_keyframe_; for (int k = 0; k < 3; k++) s.X[k] = mp->world_pose_[k]; }
        }
      }
      if (!nd || s.bad || s.obs.empty()) { members[0].push_back(i); continue; }
      if (!s.ref) throw std::runtime_error("UpdateMapPoints: a map point with observations has no reference keyframe");
      size_t kp = 0;                                           // observations[reference_keyframe] (:369-371)
      for (const auto& o : s.obs) if (o.first == s.ref) { kp = o.second; break; }
      s.level = s.ref->undistort_keypoints_[kp].octave;
      const std::vector<float> t(s.ref->scale_factors_.begin(), s.ref->scale_factors_.begin() + s.ref->n_scale_levels_);
      size_t g = 0;
      while (g < tables.size() && tables[g] != t) g++;
      if (g == tables.size()) { tables.push_back(t); if (g > 0) members.push_back(std::vector<size_t>()); }
      members[g].push_back(i);
    }
    if (tables.empty()) tables.push_back(std::vector<float>(1, 1.0f));
    for (size_t g = 0; g < members.size(); g++) {
      const std::vector<size_t>& idx = members[g];
      if (idx.empty()) continue;
      const int n = (int)idx.size();
      std::vector<int32_t> off(n + 1, 0), obs_kf, ref_kf(n, -1), ref_level(n, 0);
      std::vector<uint8_t> pt_good(n, 0), obs_desc, kf_good;
      std::vector<double> X(3 * (size_t)n, 0.0), centers;
      std::unordered_map<KeyFrame*, int> kf_at;
      auto kf_index = [&](KeyFrame* kf) {
        auto it = kf_at.find(kf);
        if (it != kf_at.end()) return it->second;
        const Vector3d O = kf->GetCameraCenter();
        for (int k = 0; k < 3; k++) centers.push_back(O[k]);
        const int at = (int)kf_at.size();
        kf_at.emplace(kf, at);
        return at;
      };
      for (int j = 0; j < n; j++) {
        const Snap& s = S[idx[j]];
        pt_good[j] = s.bad ? 0 : 1;
        for (const auto& o : s.obs) {
          if (nd) obs_kf.push_back(kf_index(o.first));
          if (desc) {
            kf_good.push_back(o.first->isBad() ? 0 : 1);                          // (:276)
            const uint8_t* row = o.first->descriptors_.ptr((int)o.second);
            obs_desc.insert(obs_desc.end(), row, row + 32);
          }
        }
        off[j + 1] = off[j] + (int32_t)s.obs.size();
        if (nd && !s.bad && !s.obs.empty()) { ref_kf[j] = kf_index(s.ref); ref_level[j] = s.level; for (int k = 0; k < 3; k++) X[3 * (size_t)j + k] = s.X[k]; }
      }
      const int nobs = off[n];
      std::vector<int32_t> best(n, -1); std::vector<uint8_t> dout(32 * (size_t)n), wrote(n, 0);
      std::vector<double> normal(3 * (size_t)n); std::vector<float> mm(2 * (size_t)n);
      const std::vector<float>& table = tables[std::min(g, tables.size() - 1)];
      dropin::check(orbl_update_map_points(n, off.data(), X.data(), ref_kf.data(), ref_level.data(), pt_good.data(), nobs, nd ? obs_kf.data() : nullptr,
                                           desc ? obs_desc.data() : nullptr, desc ? kf_good.data() : nullptr, (int)kf_at.size(), centers.data(), table.data(),
                                           (int)table.size(), what & (ORBL_MP_DESC | ORBL_MP_NORMAL_DEPTH), best.data(), dout.data(), normal.data(), mm.data(),
                                           wrote.data()), "orbl_update_map_points");
      for (int j = 0; j < n; j++) {
        MapPoint* mp = points[idx[j]];
        const Snap& s = S[idx[j]];
        if (desc && best[j] >= 0) {
          const std::pair<KeyFrame*, size_t>& o = s.obs[best[j]];
          std::unique_lock<std::mutex> lock = lock_features(mp, 0);
          mp->descriptor_ = dropin::row_copy(o.first->descriptors_, (int)o.second, 0);       // (:311-314) descriptors[best_index].clone()
        }
        if (nd && wrote[j]) {
          Vector3d v;
          for (int k = 0; k < 3; k++) v[k] = normal[3 * (size_t)j + k];
          std::unique_lock<std::mutex> lock = lock_pose(mp, 0);                           // (:373-377)
          mp->max_distance_ = mm[2 * (size_t)j + 1];
          mp->min_distance_ = mm[2 * (size_t)j];
          mp->normal_vector_ = v;
        }
      }
    }
  }

  // LocalMapping::KeyFrameCulling (src/LocalMapping.cc:576-637, monocular) in ONE library call (orbl_keyframe_culling), the body of
  // that member function: `FrameOpsHip::KeyFrameCulling(current_keyframe_);`.  The candidates are GetVectorCovisibleKeyFrames() in
  // order; the map is flattened through the reference's own accessors, so under its lock scopes (GetMapPointMatches(), isBad(),
  // Observations(), GetObservations() take mutex_features_ / mutex_connections_ themselves; do_not_erase_ is read under
  // mutex_connections_ as KeyFrame::SetBadFlag reads it, src/KeyFrame.cc:462-468 - protected there: the friend declaration of
  // INTEGRATION.md section 4).  The library call reproduces the loop's order dependence (a culled keyframe's SetBadFlag() erases
  // observations and may turn points bad before the next candidate counts); then SetBadFlag() runs on the flagged keyframes in list
  // order, which applies exactly the state the call assumed.  Returns the number of keyframes flagged.
  // PRECONDITION, checked while flattening: the map is consistent - a candidate holds point p in slot i iff p's observations contain
  // (candidate, i), and every observation's index is a keypoint of its keyframe.  On a violation nothing is called and nothing is
  // changed: returns -1 (the caller falls back to its own loop).
  // (A member template over the keyframe type, KF = Types::KeyFrame at the call site: it is instantiated only where it is called, so a
  // data model without SetBadFlag() / do_not_erase_ can still instantiate the rest of FrameOpsT explicitly.)
  template <class KF> static int KeyFrameCulling(KF* current_keyframe, int th_obs = 3, double ratio = 0.9) {
    const std::vector<KF*> cands = current_keyframe->GetVectorCovisibleKeyFrames();          // (:581-582)
    const int ncand = (int)cands.size();
    if (ncand == 0) return 0;
    std::unordered_map<KF*, int> kf_at;
    auto kf_index = [&](KF* kf) { return kf_at.emplace(kf, (int)kf_at.size()).first->second; };
    std::unordered_map<MapPoint*, int> pt_at;
    std::vector<MapPoint*> pts;
    std::vector<std::vector<MapPoint*> > matches(ncand);
    std::vector<int32_t> cand_kf(ncand), slot_off(ncand + 1, 0), slot_pt, slot_level, slot_index;
    std::vector<uint8_t> cand_flags(ncand, 0);
    for (int c = 0; c < ncand; c++) {
      KF* kf = cands[c];
      if (kf_at.count(kf)) return -1;                               // (a keyframe listed twice)
      cand_kf[c] = kf_index(kf);
      bool keep;
      { std::unique_lock<std::mutex> lock = lock_connections(kf, 0); keep = kf->do_not_erase_; }
      cand_flags[c] = (uint8_t)((kf->id_ == 0 ? 1 : 0) | (keep ? 2 : 0));
      matches[c] = kf->GetMapPointMatches();                        // (:589)
      for (size_t i = 0; i < matches[c].size(); i++) {
        MapPoint* mp = matches[c][i];
        if (!mp) continue;
        if (i >= kf->undistort_keypoints_.size()) return -1;
        auto it = pt_at.find(mp);
        if (it == pt_at.end()) { it = pt_at.emplace(mp, (int)pts.size()).first; pts.push_back(mp); }
        slot_pt.push_back(it->second); slot_level.push_back(kf->undistort_keypoints_[i].octave); slot_index.push_back((int32_t)i);
      }
      slot_off[c + 1] = (int32_t)slot_pt.size();
    }
    const int npts = (int)pts.size();
    std::vector<int32_t> obs_off(npts + 1, 0), obs_kf, obs_level, pt_nobs(npts, 0);
    std::vector<uint8_t> pt_bad(npts, 0);
    std::vector<std::map<int, size_t> > own(npts);                  // per point: candidate -> the index its observation names
    for (int p = 0; p < npts; p++) {
      MapPoint* mp = pts[p];
      pt_bad[p] = mp->isBad() ? 1 : 0;                              // (:598)
      if (!pt_bad[p]) {
        pt_nobs[p] = mp->Observations();                            // (:606)
        const auto observations = mp->GetObservations();            // (:608-609)
        for (const auto& o : observations) {
          if (o.second >= o.first->undistort_keypoints_.size()) return -1;
          const int k = kf_index(o.first);
          if (k < ncand) own[p][k] = o.second;                      // (candidates were numbered first: index = list position)
          obs_kf.push_back(k); obs_level.push_back(o.first->undistort_keypoints_[o.second].octave);   // (:617-618)
        }
      }
      obs_off[p + 1] = (int32_t)obs_kf.size();
    }
    // consistency, both directions: every slot of a good point is the point's observation by that candidate, and every observation by a
    // candidate is one of its slots
    std::vector<size_t> n_slots_of(npts, 0);
    for (int c = 0; c < ncand; c++)
      for (int s = slot_off[c]; s < slot_off[c + 1]; s++) {
        const int p = slot_pt[s];
        if (pt_bad[p]) continue;
        auto it = own[p].find(c);
        if (it == own[p].end() || it->second != (size_t)slot_index[s]) return -1;
        n_slots_of[p]++;
      }
    for (int p = 0; p < npts; p++) {
      if (pt_bad[p]) continue;
      if (n_slots_of[p] != own[p].size()) return -1;
      for (const auto& o : own[p]) if (o.second >= matches[o.first].size() || matches[o.first][o.second] != pts[p]) return -1;
    }
    std::vector<uint8_t> culled(ncand, 0);
    std::vector<int32_t> n_redundant(ncand, 0), n_map_points(ncand, 0);
    dropin::check(orbl_keyframe_culling(ncand, cand_kf.data(), cand_flags.data(), slot_off.data(), slot_pt.data(), slot_level.data(), (int)kf_at.size(), npts,
                                        obs_off.data(), obs_kf.data(), obs_level.data(), pt_bad.data(), pt_nobs.data(), th_obs, ratio, culled.data(),
                                        n_redundant.data(), n_map_points.data(), nullptr, nullptr, nullptr), "orbl_keyframe_culling");
    int n = 0;
    for (int c = 0; c < ncand; c++)
      if (culled[c]) { cands[c]->SetBadFlag(); n++; }                // (:633-635)
    return n;
  }

  // Tracking::UpdateLocalKeyFrames (src/Tracking.cc:874-977) in ONE library call (orbt_update_local_keyframes), the body of that member
  // function: `FrameOpsHip::UpdateLocalKeyFrames(current_frame_, local_keyframes_, reference_keyframe_);`.  Only the part of the graph
  // the function can touch is flattened, through the reference's own accessors: the observers of the frame's points (the voted
  // keyframes), their GetBestCovisibilityKeyFrames(10), GetChilds() and GetParent(), and local_keyframes_ as the frame before left it.
  // The two pointer orders the reference's result depends on are passed on as they are: kf_rank = the keyframes' order under
  // std::less<KeyFrame*> (the iteration order of std::map<KeyFrame*, int> keyframeCounter), the children in the iteration order of the
  // std::set GetChilds() returns.  Afterwards: the frame's slots whose point is bad are cleared, and - unless nobody voted, where the
  // reference returns with everything as it was - local_keyframes is replaced, track_reference_for_frame_ = current_frame.id_ is written
  // on every keyframe of it, and reference_keyframe / current_frame.reference_keyframe_ are set when a voted keyframe is not bad.
  // Returns the library's status (ORBT_ULM_OK / ORBT_ULM_NO_VOTES).
  // (Member templates over the frame and keyframe types: instantiated only where they are called, as KeyFrameCulling is.)
  template <class F, class KF> static int UpdateLocalKeyFrames(F& current_frame, std::vector<KF*>& local_keyframes, KF*& reference_keyframe) {
    typedef typename std::remove_pointer<typename std::decay<decltype(current_frame.map_points_[0])>::type>::type MP;
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*> kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    std::unordered_map<MP*, int> pt_at;
    const int n_kp = (int)current_frame.map_points_.size();
    std::vector<int32_t> frame_pt(n_kp, -1), obs_off(1, 0), obs_kf;
    std::vector<uint8_t> pt_bad;
    for (int i = 0; i < n_kp; i++) {                                // (:877-892)
      MP* mp = current_frame.map_points_[i];
      if (!mp) continue;
      auto it = pt_at.find(mp);
      if (it == pt_at.end()) {
        it = pt_at.emplace(mp, (int)pt_bad.size()).first;
        const bool bad = mp->isBad();
        pt_bad.push_back(bad ? 1 : 0);
        if (!bad) { const auto observations = mp->GetObservations(); for (const auto& o : observations) obs_kf.push_back(kf_index(o.first)); }
        obs_off.push_back((int32_t)obs_kf.size());
      }
      frame_pt[i] = it->second;
    }
    const int n_voted = (int)kfs.size();                            // (only these are walked: their rows are the ones the call reads)
    std::vector<int32_t> cov_off(1, 0), cov_kf, child_off(1, 0), child_kf, parent;
    for (int k = 0; k < n_voted; k++) {
      KF* kf = kfs[k];
      const std::vector<KF*> neighbours = kf->GetBestCovisibilityKeyFrames(10);            // (:932-933)
      for (size_t j = 0; j < neighbours.size() && j < 10; j++) cov_kf.push_back(kf_index(neighbours[j]));
      cov_off.push_back((int32_t)cov_kf.size());
      const std::set<KF*> children = kf->GetChilds();                                    // (:949)
      for (KF* c : children) child_kf.push_back(kf_index(c));
      child_off.push_back((int32_t)child_kf.size());
      KF* par = kf->GetParent();                                                          // (:963)
      parent.push_back(par ? kf_index(par) : -1);
    }
    std::vector<int32_t> prev(local_keyframes.size());
    for (size_t i = 0; i < local_keyframes.size(); i++) prev[i] = kf_index(local_keyframes[i]);
    const int nkf = (int)kfs.size(), npts = (int)pt_bad.size();
    cov_off.resize(nkf + 1, (int32_t)cov_kf.size()); child_off.resize(nkf + 1, (int32_t)child_kf.size()); parent.resize(nkf, -1);
    std::vector<uint8_t> kf_bad(nkf);
    for (int k = 0; k < nkf; k++) kf_bad[k] = kfs[k]->isBad() ? 1 : 0;
    std::vector<int32_t> by_pointer(nkf), kf_rank(nkf);             // the order of std::map<KeyFrame*, int>
    for (int k = 0; k < nkf; k++) by_pointer[k] = k;
    std::sort(by_pointer.begin(), by_pointer.end(), [&](int a, int b) { return std::less<KF*>()(kfs[a], kfs[b]); });
    for (int r = 0; r < nkf; r++) kf_rank[by_pointer[r]] = r;
    std::vector<int32_t> frame_pt_out(n_kp, -1), local_kf(std::max(nkf, 1));
    int32_t n_local = 0, ref = -1, status = 0;
    dropin::check(orbt_update_local_keyframes(n_kp, frame_pt.data(), npts, pt_bad.data(), obs_off.data(), obs_kf.data(), nkf, kf_bad.data(), kf_rank.data(), parent.data(),
                                              cov_off.data(), cov_kf.data(), child_off.data(), child_kf.data(), (int)prev.size(), prev.data(), nkf,
                                              frame_pt_out.data(), local_kf.data(), &n_local, &ref, &status, nullptr), "orbt_update_local_keyframes");
    for (int i = 0; i < n_kp; i++)
      if (frame_pt[i] >= 0 && frame_pt_out[i] < 0) current_frame.map_points_[i] = nullptr;          // (:889)
    if (status == ORBT_ULM_NO_VOTES) return status;                 // (:894-896)
    local_keyframes.clear();
    for (int i = 0; i < n_local; i++) {
      KF* kf = kfs[local_kf[i]];
      local_keyframes.push_back(kf);
      kf->track_reference_for_frame_ = current_frame.id_;
    }
    if (ref >= 0) { reference_keyframe = kfs[ref]; current_frame.reference_keyframe_ = reference_keyframe; }      // (:973-976)
    return status;
  }

  // Tracking::UpdateLocalPoints (src/Tracking.cc:847-872) in ONE library call (orbt_update_local_points):
  // `FrameOpsHip::UpdateLocalPoints(current_frame_, local_keyframes_, local_map_points_);`.  The slot tables (GetMapPointMatches()) of the
  // local keyframes only are flattened, never the whole map.  local_map_points is replaced and track_reference_for_frame_ =
  // current_frame.id_ is written on every point of it.  PRECONDITION (the reference's own): no point carries that id at entry.
  template <class F, class KF, class MP> static void UpdateLocalPoints(F& current_frame, const std::vector<KF*>& local_keyframes, std::vector<MP*>& local_map_points) {
    std::unordered_map<MP*, int> pt_at;
    std::vector<MP*> pts;
    std::vector<int32_t> slot_off(1, 0), slot_pt;
    std::vector<uint8_t> pt_bad;
    for (KF* kf : local_keyframes) {
      const std::vector<MP*> matches = kf->GetMapPointMatches();    // (:854)
      for (MP* mp : matches) {
        if (!mp) { slot_pt.push_back(-1); continue; }
        auto it = pt_at.find(mp);
        if (it == pt_at.end()) { it = pt_at.emplace(mp, (int)pts.size()).first; pts.push_back(mp); pt_bad.push_back(mp->isBad() ? 1 : 0); }
        slot_pt.push_back(it->second);
      }
      slot_off.push_back((int32_t)slot_pt.size());
    }
    const int npts = (int)pts.size();
    std::vector<int32_t> local_pt(std::max(npts, 1));
    int32_t n_local = 0;
    dropin::check(orbt_update_local_points((int)local_keyframes.size(), slot_off.data(), slot_pt.data(), npts, pt_bad.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr, 0, nullptr, 0, nullptr, npts, local_pt.data(), &n_local, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr), "orbt_update_local_points");
    local_map_points.clear();
    for (int j = 0; j < n_local; j++) {
      MP* mp = pts[local_pt[j]];
      local_map_points.push_back(mp);
      mp->track_reference_for_frame_ = current_frame.id_;
    }
  }

  // KeyFrame::UpdateConnections (src/KeyFrame.cc:314-398) on every keyframe of `keyframes`, in order, in ONE library call
  // (orbl_update_connections): `FrameOpsHip::UpdateConnections({current_keyframe_});` in LocalMapping (src/LocalMapping.cc:161, :487),
  // `FrameOpsHip::UpdateConnections(current_connected_keyframes_, &loop_connections);` for the loop of LoopClosing::CorrectLoop
  // (src/LoopClosing.cc:551-573), which then holds what :561-572 put into loop_connections.  Only the part of the graph the loop can touch
  // is flattened: the targets, the observers of their points, and connected_keyframe_weights_ of those keyframes (the keyframes these
  // maps name are indexed too, with empty rows: nothing is ever sent to them).  kf_rank = the order under std::less<KeyFrame*>, which is the
  // iteration order of keyframe_counter, the tie-break of both sorts and the order of the std::set.  Written back on the keyframes the
  // loop would have written: connected_keyframe_weights_, ordered_connected_keyframes_, ordered_weights_, and for a first connection
  // parent_ + AddChild and is_first_connection_ - members the reference keeps protected: the friend declaration of INTEGRATION.md
  // section 4.  Each keyframe's members are read and written under its mutex_connections_; the caller holds what the reference's call
  // sites hold (nothing in LocalMapping, Map::mutex_map_update_ in CorrectLoop).  A keyframe listed twice: nothing is called, nothing is
  // changed, returns -1.  Otherwise returns the number of keyframes written.
  // (A member template over the keyframe type, as KeyFrameCulling is.)
  template <class KF> static int UpdateConnections(const std::vector<KF*>& keyframes, std::map<KF*, std::set<KF*> >* loop_connections = nullptr, int th = 15) {
    typedef typename std::remove_pointer<typename std::decay<decltype(keyframes[0]->GetMapPointMatches()[0])>::type>::type MP;
    const int ntgt = (int)keyframes.size();
    if (ntgt == 0) return 0;
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*> kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    std::vector<int32_t> tgt_kf(ntgt);
    for (int t = 0; t < ntgt; t++) {
      if (kf_at.count(keyframes[t])) return -1;
      tgt_kf[t] = kf_index(keyframes[t]);                           // (targets are numbered first: index = list position)
    }
    std::unordered_map<MP*, int> pt_at;
    std::vector<int32_t> slot_off(1, 0), slot_pt, obs_off(1, 0), obs_kf, prev_off(1, 0), prev_kf;
    std::vector<uint8_t> tgt_flags(ntgt, 0), pt_bad;
    for (int t = 0; t < ntgt; t++) {
      KF* kf = keyframes[t];
      { std::unique_lock<std::mutex> lock = lock_connections(kf, 0); tgt_flags[t] = (kf->is_first_connection_ && kf->id_ != 0) ? 1 : 0; }      // (:392)
      const std::vector<MP*> matches = kf->GetMapPointMatches();    // (:319-322)
      for (MP* mp : matches) {
        if (!mp) { slot_pt.push_back(-1); continue; }
        auto it = pt_at.find(mp);
        if (it == pt_at.end()) {
          it = pt_at.emplace(mp, (int)pt_bad.size()).first;
          const bool bad = mp->isBad();                             // (:333)
          pt_bad.push_back(bad ? 1 : 0);
          if (!bad) { const auto observations = mp->GetObservations(); for (const auto& o : observations) obs_kf.push_back(kf_index(o.first)); }      // (:335)
          obs_off.push_back((int32_t)obs_kf.size());
        }
        slot_pt.push_back(it->second);
      }
      slot_off.push_back((int32_t)slot_pt.size());
      if (loop_connections) {
        const std::vector<KF*> previous = kf->GetVectorCovisibleKeyFrames();               // (LoopClosing.cc:556-557)
        for (KF* p : previous) prev_kf.push_back(kf_index(p));
        prev_off.push_back((int32_t)prev_kf.size());
      }
    }
    const int n_rows = (int)kfs.size();                             // (targets and observers: the rows the call can read)
    std::vector<int32_t> conn_off(1, 0), conn_kf, conn_w;
    for (int k = 0; k < n_rows; k++) {
      std::map<KF*, int> weights;
      { std::unique_lock<std::mutex> lock = lock_connections(kfs[k], 0); weights = kfs[k]->connected_keyframe_weights_; }
      for (const auto& w : weights) { conn_kf.push_back(kf_index(w.first)); conn_w.push_back(w.second); }
      conn_off.push_back((int32_t)conn_kf.size());
    }
    const int nkf = (int)kfs.size(), npts = (int)pt_bad.size(), nconn = (int)conn_kf.size();
    conn_off.resize(nkf + 1, (int32_t)nconn);
    std::vector<int32_t> by_pointer(nkf), kf_rank(nkf);
    for (int k = 0; k < nkf; k++) by_pointer[k] = k;
    std::sort(by_pointer.begin(), by_pointer.end(), [&](int a, int b) { return std::less<KF*>()(kfs[a], kfs[b]); });
    for (int r = 0; r < nkf; r++) kf_rank[by_pointer[r]] = r;
    // capacities no call exceeds: a written map is a counter (at most nkf - 1 entries) or an input row plus one entry per target
    const size_t cap = std::min((size_t)nkf * (size_t)std::max(nkf - 1, 0), (size_t)nconn + 2 * (size_t)ntgt * (size_t)nkf);
    const size_t cap_link = loop_connections ? (size_t)ntgt * (size_t)nkf : 0;
    if (cap > 0x7FFFFFFFu || cap_link > 0x7FFFFFFFu) throw std::runtime_error("FrameOpsT::UpdateConnections: keyframe list too large for one call");
    std::vector<int32_t> tgt_status(ntgt), tgt_parent(ntgt), aff_kf(nkf), oconn_off(nkf + 1), oord_off(nkf + 1), oconn_kf(std::max<size_t>(cap, 1)),
        oconn_w(std::max<size_t>(cap, 1)), oord_kf(std::max<size_t>(cap, 1)), oord_w(std::max<size_t>(cap, 1)), link_off(ntgt + 1), link_kf(std::max<size_t>(cap_link, 1));
    int32_t counts[4] = {0, 0, 0, 0};
    dropin::check(orbl_update_connections(ntgt, tgt_kf.data(), tgt_flags.data(), slot_off.data(), slot_pt.data(), nkf, npts, obs_off.data(), obs_kf.data(), pt_bad.data(),
                                          kf_rank.data(), conn_off.data(), conn_kf.data(), conn_w.data(), loop_connections ? prev_off.data() : nullptr,
                                          loop_connections ? prev_kf.data() : nullptr, th, nkf, (int)cap, (int)cap, (int)cap_link, tgt_status.data(),
                                          tgt_parent.data(), aff_kf.data(), oconn_off.data(), oconn_kf.data(), oconn_w.data(), oord_off.data(), oord_kf.data(),
                                          oord_w.data(), loop_connections ? link_off.data() : nullptr, loop_connections ? link_kf.data() : nullptr, counts),
                  "orbl_update_connections");
    for (int i = 0; i < counts[0]; i++) {                           // (:383-390, :172-193)
      KF* kf = kfs[aff_kf[i]];
      std::map<KF*, int> weights;
      for (int e = oconn_off[i]; e < oconn_off[i + 1]; e++) weights.emplace_hint(weights.end(), kfs[oconn_kf[e]], oconn_w[e]);      // (rows come in map order)
      std::vector<KF*> ordered; std::vector<int> ordered_w;
      ordered.reserve(oord_off[i + 1] - oord_off[i]); ordered_w.reserve(oord_off[i + 1] - oord_off[i]);
      for (int e = oord_off[i]; e < oord_off[i + 1]; e++) { ordered.push_back(kfs[oord_kf[e]]); ordered_w.push_back(oord_w[e]); }
      std::unique_lock<std::mutex> lock = lock_connections(kf, 0);
      kf->connected_keyframe_weights_.swap(weights); kf->ordered_connected_keyframes_.swap(ordered); kf->ordered_weights_.swap(ordered_w);
    }
    for (int t = 0; t < ntgt; t++) {
      KF* kf = keyframes[t];
      if (tgt_status[t] == 0 && tgt_parent[t] >= 0) {               // (:392-396; AddChild takes the parent's lock itself)
        KF* parent = kfs[tgt_parent[t]];
        { std::unique_lock<std::mutex> lock = lock_connections(kf, 0); kf->parent_ = parent; kf->is_first_connection_ = false; }
        parent->AddChild(kf);
      }
      if (loop_connections) {                                       // (LoopClosing.cc:561-572)
        std::set<KF*>& links = (*loop_connections)[kf];
        links.clear();
        for (int e = link_off[t]; e < link_off[t + 1]; e++) links.insert(kfs[link_kf[e]]);
      }
    }
    return counts[0];
  }

  // KeyFrame::SetBadFlag (src/KeyFrame.cc:460-553) on every keyframe of `keyframes`, in order, in ONE library call (orbl_set_bad_keyframes):
  // `FrameOpsHip::SetBadFlags(culled);` for the keyframes LocalMapping::KeyFrameCulling decided on.  Flattened, through the reference's
  // accessors and under its lock scopes: the targets; the keyframes their maps name, their parents and children and the observers of
  // their points ("rows": map, ordered lists, parent, children, pose, slots - of a keyframe that is no target only the slots that hold
  // a target's point); the keyframes those tables name are indexed too, with empty rows: nothing of them is read or written.  kf_rank =
  // the order under std::less<KeyFrame*>.  Written back on the rows that changed: connected_keyframe_weights_, ordered_connected_keyframes_,
  // ordered_weights_, parent_, childrens_, EraseMapPointMatch; on the points: observations_, n_observations_, reference_keyframe_,
  // is_bad_; on the targets that went: Tcp_, is_bad_ - members the reference keeps protected: the friend declaration of INTEGRATION.md
  // section 4.  Then the caller-side remainder: do_to_be_erased_ on a target with do_not_erase_ (:465-468), map_->EraseMapPoint of every
  // point that turned bad, map_->EraseKeyFrame and keyframe_database_->erase of every keyframe that went (:551-552).  A keyframe listed
  // twice, or a map the library refuses as inconsistent (a target that is bad or has no parent, an observation whose slot does not
  // hold its point): nothing is called, nothing is changed, returns -1.  Otherwise returns the number of keyframes that went bad.
  // (A member template over the keyframe type, as UpdateConnections is.)
  template <class KF> static int SetBadFlags(const std::vector<KF*>& keyframes) {
    typedef typename std::remove_pointer<typename std::decay<decltype(keyframes[0]->GetMapPointMatches()[0])>::type>::type MP;
    typedef typename std::decay<decltype(keyframes[0]->GetPose())>::type M4;
    const int ntgt = (int)keyframes.size();
    if (ntgt == 0) return 0;
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*> kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    std::vector<int32_t> tgt_kf(ntgt);
    std::vector<uint8_t> tgt_flags(ntgt, 0);
    for (int t = 0; t < ntgt; t++) {
      if (kf_at.count(keyframes[t])) return -1;
      tgt_kf[t] = kf_index(keyframes[t]);                           // (targets are numbered first: index = list position)
    }
    // the points of the targets with their observations, and the rows
    std::unordered_map<MP*, int> pt_at;
    std::vector<MP*> pts;
    std::vector<std::map<KF*, size_t> > pt_obs;
    for (int t = 0; t < ntgt; t++) {
      KF* kf = keyframes[t];
      bool keep; KF* parent; std::set<KF*> children; std::map<KF*, int> weights;
      {
        std::unique_lock<std::mutex> lock = lock_connections(kf, 0);
        keep = kf->do_not_erase_; parent = kf->parent_; children = kf->childrens_; weights = kf->connected_keyframe_weights_;
      }
      tgt_flags[t] = (uint8_t)((kf->id_ == 0 ? 1 : 0) | (keep ? 2 : 0));       // (:463-468)
      if (tgt_flags[t]) continue;
      if (parent) kf_index(parent);
      for (KF* c : children) kf_index(c);
      for (const auto& w : weights) kf_index(w.first);
      const std::vector<MP*> matches = kf->GetMapPointMatches();
      for (MP* mp : matches) {
        if (!mp || pt_at.count(mp)) continue;
        pt_at.emplace(mp, (int)pts.size());
        pts.push_back(mp);
        pt_obs.push_back(mp->GetObservations());
        for (const auto& o : pt_obs.back()) kf_index(o.first);
      }
    }
    const int n_rows = (int)kfs.size(), npts = (int)pts.size();
    std::vector<int32_t> kf_parent, child_off(1, 0), child_kf, conn_off(1, 0), conn_kf, conn_w, ord_off(1, 0), ord_kf, ord_w, slot_off(1, 0), slot_pt;
    std::vector<uint8_t> kf_bad;
    for (int k = 0; k < n_rows; k++) {
      KF* kf = kfs[k];
      KF* parent; std::set<KF*> children; std::map<KF*, int> weights; std::vector<KF*> ordered; std::vector<int> ordered_w; bool bad;
      {
        std::unique_lock<std::mutex> lock = lock_connections(kf, 0);
        parent = kf->parent_; children = kf->childrens_; weights = kf->connected_keyframe_weights_; ordered = kf->ordered_connected_keyframes_;
        ordered_w = kf->ordered_weights_; bad = kf->is_bad_;
      }
      kf_parent.push_back(parent ? kf_index(parent) : -1);
      kf_bad.push_back(bad ? 1 : 0);
      for (KF* c : children) child_kf.push_back(kf_index(c));
      child_off.push_back((int32_t)child_kf.size());
      for (const auto& w : weights) { conn_kf.push_back(kf_index(w.first)); conn_w.push_back(w.second); }
      conn_off.push_back((int32_t)conn_kf.size());
      if (ordered.size() != ordered_w.size()) return -1;
      for (size_t i = 0; i < ordered.size(); i++) { ord_kf.push_back(kf_index(ordered[i])); ord_w.push_back(ordered_w[i]); }
      ord_off.push_back((int32_t)ord_kf.size());
      const std::vector<MP*> matches = kf->GetMapPointMatches();
      for (MP* mp : matches) { auto it = mp ? pt_at.find(mp) : pt_at.end(); slot_pt.push_back(it == pt_at.end() ? -1 : it->second); }
      slot_off.push_back((int32_t)slot_pt.size());
    }
    const int nkf = (int)kfs.size();                               // (the keyframes the rows name beyond themselves: empty rows)
    for (int k = n_rows; k < nkf; k++) { kf_parent.push_back(-1); kf_bad.push_back(kfs[k]->isBad() ? 1 : 0); }
    child_off.resize(nkf + 1, child_off.back()); conn_off.resize(nkf + 1, conn_off.back()); ord_off.resize(nkf + 1, ord_off.back()); slot_off.resize(nkf + 1, slot_off.back());
    std::vector<double> Tcw(12 * (size_t)nkf, 0.0);
    for (int k = 0; k < nkf; k++) {
      const M4 T = kfs[k]->GetPose();
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) Tcw[12 * (size_t)k + 4 * r + c] = T(r, c);
    }
    std::vector<int32_t> by_pointer(nkf), kf_rank(nkf);
    for (int k = 0; k < nkf; k++) by_pointer[k] = k;
    std::sort(by_pointer.begin(), by_pointer.end(), [&](int a, int b) { return std::less<KF*>()(kfs[a], kfs[b]); });
    for (int r = 0; r < nkf; r++) kf_rank[by_pointer[r]] = r;
    std::vector<int32_t> obs_off(1, 0), obs_kf, obs_slot, pt_nobs(npts), pt_ref(npts);
    std::vector<uint8_t> pt_bad(npts);
    for (int p = 0; p < npts; p++) {
      for (const auto& o : pt_obs[p]) { obs_kf.push_back(kf_at[o.first]); obs_slot.push_back((int32_t)o.second); }
      obs_off.push_back((int32_t)obs_kf.size());
      pt_nobs[p] = pts[p]->Observations(); pt_bad[p] = pts[p]->isBad() ? 1 : 0;
      std::unique_lock<std::mutex> lock = lock_features(pts[p], 0);
      auto it = pts[p]->reference_keyframe_ ? kf_at.find(pts[p]->reference_keyframe_) : kf_at.end();
      pt_ref[p] = it == kf_at.end() ? -1 : it->second;             // (a reference keyframe outside the rows cannot be a target)
    }
    const size_t cap_ord = conn_kf.size() + ord_kf.size(), cap_child = child_kf.size() + (size_t)ntgt * (size_t)nkf;
    if (cap_ord > 0x7FFFFFFFu || cap_child > 0x7FFFFFFFu) throw std::runtime_error("FrameOpsT::SetBadFlags: keyframe list too large for one call");
    const std::vector<int32_t> parent_in = kf_parent, slot_in = slot_pt;
    std::vector<uint8_t> pt_bad_in = pt_bad, obs_erased(std::max<size_t>(obs_kf.size(), 1), 0);
    std::vector<int32_t> tgt_status(ntgt), oconn_off(nkf + 1), oconn_kf(std::max<size_t>(conn_kf.size(), 1)), oconn_w(std::max<size_t>(conn_kf.size(), 1)),
        oord_off(nkf + 1), oord_kf(std::max<size_t>(cap_ord, 1)), oord_w(std::max<size_t>(cap_ord, 1)), ochild_off(nkf + 1), ochild_kf(std::max<size_t>(cap_child, 1));
    std::vector<double> Tcp(12 * (size_t)ntgt);
    obs_kf.resize(std::max<size_t>(obs_kf.size(), 1)); obs_slot.resize(obs_kf.size()); slot_pt.resize(std::max<size_t>(slot_pt.size(), 1), -1);
    child_kf.resize(std::max<size_t>(child_kf.size(), 1)); conn_kf.resize(std::max<size_t>(conn_kf.size(), 1)); conn_w.resize(conn_kf.size());
    ord_kf.resize(std::max<size_t>(ord_kf.size(), 1)); ord_w.resize(ord_kf.size());
    pt_bad.resize(std::max(npts, 1)); pt_nobs.resize(std::max(npts, 1)); pt_ref.resize(std::max(npts, 1));
    int32_t counts[6] = {0, 0, 0, 0, 0, 0};
    const int rc = orbl_set_bad_keyframes(ntgt, tgt_kf.data(), tgt_flags.data(), nullptr, nkf, kf_bad.data(), kf_parent.data(), kf_rank.data(), Tcw.data(), child_off.data(),
                                          child_kf.data(), conn_off.data(), conn_kf.data(), conn_w.data(), ord_off.data(), ord_kf.data(), ord_w.data(), npts, slot_off.data(),
                                          slot_pt.data(), pt_bad.data(), pt_nobs.data(), pt_ref.data(), obs_off.data(), obs_kf.data(), obs_slot.data(), obs_erased.data(),
                                          (int)cap_ord, (int)cap_child, tgt_status.data(), Tcp.data(), oconn_off.data(), oconn_kf.data(), oconn_w.data(), oord_off.data(),
                                          oord_kf.data(), oord_w.data(), ochild_off.data(), ochild_kf.data(), counts);
    if (rc == ORBHIP_EINVAL) return -1;                             // (an inconsistent map: nothing was changed)
    dropin::check(rc, "orbl_set_bad_keyframes");
    for (int k = 0; k < n_rows; k++) {                              // the rows that changed
      KF* kf = kfs[k];
      const int c0 = oconn_off[k], c1 = oconn_off[k + 1], o0 = oord_off[k], o1 = oord_off[k + 1], h0 = ochild_off[k], h1 = ochild_off[k + 1];
      const bool conn_changed = c1 - c0 != conn_off[k + 1] - conn_off[k];      // (a row only ever loses entries)
      const bool ord_changed = o1 - o0 != ord_off[k + 1] - ord_off[k] || !std::equal(oord_kf.begin() + o0, oord_kf.begin() + o1, ord_kf.begin() + ord_off[k]) ||
                               !std::equal(oord_w.begin() + o0, oord_w.begin() + o1, ord_w.begin() + ord_off[k]);
      std::set<int32_t> child_in(child_kf.begin() + child_off[k], child_kf.begin() + child_off[k + 1]), child_out(ochild_kf.begin() + h0, ochild_kf.begin() + h1);
      std::map<KF*, int> weights; std::vector<KF*> ordered; std::vector<int> ordered_w; std::set<KF*> children;
      for (int e = c0; e < c1; e++) weights[kfs[oconn_kf[e]]] = oconn_w[e];
      for (int e = o0; e < o1; e++) { ordered.push_back(kfs[oord_kf[e]]); ordered_w.push_back(oord_w[e]); }
      for (int e = h0; e < h1; e++) children.insert(kfs[ochild_kf[e]]);
      {
        std::unique_lock<std::mutex> lock = lock_connections(kf, 0);
        if (conn_changed) kf->connected_keyframe_weights_.swap(weights);
        if (ord_changed) { kf->ordered_connected_keyframes_.swap(ordered); kf->ordered_weights_.swap(ordered_w); }
        if (child_in != child_out) kf->childrens_.swap(children);
        if (kf_parent[k] != parent_in[k]) kf->parent_ = kfs[kf_parent[k]];
      }
      for (int s = slot_off[k]; s < slot_off[k + 1]; s++)
        if (slot_in[s] >= 0 && slot_pt[s] < 0) kf->EraseMapPointMatch((size_t)(s - slot_off[k]));       // (MapPoint::SetBadFlag, src/MapPoint.cc:183-188)
    }
    std::vector<MP*> turned_bad;
    for (int p = 0; p < npts; p++) {                                // (src/MapPoint.cc:140-191)
      bool any = false;
      for (int e = obs_off[p]; e < obs_off[p + 1]; e++) any |= obs_erased[e] != 0;
      if (!any) continue;
      MP* mp = pts[p];
      const bool bad = pt_bad[p] && !pt_bad_in[p];
      {
        std::unique_lock<std::mutex> lock1 = lock_features(mp, 0);
        std::unique_lock<std::mutex> lock2 = bad ? lock_pose(mp, 0) : std::unique_lock<std::mutex>();
        for (int e = obs_off[p]; e < obs_off[p + 1]; e++) if (obs_erased[e]) mp->observations_.erase(kfs[obs_kf[e]]);
        mp->n_observations_ = pt_nobs[p];
        if (pt_ref[p] >= 0) mp->reference_keyframe_ = kfs[pt_ref[p]];
        if (bad) mp->is_bad_ = true;
      }
      if (bad) turned_bad.push_back(mp);
    }
    for (MP* mp : turned_bad) mp->map_->EraseMapPoint(mp);          // (:190)
    for (int t = 0; t < ntgt; t++) {
      KF* kf = keyframes[t];
      if (tgt_status[t] == 2) { std::unique_lock<std::mutex> lock = lock_connections(kf, 0); kf->do_to_be_erased_ = true; }       // (:466)
      if (tgt_status[t] != 0) continue;
      M4 T = kf->GetPose();
      for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T(i, j) = Tcp[12 * (size_t)t + 4 * i + j];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      { std::unique_lock<std::mutex> lock = lock_connections(kf, 0); kf->Tcp_ = T; kf->is_bad_ = true; }        // (:547-548)
      kf->map_->EraseKeyFrame(kf);                                  // (:551-552)
      kf->keyframe_database_->erase(kf);
    }
    return counts[0];
  }

  // The front of LoopClosing::ComputeSim3, src/LoopClosing.cc:250-277, for every candidate in ONE library call (orbl_loop_sim3_candidates):
  //     std::vector<std::vector<MapPoint*> > map_point_matches_vector;
  //     FrameOpsHip::LoopSim3Data<MapPoint> data;
  //     int n_candidates = FrameOpsHip::LoopSim3Candidates(current_keyframe_, enough_consistent_candidates_, map_point_matches_vector, &data);
  // matches_out[i] is the vector of :262 (for a bad candidate it stays empty, as the reference leaves it), data->discarded[i] the flag of
  // :258 / :266, and rows [off[i], off[i + 1]) of data hold what Sim3Solver's constructor builds for candidate i (src/Sim3Solver.cc:73-109)
  // in the layout orbt_sim3_iterate_batch_device and Sim3SolverT take.  The current keyframe, the candidates, the points in their slots and
  // those points' observations of these keyframes are flattened; level_sigma2s_ is the current keyframe's (every keyframe copies the one
  // extractor's).  SetNotErase (:255) stays with the caller.  Returns the number of candidates kept.
  template <class MP> struct LoopSim3Data {
    std::vector<bool> discarded; std::vector<int> nmatches;
    std::vector<int32_t> off, matched_indices_1;                      // rows per candidate (CSR); matched_indices_1_ per row
    std::vector<double> X1c, X2c;                                     // X3Dsc1_ / X3Dsc2_ [rows][3]
    std::vector<float> max_err1, max_err2, K1, K2;                    // max_errors_1_ / _2_ [rows]; (fx, fy, cx, cy) [candidates][4]
    std::vector<MP*> map_points_1, map_points_2;                      // map_points_1_ / _2_ [rows]
  };
  template <class KF, class MP>
  static int LoopSim3Candidates(KF* current_keyframe, const std::vector<KF*>& candidates, std::vector<std::vector<MP*> >& matches_out, LoopSim3Data<MP>* data,
                                float nnratio = 0.75f, bool check_orientation = true, int min_matches = 20) {
    const int n_cand = (int)candidates.size();
    matches_out.assign((size_t)n_cand, std::vector<MP*>());
    *data = LoopSim3Data<MP>();
    data->off.assign((size_t)n_cand + 1, 0);
    if (n_cand == 0) return 0;
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*> kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    const int32_t cur = kf_index(current_keyframe);
    std::vector<int32_t> cand_kf((size_t)n_cand);
    for (int c = 0; c < n_cand; c++) cand_kf[c] = kf_index(candidates[c]);
    const int nkf = (int)kfs.size();
    std::unordered_map<MP*, int> pt_at;
    std::vector<MP*> pts;
    std::vector<std::vector<MP*> > held((size_t)nkf);
    std::vector<int32_t> slot_off(1, 0), slot_pt, slot_level, fv_off(1, 0), ent_off(1, 0), ent;
    std::vector<uint32_t> node;
    std::vector<float> angle, K4(4 * (size_t)nkf);
    std::vector<uint8_t> desc, kf_bad((size_t)nkf), pt_bad;
    std::vector<double> Tcw(12 * (size_t)nkf), X;
    for (int k = 0; k < nkf; k++) {
      KF* kf = kfs[k];
      held[k] = kf->GetMapPointMatches();
      const int n = (int)kf->undistort_keypoints_.size();
      for (int i = 0; i < n; i++) {
        MP* mp = i < (int)held[k].size() ? held[k][i] : nullptr;
        int p = -1;
        if (mp) {
          auto it = pt_at.find(mp);
          if (it == pt_at.end()) { it = pt_at.emplace(mp, (int)pts.size()).first; pts.push_back(mp); }
          p = it->second;
        }
        slot_pt.push_back(p); slot_level.push_back(kf->undistort_keypoints_[i].octave); angle.push_back(kf->undistort_keypoints_[i].angle);
        const uint8_t* d = kf->descriptors_.ptr(i);                   // (cv::Mat rows may be padded: copied row by row)
        desc.insert(desc.end(), d, d + 32);
      }
      slot_off.push_back((int32_t)slot_pt.size());
      for (auto it = kf->feature_vector_.begin(); it != kf->feature_vector_.end(); ++it) {
        node.push_back((uint32_t)it->first);
        for (auto v : it->second) ent.push_back((int32_t)v);
        ent_off.push_back((int32_t)ent.size());
      }
      fv_off.push_back((int32_t)node.size());
      kf_bad[k] = kf->isBad() ? 1 : 0;
      const auto T = kf->GetPose();
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) Tcw[12 * (size_t)k + 4 * r + c] = T(r, c);
      K4[4 * (size_t)k] = kf->fx_; K4[4 * (size_t)k + 1] = kf->fy_; K4[4 * (size_t)k + 2] = kf->cx_; K4[4 * (size_t)k + 3] = kf->cy_;
    }
    const int npts = (int)pts.size();
    std::vector<int32_t> obs_off(1, 0), obs_kf, obs_slot;
    for (MP* mp : pts) {                                              // (only the observations GetIndexInKeyFrame can be asked about)
      pt_bad.push_back(mp->isBad() ? 1 : 0);
      const auto P = mp->GetWorldPos();
      for (int k = 0; k < 3; k++) X.push_back(P[k]);
      const auto observations = mp->GetObservations();
      for (const auto& o : observations) {
        auto it = kf_at.find(o.first);
        if (it != kf_at.end()) { obs_kf.push_back(it->second); obs_slot.push_back((int32_t)o.second); }
      }
      obs_off.push_back((int32_t)obs_kf.size());
    }
    const std::vector<float> sigma2(current_keyframe->level_sigma2s_.begin(), current_keyframe->level_sigma2s_.end());
    const int n1 = slot_off[cur + 1] - slot_off[cur];
    const size_t cap_rows = (size_t)n_cand * (size_t)n1, nc = (size_t)n_cand;
    std::vector<int32_t> m12(std::max<size_t>(cap_rows, 1), -1), nm(nc), status(nc), i1(std::max<size_t>(cap_rows, 1)), p1(i1.size()), p2(i1.size());
    std::vector<double> X1(3 * i1.size()), X2(3 * i1.size());
    std::vector<float> e1(i1.size()), e2(i1.size());
    data->K1.assign(4 * nc, 0.f); data->K2.assign(4 * nc, 0.f);
    int32_t counts[2] = {0, 0};
    dropin::check(orbl_loop_sim3_candidates(cur, n_cand, cand_kf.data(), nkf, kf_bad.data(), Tcw.data(), K4.data(), slot_off.data(), slot_pt.data(), slot_level.data(),
                                            angle.data(), desc.data(), fv_off.data(), node.data(), ent_off.data(), ent.data(), npts, pt_bad.data(), X.data(), obs_off.data(),
                                            obs_kf.data(), obs_slot.data(), sigma2.data(), (int)sigma2.size(), nnratio, check_orientation ? 1 : 0, min_matches, n1,
                                            (int)cap_rows, m12.data(), nm.data(), status.data(), data->K1.data(), data->K2.data(), data->off.data(), X1.data(), X2.data(),
                                            e1.data(), e2.data(), i1.data(), p1.data(), p2.data(), counts),
                  "orbl_loop_sim3_candidates");
    const size_t rows = (size_t)counts[0];
    data->discarded.resize(nc); data->nmatches.assign(nm.begin(), nm.end());
    for (int c = 0; c < n_cand; c++) {
      data->discarded[c] = status[c] != 0;
      if (status[c] == 1) continue;                                   // (:257-260: SearchByBoW never ran, the vector stays empty)
      const std::vector<MP*>& in2 = held[cand_kf[c]];
      matches_out[c].assign((size_t)n1, static_cast<MP*>(nullptr));   // (:482-483)
      for (int i = 0; i < n1; i++) { const int m = m12[(size_t)c * n1 + i]; if (m >= 0) matches_out[c][i] = in2[m]; }
    }
    data->matched_indices_1.assign(i1.begin(), i1.begin() + rows);
    data->X1c.assign(X1.begin(), X1.begin() + 3 * rows); data->X2c.assign(X2.begin(), X2.begin() + 3 * rows);
    data->max_err1.assign(e1.begin(), e1.begin() + rows); data->max_err2.assign(e2.begin(), e2.begin() + rows);
    data->map_points_1.resize(rows); data->map_points_2.resize(rows);
    for (size_t r = 0; r < rows; r++) { data->map_points_1[r] = pts[p1[r]]; data->map_points_2[r] = pts[p2[r]]; }
    return counts[1];
  }

  // LoopClosing::CorrectLoop, src/LoopClosing.cc:437-523, in ONE library call (orbl_correct_loop) followed by the UpdateConnections
  // drop-in: `FrameOpsHip::CorrectLoopPoses(current_keyframe_, current_connected_keyframes_, sophus_sim3_Scw_, sophus_corrected_sim3,
  // sophus_non_corrected_sim3);` under the mutex_map_update_ the caller holds, as the reference does.  Only the group's slots and the
  // observers of their points are flattened; conn_rank = the group's order under std::less<KF*>, the iteration order of
  // sophus_corrected_sim3.  Written back: both Sim3 maps, and on the moved points SetWorldPos, corrected_by_keyframe_,
  // corrected_reference_, normal_vector_ / min_distance_ / max_distance_ (under mutex_pose_ when the type has it: the friend declaration
  // of INTEGRATION.md section 4), then SetPose on the group, then UpdateConnections() of the group in map order (:522 - it reads nothing
  // the correction writes).  The scale-factor table is the current keyframe's (every keyframe copies the one extractor's).  Sim3T is
  // Sophus::Sim3d or anything whose data() is its storage.  Returns the number of points moved.
  // (A member template over the keyframe type: data models without these members stay instantiable.)
  template <class KF, class Sim3T>
  static int CorrectLoopPoses(KF* current_keyframe, const std::vector<KF*>& current_connected_keyframes, const Sim3T& Scw, std::map<KF*, Sim3T>& corrected_sim3,
                              std::map<KF*, Sim3T>& non_corrected_sim3, int th = 15) {
    typedef typename std::remove_pointer<typename std::decay<decltype(current_keyframe->GetMapPointMatches()[0])>::type>::type MP;
    typedef typename std::decay<decltype(current_keyframe->GetPose())>::type M4;
    const int nconn = (int)current_connected_keyframes.size();
    if (nconn == 0 || current_connected_keyframes.back() != current_keyframe)
      throw std::runtime_error("FrameOpsT::CorrectLoopPoses: the current keyframe must be the last entry of current_connected_keyframes");
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*> kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    std::vector<int32_t> conn_kf(nconn), conn_rank(nconn), by_pointer(nconn);
    for (int c = 0; c < nconn; c++) {
      if (kf_at.count(current_connected_keyframes[c])) throw std::runtime_error("FrameOpsT::CorrectLoopPoses: a keyframe is listed twice");
      conn_kf[c] = kf_index(current_connected_keyframes[c]);          // (the group is numbered first: index = list position)
      by_pointer[c] = c;
    }
    std::sort(by_pointer.begin(), by_pointer.end(), [&](int a, int b) { return std::less<KF*>()(kfs[a], kfs[b]); });
    for (int r = 0; r < nconn; r++) conn_rank[by_pointer[r]] = r;
    std::unordered_map<MP*, int> pt_at;
    std::vector<MP*> pts;
    std::vector<int32_t> slot_off(1, 0), slot_pt, obs_off(1, 0), obs_kf, ref_kf, ref_level;
    std::vector<uint8_t> pt_bad, pt_done;
    std::vector<double> X;
    for (int c = 0; c < nconn; c++) {
      const std::vector<MP*> matches = current_connected_keyframes[c]->GetMapPointMatches();      // (:482)
      for (MP* mp : matches) {
        if (!mp) { slot_pt.push_back(-1); continue; }
        auto it = pt_at.find(mp);
        if (it == pt_at.end()) {
          it = pt_at.emplace(mp, (int)pts.size()).first;
          pts.push_back(mp);
          const bool bad = mp->isBad();
          pt_bad.push_back(bad ? 1 : 0);
          pt_done.push_back(mp->corrected_by_keyframe_ == current_keyframe->id_ ? 1 : 0);         // (:491)
          const Vector3d P = mp->GetWorldPos();
          for (int k = 0; k < 3; k++) X.push_back(P[k]);
          int ref = 0, level = 0;
          if (!bad) {                                                 // (what UpdateNormalAndDepth snapshots, src/MapPoint.cc:339-371)
            const auto observations = mp->GetObservations();
            KF* rk = mp->GetReferenceKeyFrame();
            size_t kp = 0;
            for (const auto& o : observations) { obs_kf.push_back(kf_index(o.first)); if (o.first == rk) kp = o.second; }
            if (!observations.empty()) {
              if (!rk) throw std::runtime_error("FrameOpsT::CorrectLoopPoses: a map point with observations has no reference keyframe");
              ref = kf_index(rk); level = rk->undistort_keypoints_[kp].octave;
            }
          }
          obs_off.push_back((int32_t)obs_kf.size()); ref_kf.push_back(ref); ref_level.push_back(level);
        }
        slot_pt.push_back(it->second);
      }
      slot_off.push_back((int32_t)slot_pt.size());
    }
    const int nkf = (int)kfs.size(), npts = (int)pts.size();
    std::vector<double> Tcw(12 * (size_t)nkf), center(3 * (size_t)nkf);
    for (int k = 0; k < nkf; k++) {
      const M4 T = kfs[k]->GetPose();
      const Vector3d O = kfs[k]->GetCameraCenter();
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 4; c++) Tcw[12 * (size_t)k + 4 * r + c] = T(r, c); center[3 * (size_t)k + r] = O[r]; }
    }
    const std::vector<float> table(current_keyframe->scale_factors_.begin(), current_keyframe->scale_factors_.begin() + current_keyframe->n_scale_levels_);
    std::vector<double> corrected(7 * (size_t)nconn), non_corrected(7 * (size_t)nconn), normal(3 * (size_t)std::max(npts, 1));
    std::vector<float> mm(2 * (size_t)std::max(npts, 1));
    std::vector<int32_t> owner(std::max(npts, 1), -1);
    std::vector<uint8_t> wrote(std::max(npts, 1), 0);
    if (obs_kf.empty()) obs_kf.push_back(0);
    if (slot_pt.empty()) slot_pt.push_back(-1);
    X.resize(std::max<size_t>(X.size(), 3)); pt_bad.resize(std::max(npts, 1)); pt_done.resize(std::max(npts, 1)); ref_kf.resize(std::max(npts, 1)); ref_level.resize(std::max(npts, 1));
    int32_t counts[2] = {0, 0};
    dropin::check(orbl_correct_loop(nkf, Tcw.data(), center.data(), nconn, conn_kf.data(), conn_rank.data(), Scw.data(), slot_off.data(), slot_pt.data(), npts, X.data(),
                                    pt_bad.data(), pt_done.data(), obs_off.data(), obs_kf.data(), ref_kf.data(), ref_level.data(), table.data(), (int)table.size(),
                                    corrected.data(), non_corrected.data(), owner.data(), normal.data(), mm.data(), wrote.data(), counts),
                  "orbl_correct_loop");
    for (int c = 0; c < nconn; c++) {                                 // (:438, :461, :468)
      Sim3T Sc = Scw, Sn = Scw;
      for (int k = 0; k < 7; k++) { Sc.data()[k] = corrected[7 * (size_t)c + k]; Sn.data()[k] = non_corrected[7 * (size_t)c + k]; }
      corrected_sim3[current_connected_keyframes[c]] = Sc; non_corrected_sim3[current_connected_keyframes[c]] = Sn;
    }
    for (int p = 0; p < npts; p++) {                                  // (:500-503)
      if (owner[p] < 0) continue;
      MP* mp = pts[p];
      Vector3d P, v;
      for (int k = 0; k < 3; k++) { P[k] = X[3 * (size_t)p + k]; v[k] = normal[3 * (size_t)p + k]; }
      mp->SetWorldPos(P);
      mp->corrected_by_keyframe_ = current_keyframe->id_;
      mp->corrected_reference_ = kfs[owner[p]]->id_;
      if (wrote[p]) {
        std::unique_lock<std::mutex> lock = lock_pose(mp, 0);
        mp->max_distance_ = mm[2 * (size_t)p + 1]; mp->min_distance_ = mm[2 * (size_t)p]; mp->normal_vector_ = v;
      }
    }
    std::vector<KF*> in_map_order(nconn);
    for (int r = 0; r < nconn; r++) {                                 // (:519, :522)
      const int k = conn_kf[by_pointer[r]];
      M4 T = kfs[k]->GetPose();
      for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T(i, j) = Tcw[12 * (size_t)k + 4 * i + j];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      kfs[k]->SetPose(T);
      in_map_order[r] = kfs[k];
    }
    UpdateConnections(in_map_order, (std::map<KF*, std::set<KF*> >*)nullptr, th);
    return counts[0];
  }

  // The write-back of LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:681-739, in ONE library call (orbl_propagate_global_ba):
  // `FrameOpsHip::PropagateGlobalBA(map_, nLoopKF);` under mutex_map_update_, before map_->InformNewBigChange().  The tree is read
  // through GetChilds() from keyframe_origins_ and from every keyframe of the map (kf_parent[c] = p iff c is in p->GetChilds()).
  // Written back: global_BA_Tcw_ and n_BA_global_for_keyframe_ of the keyframes the walk carried the correction to, global_BA_Bef_Tcw_
  // and SetPose of every keyframe it reached, SetWorldPos of every point it moved.  The one departure include/orbslam_hip.h states: the
  // points of a flagged keyframe the walk does not reach stay put.  Returns the number of points moved.
  template <class MapT> static int PropagateGlobalBA(MapT* map, unsigned long nLoopKF) {
    typedef typename std::remove_pointer<typename std::decay<decltype(map->GetAllKeyFrames()[0])>::type>::type KF;
    typedef typename std::remove_pointer<typename std::decay<decltype(map->GetAllMapPoints()[0])>::type>::type MP;
    typedef typename std::decay<decltype(map->GetAllKeyFrames()[0]->GetPose())>::type M4;
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*> kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    std::vector<int32_t> origin_kf;
    for (KF* kf : map->keyframe_origins_) origin_kf.push_back(kf_index(kf));
    for (KF* kf : map->GetAllKeyFrames()) kf_index(kf);
    const std::vector<MP*> points = map->GetAllMapPoints();
    const int npts = (int)points.size();
    std::vector<int32_t> pt_ref(std::max(npts, 1), 0);
    std::vector<uint8_t> pt_bad(std::max(npts, 1), 0), pt_in(std::max(npts, 1), 0), moved(std::max(npts, 1), 0);
    std::vector<double> X(3 * (size_t)std::max(npts, 1), 0.0), GX(3 * (size_t)std::max(npts, 1), 0.0);
    for (int p = 0; p < npts; p++) {
      MP* mp = points[p];
      pt_bad[p] = mp->isBad() ? 1 : 0;
      if (pt_bad[p]) continue;
      pt_in[p] = mp->n_BA_global_for_keyframe_ == nLoopKF ? 1 : 0;
      const Vector3d P = mp->GetWorldPos();
      for (int k = 0; k < 3; k++) { X[3 * (size_t)p + k] = P[k]; GX[3 * (size_t)p + k] = mp->global_BA_pose_[k]; }
      if (pt_in[p]) continue;
      KF* rk = mp->GetReferenceKeyFrame();
      if (!rk) throw std::runtime_error("FrameOpsT::PropagateGlobalBA: a map point without a reference keyframe");
      pt_ref[p] = kf_index(rk);
    }
    std::vector<int32_t> parent;
    for (size_t k = 0; k < kfs.size(); k++) {                          // (kfs grows while children that the map does not list turn up)
      const auto childs = kfs[k]->GetChilds();
      for (KF* c : childs) { const int ci = kf_index(c); if ((size_t)ci >= parent.size()) parent.resize(ci + 1, -1); parent[ci] = (int32_t)k; }
    }
    const int nkf = (int)kfs.size();
    parent.resize(nkf, -1);
    std::vector<double> Tcw(12 * (size_t)nkf), gba(12 * (size_t)nkf), bef(12 * (size_t)nkf);
    std::vector<uint8_t> in_gba(nkf), reached(nkf, 0), in_before;
    for (int k = 0; k < nkf; k++) {
      const M4 T = kfs[k]->GetPose();
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { Tcw[12 * (size_t)k + 4 * r + c] = T(r, c); gba[12 * (size_t)k + 4 * r + c] = kfs[k]->global_BA_Tcw_(r, c); }
      in_gba[k] = kfs[k]->n_BA_global_for_keyframe_ == nLoopKF ? 1 : 0;
    }
    in_before = in_gba;
    int32_t counts[4] = {0, 0, 0, 0};
    dropin::check(orbl_propagate_global_ba(nkf, Tcw.data(), gba.data(), in_gba.data(), parent.data(), (int)origin_kf.size(), origin_kf.data(), nullptr, npts, X.data(),
                                           pt_bad.data(), pt_in.data(), GX.data(), pt_ref.data(), bef.data(), reached.data(), moved.data(), counts),
                  "orbl_propagate_global_ba");
    auto to_m4 = [](const M4& like, const double* t) {
      M4 T = like;
      for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T(i, j) = t[4 * i + j];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      return T;
    };
    for (int k = 0; k < nkf; k++) {                                   // (:693-695, :700-701)
      if (!reached[k]) continue;
      KF* kf = kfs[k];
      const M4 like = kf->GetPose();
      if (!in_before[k]) { kf->global_BA_Tcw_ = to_m4(like, gba.data() + 12 * (size_t)k); kf->n_BA_global_for_keyframe_ = nLoopKF; }
      kf->global_BA_Bef_Tcw_ = to_m4(like, bef.data() + 12 * (size_t)k);
      kf->SetPose(to_m4(like, Tcw.data() + 12 * (size_t)k));
    }
    for (int p = 0; p < npts; p++) {                                  // (:715, :737)
      if (!moved[p]) continue;
      Vector3d P;
      for (int k = 0; k < 3; k++) P[k] = X[3 * (size_t)p + k];
      points[p]->SetWorldPos(P);
    }
    return counts[2];
  }

  // CeresOptimizer::LocalBundleAdjustment, src/CeresOptimizer.cc:344-599, with BOTH halves around the optimisation in the library
  // (orbl_local_ba_assemble, orbl_local_ba_apply): `FrameOpsHip::LocalBundleAdjustment(current_keyframe_, &is_abort_BA_, map_);` at
  // src/LocalMapping.cc:89.  AssembleLocalBA flattens the current keyframe, its covisible keyframes, the points in their slots and the
  // observers of those points (kf_rank / pt_rank = their orders under std::less), and keeps the tables beside the assembled problem;
  // ApplyLocalBA runs the write-back on those tables and carries the changes into the objects: EraseMapPointMatch on every emptied slot,
  // the observations, Observations(), the reference keyframe and the bad flag of every point that lost an observation (under
  // mutex_features_ when the type has it; map_->EraseMapPoint of a point that turned bad stays with the caller), SetPose, SetWorldPos,
  // normal_vector_ / min_distance_ / max_distance_.  Both return -1, with the map untouched, when the flattened part of the map is not
  // consistent: keyframe k holds p in slot i iff p's observations contain (k, i).
  template <class KF, class MP> struct LocalBAProblemT {
    std::vector<KF*> kfs; std::vector<MP*> pts; KF* current = nullptr;
    std::vector<double> kf_Tcw, kf_center, X; std::vector<int32_t> slot_off, slot_pt, pt_nobs, pt_ref, obs_off, obs_kf, obs_slot, obs_level, kf_level0;
    std::vector<uint8_t> pt_bad; std::vector<float> scale_factors;
    int32_t counts[4] = {0, 0, 0, 0};                                // {ncam, n_local_cam, npts_local, nobs_local}
    std::vector<int32_t> cam_kf, lpt_pt, lobs_cam, lobs_pt, lobs_src; std::vector<double> K4, poses7, pts3, lobs_uv; std::vector<float> lobs_inv_sigma2;
    std::vector<uint8_t> cam_fixed, cam_local, kf_role, pt_local;
  };

  template <class KF, class MP> static int AssembleLocalBA(KF* keyframe, LocalBAProblemT<KF, MP>* P) {
    typedef typename std::decay<decltype(keyframe->GetPose())>::type M4;
    *P = LocalBAProblemT<KF, MP>();
    P->current = keyframe;
    std::unordered_map<KF*, int> kf_at;
    std::vector<KF*>& kfs = P->kfs;
    auto kf_index = [&](KF* kf) {
      auto it = kf_at.find(kf);
      if (it == kf_at.end()) { it = kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    kf_index(keyframe);
    const std::vector<KF*> neighbor_keyframes = keyframe->GetVectorCovisibleKeyFrames();
    std::vector<int32_t> nbr_kf;
    for (KF* nb : neighbor_keyframes) nbr_kf.push_back(kf_index(nb));
    const int n_stamped = (int)kfs.size();
    std::unordered_map<MP*, int> pt_at;
    std::vector<MP*>& pts = P->pts;
    std::vector<float> obs_uv;
    for (int k = 0; k < n_stamped; k++) {                             // the points in the slots of the local keyframes (":366-384")
      if (k > 0 && kfs[k]->isBad()) continue;
      const std::vector<MP*> matches = kfs[k]->GetMapPointMatches();
      for (MP* mp : matches) {
        if (!mp || pt_at.count(mp)) continue;
        pt_at.emplace(mp, (int)pts.size()); pts.push_back(mp);
        const bool bad = mp->isBad();
        P->pt_bad.push_back(bad ? 1 : 0);
        const Vector3d X = mp->GetWorldPos();
        for (int c = 0; c < 3; c++) P->X.push_back(X[c]);
        if (!bad) {
          const auto observations = mp->GetObservations();
          for (const auto& o : observations) {
            const auto& kp = o.first->undistort_keypoints_[o.second];
            P->obs_kf.push_back(kf_index(o.first)); P->obs_slot.push_back((int32_t)o.second); P->obs_level.push_back(kp.octave);
            obs_uv.push_back(kp.pt.x); obs_uv.push_back(kp.pt.y);
          }
        }
        P->obs_off.push_back((int32_t)P->obs_kf.size());
        P->pt_nobs.push_back(mp->Observations());
        KF* rk = mp->GetReferenceKeyFrame();
        P->pt_ref.push_back(rk ? kf_index(rk) : -1);              // (-1: no reference keyframe; it is compared and never dereferenced)
      }
    }
    P->obs_off.insert(P->obs_off.begin(), 0);
    const int nkf = (int)kfs.size(), npts = (int)pts.size(), nobs = (int)P->obs_kf.size();
    std::vector<int32_t> kf_id(nkf), kf_rank(nkf), pt_rank(std::max(npts, 1)), by(nkf);
    std::vector<uint8_t> kf_bad(nkf);
    std::vector<double> kf_K4(4 * (size_t)nkf);
    P->kf_Tcw.resize(12 * (size_t)nkf); P->kf_center.resize(3 * (size_t)nkf); P->kf_level0.resize(nkf); P->slot_off.assign(1, 0);
    for (int k = 0; k < nkf; k++) {
      KF* kf = kfs[k];
      const M4 T = kf->GetPose();
      const Vector3d O = kf->GetCameraCenter();
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 4; c++) P->kf_Tcw[12 * (size_t)k + 4 * r + c] = T(r, c); P->kf_center[3 * (size_t)k + r] = O[r]; }
      kf_id[k] = (int32_t)kf->id_; kf_bad[k] = kf->isBad() ? 1 : 0;
      kf_K4[4 * (size_t)k] = kf->fx_; kf_K4[4 * (size_t)k + 1] = kf->fy_; kf_K4[4 * (size_t)k + 2] = kf->cx_; kf_K4[4 * (size_t)k + 3] = kf->cy_;
      P->kf_level0[k] = kf->undistort_keypoints_.empty() ? 0 : kf->undistort_keypoints_[0].octave;
      const std::vector<MP*> matches = kf->GetMapPointMatches();      // a point the flattening does not know is an empty slot: nothing writes it
      for (MP* mp : matches) { auto it = mp ? pt_at.find(mp) : pt_at.end(); P->slot_pt.push_back(it == pt_at.end() ? -1 : it->second); }
      P->slot_off.push_back((int32_t)P->slot_pt.size());
      by[k] = k;
    }
    // consistency of what was flattened: every observation's slot holds its point, every slot's point lists that slot.  A BAD point in
    // a slot is exempt: between `is_bad_ = true` and the EraseMapPointMatch loop of SetBadFlag (src/MapPoint.cc:179-188) it sits there with
    // its observations cleared, and the reference, which collects without mutex_map_update_, skips it (":376") and runs.
    for (int p = 0; p < npts; p++)
      for (int e = P->obs_off[p]; e < P->obs_off[p + 1]; e++) {
        const int k = P->obs_kf[e], s = P->obs_slot[e];
        if (s < 0 || s >= P->slot_off[k + 1] - P->slot_off[k] || P->slot_pt[P->slot_off[k] + s] != p) return -1;
      }
    for (int k = 0; k < nkf; k++)
      for (int s = P->slot_off[k]; s < P->slot_off[k + 1]; s++) {
        const int p = P->slot_pt[s];
        if (p < 0 || P->pt_bad[p]) continue;
        bool listed = false;
        for (int e = P->obs_off[p]; e < P->obs_off[p + 1] && !listed; e++) listed = P->obs_kf[e] == k && P->obs_slot[e] == s - P->slot_off[k];
        if (!listed) return -1;
      }
    std::sort(by.begin(), by.end(), [&](int a, int b) { return std::less<KF*>()(kfs[a], kfs[b]); });
    for (int r = 0; r < nkf; r++) kf_rank[by[r]] = r;
    std::vector<int32_t> byp(npts);
    for (int p = 0; p < npts; p++) byp[p] = p;
    std::sort(byp.begin(), byp.end(), [&](int a, int b) { return std::less<MP*>()(pts[a], pts[b]); });
    for (int r = 0; r < npts; r++) pt_rank[byp[r]] = r;
    const int n_levels = keyframe->n_scale_levels_;
    const std::vector<float> isg(keyframe->inv_level_sigma2s_.begin(), keyframe->inv_level_sigma2s_.begin() + n_levels);
    P->scale_factors.assign(keyframe->scale_factors_.begin(), keyframe->scale_factors_.begin() + n_levels);
    const size_t cc = (size_t)nkf, cp = (size_t)std::max(npts, 1), co = (size_t)std::max(nobs, 1);
    P->cam_kf.resize(cc); P->K4.resize(4 * cc); P->poses7.resize(7 * cc); P->cam_fixed.resize(cc); P->cam_local.resize(cc); P->lpt_pt.resize(cp); P->pts3.resize(3 * cp);
    P->lobs_cam.resize(co); P->lobs_pt.resize(co); P->lobs_uv.resize(2 * co); P->lobs_inv_sigma2.resize(co); P->lobs_src.resize(co); P->kf_role.resize(cc); P->pt_local.resize(cp);
    P->X.resize(3 * cp); P->pt_bad.resize(cp); P->pt_nobs.resize(cp); P->pt_ref.resize(cp);
    P->obs_kf.resize(co); P->obs_slot.resize(co); P->obs_level.resize(co); obs_uv.resize(2 * co);
    if (P->slot_pt.empty()) P->slot_pt.push_back(-1);
    if (nbr_kf.empty()) nbr_kf.push_back(0);
    dropin::check(orbl_local_ba_assemble(0, (int)neighbor_keyframes.size(), nbr_kf.data(), nkf, kf_id.data(), kf_bad.data(), kf_rank.data(), P->kf_Tcw.data(), kf_K4.data(),
                                         P->slot_off.data(), P->slot_pt.data(), npts, P->X.data(), P->pt_bad.data(), pt_rank.data(), P->obs_off.data(), P->obs_kf.data(),
                                         obs_uv.data(), P->obs_level.data(), isg.data(), n_levels, nkf, npts, nobs, P->counts, P->cam_kf.data(), P->K4.data(),
                                         P->poses7.data(), P->cam_fixed.data(), P->cam_local.data(), P->lpt_pt.data(), P->pts3.data(), P->lobs_cam.data(), P->lobs_pt.data(),
                                         P->lobs_uv.data(), P->lobs_inv_sigma2.data(), P->lobs_src.data(), P->kf_role.data(), P->pt_local.data()),
                  "orbl_local_ba_assemble");
    const size_t ncam = (size_t)P->counts[0], npl = (size_t)P->counts[2], nol = (size_t)P->counts[3];
    P->cam_kf.resize(ncam); P->K4.resize(4 * ncam); P->poses7.resize(7 * ncam); P->cam_fixed.resize(ncam); P->cam_local.resize(ncam); P->lpt_pt.resize(npl); P->pts3.resize(3 * npl);
    P->lobs_cam.resize(nol); P->lobs_pt.resize(nol); P->lobs_uv.resize(2 * nol); P->lobs_inv_sigma2.resize(nol); P->lobs_src.resize(nol);
    // the reference's stamps (":351", ":358", ":379", ":399")
    for (int k = 0; k < nkf; k++) if (P->kf_role[k] == 1 || P->kf_role[k] == 3) kfs[k]->n_BA_local_for_keyframe_ = keyframe->id_;
    for (size_t j = 0; j < npl; j++) {
      const int p = P->lpt_pt[j];
      pts[p]->n_BA_local_for_keyframe_ = keyframe->id_;
      for (int e = P->obs_off[p]; e < P->obs_off[p + 1]; e++) { const int r = P->kf_role[P->obs_kf[e]]; if (r == 0 || r == 2) kfs[P->obs_kf[e]]->n_BA_fixed_for_keyframe_ = keyframe->id_; }
    }
    return (int)nol;
  }

  // poses7[ncam][7], pts3[npts_local][3], obs_erase[nobs_local]: what ba_local_bundle_adjustment left.  Returns the number of observations erased.
  // turned_bad (optional): the points this call turned bad, for the caller's map_->EraseMapPoint.
  template <class KF, class MP> static int ApplyLocalBA(LocalBAProblemT<KF, MP>* P, const double* poses7, const double* pts3, const uint8_t* obs_erase,
                                                        std::vector<MP*>* turned_bad = nullptr) {
    typedef typename std::decay<decltype(P->current->GetPose())>::type M4;
    const int nkf = (int)P->kfs.size(), npts = (int)P->pts.size(), nobs = P->obs_off.back();
    const int ncam = P->counts[0], npl = P->counts[2], nol = P->counts[3];
    std::vector<int32_t> slots = P->slot_pt, nobs_after = P->pt_nobs, ref = P->pt_ref;
    std::vector<uint8_t> bad = P->pt_bad, erased((size_t)std::max(nobs, 1), 0), wrote((size_t)std::max(npts, 1), 0);
    std::vector<double> Tcw = P->kf_Tcw, center = P->kf_center, X = P->X, normal(3 * (size_t)std::max(npts, 1));
    std::vector<float> mm(2 * (size_t)std::max(npts, 1));
    const uint8_t none = 0;
    int32_t counts[4] = {0, 0, 0, 0};
    dropin::check(orbl_local_ba_apply(ncam, P->cam_kf.data(), P->cam_local.data(), poses7, npl, P->lpt_pt.data(), pts3, nol, P->lobs_src.data(), nol ? obs_erase : &none, nkf,
                                      Tcw.data(), center.data(), P->slot_off.data(), slots.data(), npts, X.data(), bad.data(), nobs_after.data(), ref.data(), P->obs_off.data(),
                                      P->obs_kf.data(), P->obs_slot.data(), P->obs_level.data(), P->kf_level0.data(), P->scale_factors.data(), (int)P->scale_factors.size(),
                                      erased.data(), normal.data(), mm.data(), wrote.data(), counts),
                  "orbl_local_ba_apply");
    for (int k = 0; k < nkf; k++)                                     // (":578", src/MapPoint.cc:187)
      for (int s = P->slot_off[k]; s < P->slot_off[k + 1]; s++)
        if (slots[s] < 0 && P->slot_pt[s] >= 0) { const size_t index = (size_t)(s - P->slot_off[k]); P->kfs[k]->EraseMapPointMatch(index); }
    for (int p = 0; p < npts; p++) {                                  // (":579", src/MapPoint.cc:140-188)
      bool lost = false;
      for (int e = P->obs_off[p]; e < P->obs_off[p + 1]; e++) lost = lost || erased[e];
      if (!lost) continue;
      MP* mp = P->pts[p];
      std::unique_lock<std::mutex> lock = lock_features(mp, 0);
      for (int e = P->obs_off[p]; e < P->obs_off[p + 1]; e++) if (erased[e]) mp->observations_.erase(P->kfs[P->obs_kf[e]]);
      mp->n_observations_ = nobs_after[p];
      if (ref[p] >= 0 && ref[p] != P->pt_ref[p]) mp->reference_keyframe_ = P->kfs[ref[p]];
      if (bad[p] && !P->pt_bad[p]) { mp->is_bad_ = true; if (turned_bad) turned_bad->push_back(mp); }
    }
    for (int c = 0; c < ncam; c++) {                                  // (":585-591")
      if (!P->cam_local[c]) continue;
      const int k = P->cam_kf[c];
      M4 T = P->kfs[k]->GetPose();
      for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T(i, j) = Tcw[12 * (size_t)k + 4 * i + j];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      P->kfs[k]->SetPose(T);
    }
    for (int j = 0; j < npl; j++) {                                   // (":593-598")
      const int p = P->lpt_pt[j];
      MP* mp = P->pts[p];
      Vector3d Q, v;
      for (int c = 0; c < 3; c++) { Q[c] = X[3 * (size_t)p + c]; v[c] = normal[3 * (size_t)p + c]; }
      mp->SetWorldPos(Q);
      if (wrote[p]) {
        std::unique_lock<std::mutex> lock = lock_pose(mp, 0);
        mp->max_distance_ = mm[2 * (size_t)p + 1]; mp->min_distance_ = mm[2 * (size_t)p]; mp->normal_vector_ = v;
      }
    }
    return counts[0];
  }

  // 0 when the map was optimised or the stop flag ended the call first (":509-512": the reference returns without writing back), -1 when
  // the map is not consistent (it is left untouched).  turned_bad (optional): the points the write-back turned bad - SetBadFlag's
  // map_->EraseMapPoint(this) (src/MapPoint.cc:190) is the caller's: `for (MapPoint* mp : turned_bad) map_->EraseMapPoint(mp);`
  template <class KF, class MapT, class MP = typename std::remove_pointer<typename std::decay<decltype(std::declval<KF*>()->GetMapPointMatches()[0])>::type>::type>
  static int LocalBundleAdjustment(KF* keyframe, bool* stop_flag, MapT* map, std::vector<MP*>* turned_bad = nullptr) {
    LocalBAProblemT<KF, MP> P;
    if (AssembleLocalBA(keyframe, &P) < 0) return -1;
    if (stop_flag && *stop_flag) return 0;
    std::vector<uint8_t> erase(P.lobs_cam.size() ? P.lobs_cam.size() : 1, 0);
    std::vector<double> poses7 = P.poses7, pts3 = P.pts3;
    if (pts3.empty()) pts3.resize(3);
    int aborted = 0;
    dropin::check(ba_local_bundle_adjustment(P.K4.data(), poses7.data(), P.cam_fixed.data(), P.cam_local.data(), P.counts[0], pts3.data(), P.counts[2], P.lobs_cam.data(),
                                             P.lobs_pt.data(), P.lobs_uv.data(), P.lobs_inv_sigma2.data(), P.counts[3], reinterpret_cast<const volatile uint8_t*>(stop_flag),
                                             1, erase.data(), &aborted, nullptr, nullptr),
                  "ba_local_bundle_adjustment");
    if (aborted) return 0;
    std::unique_lock<std::mutex> lock(map->mutex_map_update_);        // (":573")
    ApplyLocalBA(&P, poses7.data(), pts3.data(), erase.data(), turned_bad);
    return 0;
  }

  // CeresOptimizer::OptimizeEssentialGraph, src/CeresOptimizer.cc:737-957, with BOTH halves around the optimisation in the library
  // (orbl_essential_graph_assemble, orbl_essential_graph_apply): `FrameOpsHip::OptimizeEssentialGraph(map_, matched_keyframe_,
  // current_keyframe_, sophus_non_corrected_sim3, sophus_corrected_sim3, loop_connections);` at src/LoopClosing.cc:573.
  // AssembleEssentialGraph flattens GetAllKeyFrames() - isBad(), id_, GetPose(), GetParent(), GetChilds(), GetLoopEdges(), and under
  // mutex_connections_ connected_keyframe_weights_ with the two ordered lists (the friend declaration of INTEGRATION.md section 4) - the
  // two Sim3 maps and loop_connections; kf_rank is the pointer order.  A keyframe the map does not list (a parent, a child, a link) is
  // left out, as a keyframe without a parameter block is in CeresOptimizerT::OptimizeEssentialGraph.  ApplyEssentialGraph flattens
  // GetAllMapPoints() - isBad(), corrected_by_keyframe_, corrected_reference_, GetReferenceKeyFrame(), GetObservations(), the reference
  // level - runs the write-back on the tables and carries SetPose, SetWorldPos and normal_vector_ / min_distance_ / max_distance_ into
  // the objects; the caller holds map->mutex_map_update_ (":914"), as OptimizeEssentialGraph below does.  kf_id must be distinct among
  // the keyframes that are not bad (the library refuses a map where it is not).
  template <class KF> struct EssentialGraphProblemT {
    std::vector<KF*> kfs; KF* current = nullptr;
    int32_t counts[4] = {0, 0, 0, 0};                                // {n_vtx, n_edges, n_loop_connection_edges, n_dropped}
    std::vector<int32_t> vtx_kf, kf_vtx, edge_j, edge_i; std::vector<double> lie7, edge_Sji; std::vector<uint8_t> vtx_fixed, edge_kind;
  };

  template <class MapT, class KF, class Sim3T>
  static int AssembleEssentialGraph(MapT* map, KF* loop_keyframe, KF* current_keyframe, const std::map<KF*, Sim3T>& non_corrected_sim3,
                                    const std::map<KF*, Sim3T>& corrected_sim3, const std::map<KF*, std::set<KF*> >& loop_connections,
                                    EssentialGraphProblemT<KF>* P, int min_weight = 100) {
    typedef typename std::decay<decltype(current_keyframe->GetPose())>::type M4;
    *P = EssentialGraphProblemT<KF>();
    P->current = current_keyframe;
    P->kfs = map->GetAllKeyFrames();
    const std::vector<KF*>& kfs = P->kfs;
    const int nkf = (int)kfs.size();
    if (nkf == 0) return 0;
    std::unordered_map<KF*, int> kf_at;
    for (int k = 0; k < nkf; k++) kf_at.emplace(kfs[k], k);
    auto index_of = [&](KF* kf) { auto it = kf ? kf_at.find(kf) : kf_at.end(); return it == kf_at.end() ? -1 : it->second; };
    const int loop_index = index_of(loop_keyframe), cur_index = index_of(current_keyframe);
    if (loop_index < 0 || cur_index < 0) throw std::runtime_error("FrameOpsT::AssembleEssentialGraph: the loop or the current keyframe is not in the map");
    std::vector<int32_t> kf_id(nkf), kf_rank(nkf), kf_parent(nkf), by(nkf), child_off(1, 0), child_kf, loop_off(1, 0), loop_kf, conn_off(1, 0), conn_kf, conn_w, ord_off(1, 0), ord_kf,
        ord_w;
    std::vector<uint8_t> kf_bad(nkf);
    std::vector<double> Tcw(12 * (size_t)nkf);
    for (int k = 0; k < nkf; k++) {
      KF* kf = kfs[k];
      const M4 T = kf->GetPose();
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) Tcw[12 * (size_t)k + 4 * r + c] = T(r, c);
      kf_id[k] = (int32_t)kf->id_; kf_bad[k] = kf->isBad() ? 1 : 0; kf_parent[k] = index_of(kf->GetParent()); by[k] = k;
      const auto childs = kf->GetChilds();
      for (KF* c : childs) { const int ci = index_of(c); if (ci >= 0) child_kf.push_back(ci); }
      child_off.push_back((int32_t)child_kf.size());
      const auto loop_edges = kf->GetLoopEdges();
      for (KF* l : loop_edges) { const int li = index_of(l); if (li >= 0) loop_kf.push_back(li); }
      loop_off.push_back((int32_t)loop_kf.size());
      {
        std::unique_lock<std::mutex> lock = lock_connections(kf, 0);
        for (const auto& w : kf->connected_keyframe_weights_) { const int wi = index_of(w.first); if (wi >= 0) { conn_kf.push_back(wi); conn_w.push_back((int32_t)w.second); } }
        auto wt = kf->ordered_weights_.begin();
        for (auto it = kf->ordered_connected_keyframes_.begin(); it != kf->ordered_connected_keyframes_.end(); ++it, ++wt) {
          ord_kf.push_back(index_of(*it)); ord_w.push_back((int32_t)*wt);                   // (-1 must not leave the list: the prefix rule reads every weight)
        }
      }
      conn_off.push_back((int32_t)conn_kf.size()); ord_off.push_back((int32_t)ord_kf.size());
    }
    // an ordered entry the map does not list is a keyframe without a parameter block: the library has no such index, so it is given the
    // index of a bad keyframe's stand-in - the entry's own keyframe, which no rule admits (a keyframe is never its own covisible)
    for (int k = 0; k < nkf; k++) for (int e = ord_off[k]; e < ord_off[k + 1]; e++) if (ord_kf[e] < 0) ord_kf[e] = k;
    std::sort(by.begin(), by.end(), [&](int a, int b) { return std::less<KF*>()(kfs[a], kfs[b]); });
    for (int r = 0; r < nkf; r++) kf_rank[by[r]] = r;
    std::vector<int32_t> group_kf, tgt_kf, link_off(1, 0), link_kf;
    std::vector<double> corrected, non_corrected;
    for (const auto& c : corrected_sim3) {
      const int k = index_of(c.first);
      auto n = non_corrected_sim3.find(c.first);
      if (k < 0) continue;
      if (n == non_corrected_sim3.end()) throw std::runtime_error("FrameOpsT::AssembleEssentialGraph: the two Sim3 maps name different keyframes");
      group_kf.push_back(k);
      for (int q = 0; q < 7; q++) { corrected.push_back(c.second.data()[q]); non_corrected.push_back(n->second.data()[q]); }
    }
    for (const auto& t : loop_connections) {
      const int k = index_of(t.first);
      if (k < 0) continue;
      tgt_kf.push_back(k);
      for (KF* l : t.second) { const int li = index_of(l); if (li >= 0) link_kf.push_back(li); }
      link_off.push_back((int32_t)link_kf.size());
    }
    const int nconn = (int)group_kf.size(), ntgt = (int)tgt_kf.size();
    const size_t cv = (size_t)nkf, ce = link_kf.size() + (size_t)nkf + loop_kf.size() + ord_kf.size() + 1;
    P->vtx_kf.resize(cv); P->kf_vtx.resize(cv); P->lie7.resize(7 * cv); P->vtx_fixed.resize(cv); P->edge_j.resize(ce); P->edge_i.resize(ce); P->edge_Sji.resize(7 * ce);
    P->edge_kind.resize(ce);
    dropin::check(orbl_essential_graph_assemble(nkf, kf_id.data(), kf_bad.data(), kf_rank.data(), Tcw.data(), kf_parent.data(), child_off.data(), child_kf.data(), loop_off.data(),
                                                loop_kf.data(), conn_off.data(), conn_kf.data(), conn_w.data(), ord_off.data(), ord_kf.data(), ord_w.data(), nconn, group_kf.data(),
                                                corrected.data(), non_corrected.data(), ntgt, tgt_kf.data(), link_off.data(), link_kf.data(), loop_index, cur_index, min_weight,
                                                (int)cv, (int)ce, P->counts, P->vtx_kf.data(), P->kf_vtx.data(), P->lie7.data(), P->vtx_fixed.data(), P->edge_j.data(),
                                                P->edge_i.data(), P->edge_Sji.data(), P->edge_kind.data()),
                  "orbl_essential_graph_assemble");
    const size_t nv = (size_t)P->counts[0], ne = (size_t)P->counts[1];
    P->vtx_kf.resize(nv); P->lie7.resize(7 * nv); P->vtx_fixed.resize(nv); P->edge_j.resize(ne); P->edge_i.resize(ne); P->edge_Sji.resize(7 * ne); P->edge_kind.resize(ne);
    return (int)ne;
  }

  // lie_opt[n_vtx][7]: what ba_optimize_essential_graph left.  Returns the number of points moved.
  template <class MapT, class KF> static int ApplyEssentialGraph(MapT* map, EssentialGraphProblemT<KF>* P, const double* lie_opt) {
    typedef typename std::remove_pointer<typename std::decay<decltype(map->GetAllMapPoints()[0])>::type>::type MP;
    typedef typename std::decay<decltype(P->current->GetPose())>::type M4;
    const int nkf = (int)P->kfs.size(), n_vtx = P->counts[0];
    if (nkf == 0 || n_vtx == 0) return 0;
    std::unordered_map<KF*, int> kf_at;
    std::unordered_map<unsigned long, int> kf_by_id;                   // (corrected_reference_ is a keyframe id: the non-bad keyframe that holds it)
    for (int k = 0; k < nkf; k++) { kf_at.emplace(P->kfs[k], k); if (P->kf_vtx[k] >= 0) kf_by_id.emplace((unsigned long)P->kfs[k]->id_, k); }
    const std::vector<MP*> points = map->GetAllMapPoints();
    const int npts = (int)points.size();
    const size_t np1 = (size_t)std::max(npts, 1);
    std::vector<int32_t> pt_ref(np1, -1), pt_corr(np1, -1), ref_level(np1, 0), obs_off(1, 0), obs_kf;
    std::vector<uint8_t> pt_bad(np1, 0), pt_done(np1, 0), moved(np1, 0), wrote(np1, 0), on_host(np1, 0);
    std::vector<double> X(3 * np1, 0.0), normal(3 * np1, 0.0);
    std::vector<float> mm(2 * np1, 0.f);
    for (int p = 0; p < npts; p++) {
      MP* mp = points[p];
      pt_bad[p] = mp->isBad() ? 1 : 0;
      if (!pt_bad[p]) {
        const Vector3d Q = mp->GetWorldPos();
        for (int c = 0; c < 3; c++) X[3 * (size_t)p + c] = Q[c];
        KF* rk = mp->GetReferenceKeyFrame();
        auto rit = rk ? kf_at.find(rk) : kf_at.end();
        pt_ref[p] = rit == kf_at.end() ? -1 : rit->second;
        if (mp->corrected_by_keyframe_ == P->current->id_) {           // (":942-943")
          pt_done[p] = 1;
          auto cit = kf_by_id.find((unsigned long)mp->corrected_reference_);
          pt_corr[p] = cit == kf_by_id.end() ? -1 : cit->second;
        }
        bool all_known = pt_ref[p] >= 0;                               // (what UpdateNormalAndDepth snapshots, src/MapPoint.cc:339-371)
        const auto observations = mp->GetObservations();
        size_t kp = 0;
        const size_t first = obs_kf.size();
        for (const auto& o : observations) { auto oit = kf_at.find(o.first); if (oit == kf_at.end()) { all_known = false; break; } obs_kf.push_back(oit->second); if (o.first == rk) kp = o.second; }
        if (!all_known) { obs_kf.resize(first); on_host[p] = 1; }      // (an observer outside the map: the object's own UpdateNormalAndDepth below)
        else if (!observations.empty()) ref_level[p] = rk->undistort_keypoints_[kp].octave;
      }
      obs_off.push_back((int32_t)obs_kf.size());
    }
    std::vector<double> Tcw(12 * (size_t)nkf), center(3 * (size_t)nkf);
    for (int k = 0; k < nkf; k++) {
      const M4 T = P->kfs[k]->GetPose();
      const Vector3d O = P->kfs[k]->GetCameraCenter();
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 4; c++) Tcw[12 * (size_t)k + 4 * r + c] = T(r, c); center[3 * (size_t)k + r] = O[r]; }
    }
    const std::vector<float> table(P->current->scale_factors_.begin(), P->current->scale_factors_.begin() + P->current->n_scale_levels_);
    if (obs_kf.empty()) obs_kf.push_back(0);
    int32_t counts[2] = {0, 0};
    dropin::check(orbl_essential_graph_apply(n_vtx, P->vtx_kf.data(), P->lie7.data(), lie_opt, nkf, Tcw.data(), center.data(), npts, X.data(), pt_bad.data(), pt_done.data(),
                                             pt_corr.data(), pt_ref.data(), obs_off.data(), obs_kf.data(), ref_level.data(), table.data(), (int)table.size(), normal.data(),
                                             mm.data(), wrote.data(), moved.data(), counts),
                  "orbl_essential_graph_apply");
    for (int v = 0; v < n_vtx; v++) {                                 // (":917-933")
      const int k = P->vtx_kf[v];
      M4 T = P->kfs[k]->GetPose();
      for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T(i, j) = Tcw[12 * (size_t)k + 4 * i + j];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      P->kfs[k]->SetPose(T);
    }
    for (int p = 0; p < npts; p++) {                                  // (":936-956")
      if (!moved[p]) continue;
      MP* mp = points[p];
      Vector3d Q, v;
      for (int c = 0; c < 3; c++) { Q[c] = X[3 * (size_t)p + c]; v[c] = normal[3 * (size_t)p + c]; }
      mp->SetWorldPos(Q);
      if (wrote[p]) {
        std::unique_lock<std::mutex> lock = lock_pose(mp, 0);
        mp->max_distance_ = mm[2 * (size_t)p + 1]; mp->min_distance_ = mm[2 * (size_t)p]; mp->normal_vector_ = v;
      } else if (on_host[p]) mp->UpdateNormalAndDepth();
    }
    return counts[1];
  }

  // Returns the number of edges of the problem.  summary (optional): the solver's.
  template <class MapT, class KF, class Sim3T>
  static int OptimizeEssentialGraph(MapT* map, KF* loop_keyframe, KF* current_keyframe, const std::map<KF*, Sim3T>& non_corrected_sim3,
                                    const std::map<KF*, Sim3T>& corrected_sim3, const std::map<KF*, std::set<KF*> >& loop_connections) {
    EssentialGraphProblemT<KF> P;
    const int n_edges = AssembleEssentialGraph(map, loop_keyframe, current_keyframe, non_corrected_sim3, corrected_sim3, loop_connections, &P);
    const int n_vtx = P.counts[0];
    if (n_vtx == 0) return 0;
    std::vector<double> lie = P.lie7;
    const int32_t idummy[1] = {0}; const double ddummy[7] = {0, 0, 0, 1, 0, 0, 0};
    dropin::check(ba_optimize_essential_graph(lie.data(), P.vtx_fixed.data(), n_vtx, n_edges ? P.edge_j.data() : idummy, n_edges ? P.edge_i.data() : idummy,
                                              n_edges ? P.edge_Sji.data() : ddummy, n_edges, 100, nullptr, nullptr),
                  "ba_optimize_essential_graph");
    std::unique_lock<std::mutex> lock(map->mutex_map_update_);        // (":914")
    ApplyEssentialGraph(map, &P, lie.data());
    return n_edges;
  }

  // CeresOptimizer::GlobalBundleAdjustemnt -> BundleAdjustment, src/CeresOptimizer.cc:49-225, with BOTH halves around the optimisation in
  // the library (orbl_global_ba_assemble, orbl_global_ba_apply): `FrameOpsHip::GlobalBundleAdjustemnt(map_, 10, &is_stop_global_BA_,
  // n_loop_keyframe, false);` at src/LoopClosing.cc:656 and `FrameOpsHip::GlobalBundleAdjustemnt(map_, 20);` at src/Tracking.cc:502.
  // AssembleGlobalBA flattens the two lists - isBad(), id_, GetPose(), the intrinsics, GetWorldPos(), GetObservations() in their std::map
  // order with the undistorted keypoint of each; an observer outside `keyframes` becomes a table row that the list does not name - and
  // makes the problem CeresOptimizerT::BundleAdjustment makes.  ApplyGlobalBA reads isBad() again, runs the write-back on the tables and
  // carries it into the objects: SetPose, SetWorldPos, normal_vector_ / min_distance_ / max_distance_ (n_loop_keyframe == 0), or
  // global_BA_Tcw_ / global_BA_pose_ with n_BA_global_for_keyframe_ (n_loop_keyframe != 0).  As in the reference, no map mutex is taken.
  template <class KF, class MP> struct GlobalBAProblemT {
    std::vector<KF*> kfs; std::vector<MP*> pts; std::unordered_map<KF*, int> kf_at;
    int32_t counts[3] = {0, 0, 0};                                   // {ncam, npts_ba, nobs_ba}
    std::vector<int32_t> cam_kf, kf_cam, gpt_pt, pt_idx, gobs_cam, gobs_pt, gobs_src; std::vector<double> K4, poses7, pts3, gobs_uv, gobs_weight;
    std::vector<uint8_t> cam_fixed, gobs_robust; std::vector<float> scale_factors;
  };

  // Returns the number of rows of the problem.
  template <class KF, class MP>
  static int AssembleGlobalBA(const std::vector<KF*>& keyframes, const std::vector<MP*>& map_points, bool is_robust, GlobalBAProblemT<KF, MP>* P) {
    typedef typename std::decay<decltype(keyframes[0]->GetPose())>::type M4;
    *P = GlobalBAProblemT<KF, MP>();
    if (keyframes.empty()) return 0;                                  // (":67-70")
    std::vector<KF*>& kfs = P->kfs;
    auto kf_index = [&](KF* kf) {
      auto it = P->kf_at.find(kf);
      if (it == P->kf_at.end()) { it = P->kf_at.emplace(kf, (int)kfs.size()).first; kfs.push_back(kf); }
      return it->second;
    };
    std::vector<int32_t> ba_kf, obs_off(1, 0), obs_kf, obs_level;
    for (KF* kf : keyframes) ba_kf.push_back(kf_index(kf));
    std::unordered_map<MP*, int> pt_at;
    std::vector<MP*>& pts = P->pts;
    std::vector<double> X; std::vector<uint8_t> pt_bad; std::vector<float> obs_uv;
    for (MP* mp : map_points) {
      if (!mp || pt_at.count(mp)) continue;                           // (Map hands over a std::set: distinct)
      pt_at.emplace(mp, (int)pts.size()); pts.push_back(mp);
      const bool bad = mp->isBad();
      pt_bad.push_back(bad ? 1 : 0);
      const Vector3d Q = mp->GetWorldPos();
      for (int c = 0; c < 3; c++) X.push_back(Q[c]);
      if (!bad) {
        const auto observations = mp->GetObservations();
        for (const auto& o : observations) {
          const auto& kp = o.first->undistort_keypoints_[o.second];
          obs_kf.push_back(kf_index(o.first)); obs_level.push_back(kp.octave);
          obs_uv.push_back(kp.pt.x); obs_uv.push_back(kp.pt.y);
        }
      }
      obs_off.push_back((int32_t)obs_kf.size());
    }
    const int nkf = (int)kfs.size(), npts = (int)pts.size(), nobs = (int)obs_kf.size();
    std::vector<int32_t> kf_id(nkf); std::vector<uint8_t> kf_bad(nkf); std::vector<double> kf_Tcw(12 * (size_t)nkf), kf_K4(4 * (size_t)nkf);
    for (int k = 0; k < nkf; k++) {
      KF* kf = kfs[k];
      const M4 T = kf->GetPose();
      for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) kf_Tcw[12 * (size_t)k + 4 * r + c] = T(r, c);
      kf_id[k] = (int32_t)kf->id_; kf_bad[k] = kf->isBad() ? 1 : 0;
      kf_K4[4 * (size_t)k] = kf->fx_; kf_K4[4 * (size_t)k + 1] = kf->fy_; kf_K4[4 * (size_t)k + 2] = kf->cx_; kf_K4[4 * (size_t)k + 3] = kf->cy_;
    }
    KF* first = keyframes[0];
    const int n_levels = first->n_scale_levels_;
    const std::vector<float> isg(first->inv_level_sigma2s_.begin(), first->inv_level_sigma2s_.begin() + n_levels);
    P->scale_factors.assign(first->scale_factors_.begin(), first->scale_factors_.begin() + n_levels);
    const size_t cc = (size_t)std::min(nkf, (int)ba_kf.size()), cp = (size_t)std::max(npts, 1), co = (size_t)std::max(nobs, 1);
    P->cam_kf.resize(cc); P->kf_cam.resize(nkf); P->K4.resize(4 * cc); P->poses7.resize(7 * cc); P->cam_fixed.resize(cc); P->gpt_pt.resize(cp); P->pt_idx.resize(cp);
    P->pts3.resize(3 * cp); P->gobs_cam.resize(co); P->gobs_pt.resize(co); P->gobs_uv.resize(2 * co); P->gobs_weight.resize(co); P->gobs_robust.resize(co); P->gobs_src.resize(co);
    X.resize(3 * cp); pt_bad.resize(cp); obs_kf.resize(co); obs_level.resize(co); obs_uv.resize(2 * co);
    dropin::check(orbl_global_ba_assemble((int)ba_kf.size(), ba_kf.data(), npts, nullptr, nkf, kf_id.data(), kf_bad.data(), kf_Tcw.data(), kf_K4.data(), npts, X.data(),
                                          pt_bad.data(), obs_off.data(), obs_kf.data(), obs_uv.data(), obs_level.data(), isg.data(), n_levels, is_robust ? 1 : 0, (int)cc, npts,
                                          nobs, P->counts, P->cam_kf.data(), P->kf_cam.data(), P->K4.data(), P->poses7.data(), P->cam_fixed.data(), P->gpt_pt.data(),
                                          P->pt_idx.data(), P->pts3.data(), P->gobs_cam.data(), P->gobs_pt.data(), P->gobs_uv.data(), P->gobs_weight.data(),
                                          P->gobs_robust.data(), P->gobs_src.data()),
                  "orbl_global_ba_assemble");
    const size_t ncam = (size_t)P->counts[0], npb = (size_t)P->counts[1], nob = (size_t)P->counts[2];
    P->cam_kf.resize(ncam); P->K4.resize(4 * ncam); P->poses7.resize(7 * ncam); P->cam_fixed.resize(ncam); P->gpt_pt.resize(npb); P->pts3.resize(3 * npb);
    P->gobs_cam.resize(nob); P->gobs_pt.resize(nob); P->gobs_uv.resize(2 * nob); P->gobs_weight.resize(nob); P->gobs_robust.resize(nob); P->gobs_src.resize(nob);
    return (int)nob;
  }

  // poses7[ncam][7], pts3[npts_ba][3]: what ba_solve left.  Returns the number of points written.
  template <class KF, class MP>
  static int ApplyGlobalBA(GlobalBAProblemT<KF, MP>* P, const double* poses7, const double* pts3, const unsigned long n_loop_keyframe) {
    const int nkf = (int)P->kfs.size(), npts = (int)P->pts.size(), ncam = P->counts[0], npb = P->counts[1];
    if (ncam == 0) return 0;
    typedef typename std::decay<decltype(P->kfs[0]->GetPose())>::type M4;
    const int stage = n_loop_keyframe == 0 ? 0 : 1;
    const size_t np1 = (size_t)std::max(npts, 1);
    std::vector<uint8_t> kf_bad(nkf), pt_bad(np1, 0), wrote(np1, 0), on_host(np1, 0), kin(nkf, 0), pin(np1, 0);
    std::vector<double> Tcw(12 * (size_t)nkf), center(3 * (size_t)nkf), X(3 * np1, 0.0), normal(3 * np1, 0.0), gT(12 * (size_t)nkf, 0.0), gX(3 * np1, 0.0);
    std::vector<int32_t> pt_ref(np1, -1), ref_level(np1, 0), obs_off(1, 0), obs_kf;
    std::vector<float> mm(2 * np1, 0.f);
    for (int k = 0; k < nkf; k++) {
      kf_bad[k] = P->kfs[k]->isBad() ? 1 : 0;                         // (":193": read again)
      const M4 T = P->kfs[k]->GetPose();
      const Vector3d O = P->kfs[k]->GetCameraCenter();
      for (int r = 0; r < 3; r++) { for (int c = 0; c < 4; c++) Tcw[12 * (size_t)k + 4 * r + c] = T(r, c); center[3 * (size_t)k + r] = O[r]; }
    }
    for (int p = 0; p < npts; p++) {
      MP* mp = P->pts[p];
      pt_bad[p] = mp->isBad() ? 1 : 0;                                // (":214")
      if (stage == 0 && !pt_bad[p] && P->pt_idx[p] >= 0) {             // (what UpdateNormalAndDepth snapshots, src/MapPoint.cc:339-371)
        const Vector3d Q = mp->GetWorldPos();
        for (int c = 0; c < 3; c++) X[3 * (size_t)p + c] = Q[c];
        KF* rk = mp->GetReferenceKeyFrame();
        auto rit = rk ? P->kf_at.find(rk) : P->kf_at.end();
        pt_ref[p] = rit == P->kf_at.end() ? -1 : rit->second;
        bool all_known = pt_ref[p] >= 0;
        const auto observations = mp->GetObservations();
        size_t kp = 0;
        const size_t first = obs_kf.size();
        for (const auto& o : observations) { auto oit = P->kf_at.find(o.first); if (oit == P->kf_at.end()) { all_known = false; break; } obs_kf.push_back(oit->second); if (o.first == rk) kp = o.second; }
        if (!all_known) { obs_kf.resize(first); pt_ref[p] = -1; on_host[p] = rk ? 1 : 0; }      // (an observer the flattening does not know: the object's own UpdateNormalAndDepth below)
        else if (!observations.empty()) ref_level[p] = rk->undistort_keypoints_[kp].octave;
      }
      obs_off.push_back((int32_t)obs_kf.size());
    }
    if (obs_kf.empty()) obs_kf.push_back(0);
    int32_t counts[3] = {0, 0, 0};
    const bool s0 = stage == 0;
    dropin::check(orbl_global_ba_apply(ncam, P->cam_kf.data(), poses7, npb, P->gpt_pt.data(), pts3, stage, nkf, kf_bad.data(), s0 ? Tcw.data() : nullptr,
                                       s0 ? center.data() : nullptr, npts, s0 ? X.data() : nullptr, pt_bad.data(), s0 ? nullptr : gT.data(), s0 ? nullptr : kin.data(),
                                       s0 ? nullptr : gX.data(), s0 ? nullptr : pin.data(), s0 ? pt_ref.data() : nullptr, s0 ? obs_off.data() : nullptr,
                                       s0 ? obs_kf.data() : nullptr, s0 ? ref_level.data() : nullptr, s0 ? P->scale_factors.data() : nullptr, (int)P->scale_factors.size(),
                                       s0 ? normal.data() : nullptr, s0 ? mm.data() : nullptr, s0 ? wrote.data() : nullptr, counts),
                  "orbl_global_ba_apply");
    for (int c = 0; c < ncam; c++) {                                  // (":190-205")
      const int k = P->cam_kf[c];
      if (kf_bad[k]) continue;
      M4 T = P->kfs[k]->GetPose();
      const double* src = (s0 ? Tcw.data() : gT.data()) + 12 * (size_t)k;
      for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) T(i, j) = src[4 * i + j];
      T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
      if (s0) P->kfs[k]->SetPose(T);
      else { P->kfs[k]->global_BA_Tcw_ = T; P->kfs[k]->n_BA_global_for_keyframe_ = n_loop_keyframe; }
    }
    for (int j = 0; j < npb; j++) {                                   // (":208-224")
      const int p = P->gpt_pt[j];
      if (pt_bad[p]) continue;
      MP* mp = P->pts[p];
      Vector3d Q, v;
      const double* src = (s0 ? X.data() : gX.data()) + 3 * (size_t)p;
      for (int c = 0; c < 3; c++) { Q[c] = src[c]; v[c] = normal[3 * (size_t)p + c]; }
      if (!s0) { mp->global_BA_pose_ = Q; mp->n_BA_global_for_keyframe_ = n_loop_keyframe; continue; }
      mp->SetWorldPos(Q);
      if (wrote[p]) {
        std::unique_lock<std::mutex> lock = lock_pose(mp, 0);
        mp->max_distance_ = mm[2 * (size_t)p + 1]; mp->min_distance_ = mm[2 * (size_t)p]; mp->normal_vector_ = v;
      } else if (on_host[p]) mp->UpdateNormalAndDepth();
    }
    return counts[1];
  }

  // Returns the number of rows of the problem (0: nothing to optimise, nothing written).  The write-back also runs after a raised stop
  // flag, as in the reference; RunGlobalBundleAdjustment decides afterwards whether to propagate.
  template <class MapT>
  static int GlobalBundleAdjustemnt(MapT* map, int n_iterations = 200, bool* stop_flag = nullptr, const unsigned long n_loop_keyframe = 0, const bool is_robust = true) {
    typedef typename std::remove_pointer<typename std::decay<decltype(map->GetAllKeyFrames()[0])>::type>::type KF;
    typedef typename std::remove_pointer<typename std::decay<decltype(map->GetAllMapPoints()[0])>::type>::type MP;
    const std::vector<KF*> keyframes = map->GetAllKeyFrames();
    const std::vector<MP*> map_points = map->GetAllMapPoints();
    GlobalBAProblemT<KF, MP> P;
    const int nob = AssembleGlobalBA(keyframes, map_points, is_robust, &P);
    if (P.counts[0] == 0) return 0;
    std::vector<double> poses7 = P.poses7, pts3 = P.pts3;
    if (nob > 0) {
      ba_options o; o.max_iterations = n_iterations; o.huber_delta = std::sqrt(5.991); o.fix_points = 0;
      o.stop_flag = reinterpret_cast<const volatile uint8_t*>(stop_flag);
      dropin::check(ba_solve(P.K4.data(), poses7.data(), P.cam_fixed.data(), P.counts[0], pts3.data(), P.counts[1], P.gobs_cam.data(), P.gobs_pt.data(), P.gobs_uv.data(),
                             P.gobs_weight.data(), P.gobs_robust.data(), nob, &o, nullptr),
                    "ba_solve");
    }
    ApplyGlobalBA(&P, poses7.data(), pts3.data(), n_loop_keyframe);
    return nob;
  }

 private:
  // the reference's KeyFrame::mutex_connections_ when the type has it
  template <class P> static auto lock_connections(P* p, int) -> decltype((void)p->mutex_connections_, std::unique_lock<std::mutex>()) {
    return std::unique_lock<std::mutex>(p->mutex_connections_);
  }
  template <class P> static std::unique_lock<std::mutex> lock_connections(P*, long) { return std::unique_lock<std::mutex>(); }
  // the reference's MapPoint::mutex_features_ / mutex_pose_ when the type has them (the mock data model of tests/cpp has none)
  template <class P> static auto lock_features(P* p, int) -> decltype((void)p->mutex_features_, std::unique_lock<std::mutex>()) {
    return std::unique_lock<std::mutex>(p->mutex_features_);
  }
  template <class P> static std::unique_lock<std::mutex> lock_features(P*, long) { return std::unique_lock<std::mutex>(); }
  template <class P> static auto lock_pose(P* p, int) -> decltype((void)p->mutex_pose_, std::unique_lock<std::mutex>()) {
    return std::unique_lock<std::mutex>(p->mutex_pose_);
  }
  template <class P> static std::unique_lock<std::mutex> lock_pose(P*, long) { return std::unique_lock<std::mutex>(); }
};

}  // namespace ORB_SLAM2

#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES
// Inside the reference tree (Frame.h, KeyFrame.h, MapPoint.h, Map.h, Eigen and OpenCV already included): the classes the
// call sites name.  src/ORBmatcher.cc and the three CeresOptimizer methods above drop out of the build.
namespace ORB_SLAM2 {
struct ReferenceTypes {
  typedef ORB_SLAM2::Frame Frame; typedef ORB_SLAM2::KeyFrame KeyFrame; typedef ORB_SLAM2::MapPoint MapPoint; typedef ORB_SLAM2::Map Map;
  typedef Eigen::Matrix3d Matrix3d; typedef Eigen::Matrix4d Matrix4d; typedef Eigen::Vector2d Vector2d; typedef Eigen::Vector3d Vector3d;
  typedef Eigen::Quaterniond Quaterniond; typedef cv::Mat Mat; typedef cv::Point2f Point2f;
  typedef Sophus::Sim3d Sim3; typedef LoopClosing::KeyFrameAndSim3 KeyFrameAndSim3;
};
typedef ORBmatcherT<ReferenceTypes> ORBmatcher;
typedef CeresOptimizerT<ReferenceTypes> CeresOptimizerHip;      // every static of include/CeresOptimizer.h:351-388
typedef FrameOpsT<ReferenceTypes> FrameOpsHip;
}  // namespace ORB_SLAM2
#endif
