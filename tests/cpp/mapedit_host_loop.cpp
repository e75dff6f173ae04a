// mapedit_host_loop.cpp -- the host loop tools/map_edits_time.py compares orbl_apply_map_edits with: the edit list of one call replayed by
// the MapPoint::AddObservation / Replace bodies of the shared mock data model (mock_orbslam.h: std::map / std::vector members under the
// reference's names) and a literal SetBadFlag (src/MapPoint.cc:174-191), compiled -O2.  The mock's Replace runs ComputeDistinctiveDescriptors
// inside the loop, as the reference does (all-zero descriptors here); the table call leaves that to orbl_update_map_points.  It also
// times what a host caller pays to hand the map to the table calls: flattening every observations_ map into the CSR tables.
//   mapedit_host_loop <problem file> <reps>   ->   "TIME loop_ms <median> flatten_ms <median> n_obs <final observations> n_bad <bad points>"
// The problem file is int32 words: nkf npts nslots nobs nops | kf_slot_off[nkf + 1] | kf_slot_pt[nslots] | obs_off[npts + 1] | obs_kf[nobs] |
// obs_slot[nobs] | pt_bad[npts] | pt_nobs[npts] | op_kind | op_pt | op_arg | op_kf | op_slot [nops each].
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "mock_orbslam.h"

using mock::KeyFrame;
using mock::MapPoint;

// MapPoint::SetBadFlag (src/MapPoint.cc:174-191), which the shared mock does not have; map_->EraseMapPoint stays with the caller
static void set_bad_flag(MapPoint* mp) {
  std::map<KeyFrame*, size_t> obs = mp->observations_;
  mp->is_bad_ = true;
  mp->observations_.clear();
  for (auto& kv : obs) kv.first->EraseMapPointMatch(kv.second);
}

struct Map { std::vector<KeyFrame> kfs; std::vector<MapPoint> pts; };

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: mapedit_host_loop <problem file> <reps>\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  const int reps = std::atoi(argv[2]);
  int32_t h[5];
  if (std::fread(h, 4, 5, f) != 5) return 2;
  const int nkf = h[0], npts = h[1], nslots = h[2], nobs = h[3], nops = h[4];
  auto rd = [&](size_t n) { std::vector<int32_t> v(n); if (n && std::fread(v.data(), 4, n, f) != n) std::exit(2); return v; };
  const std::vector<int32_t> slot_off = rd(nkf + 1), slot_pt = rd(nslots), obs_off = rd(npts + 1), obs_kf = rd(nobs), obs_slot = rd(nobs), pt_bad = rd(npts),
                             pt_nobs = rd(npts), op_kind = rd(nops), op_pt = rd(nops), op_arg = rd(nops), op_kf = rd(nops), op_slot = rd(nops);
  std::fclose(f);
  std::vector<double> t_loop, t_flat;
  long n_obs_out = 0, n_bad = 0;
  for (int rep = 0; rep < reps; rep++) {
    Map m;                                                              // a fresh map per repetition, built outside the timed spans
    m.kfs.resize(nkf); m.pts.resize(npts);
    for (int k = 0; k < nkf; k++) {
      m.kfs[k].N_ = slot_off[k + 1] - slot_off[k];
      m.kfs[k].map_points_.resize(m.kfs[k].N_);
      m.kfs[k].descriptors_ = mock::Mat(m.kfs[k].N_);
      for (int s = slot_off[k]; s < slot_off[k + 1]; s++) m.kfs[k].map_points_[s - slot_off[k]] = slot_pt[s] >= 0 ? &m.pts[slot_pt[s]] : nullptr;
    }
    for (int p = 0; p < npts; p++) {
      MapPoint& mp = m.pts[p];
      mp.id_ = (unsigned long)p; mp.is_bad_ = pt_bad[p] != 0; mp.n_observations_ = pt_nobs[p];
      for (int e = obs_off[p]; e < obs_off[p + 1]; e++) mp.observations_[&m.kfs[obs_kf[e]]] = (size_t)obs_slot[e];
    }
    std::vector<MapPoint*> found(nops, nullptr);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < nops; i++) {
      MapPoint* mp = op_kind[i] ? &m.pts[op_pt[i]] : nullptr;
      KeyFrame* kf = (op_kind[i] == 1 || op_kind[i] == 4 || op_kind[i] == 5) ? &m.kfs[op_kf[i]] : nullptr;
      const size_t idx = (size_t)op_slot[i];
      switch (op_kind[i]) {
        case 1:
          mp->AddObservation(kf, idx); kf->AddMapPoint(mp, idx);
          if (op_arg[i] & 1) mp->ComputeDistinctiveDescriptors();
          break;
        case 2: mp->Replace(&m.pts[op_arg[i]]); break;
        case 3: set_bad_flag(mp); break;
        case 4: {                                                       // ORBmatcher::Fuse (src/ORBmatcher.cc:746, :824-838)
          if (mp->isBad() || mp->IsInKeyFrame(kf)) break;
          MapPoint* in_kf = kf->GetMapPoint(idx);
          if (in_kf) {
            if (!in_kf->isBad()) {
              found[i] = in_kf;
              if (in_kf->Observations() > mp->Observations()) mp->Replace(in_kf);
              else in_kf->Replace(mp);
            }
          } else {
            mp->AddObservation(kf, idx); kf->AddMapPoint(mp, idx);
          }
          break;
        }
        case 5: {                                                       // (src/ORBmatcher.cc:941-950)
          MapPoint* in_kf = kf->GetMapPoint(idx);
          if (in_kf) { if (!in_kf->isBad()) found[i] = in_kf; }
          else { mp->AddObservation(kf, idx); kf->AddMapPoint(mp, idx); }
          break;
        }
        case 6: if (found[op_arg[i]]) found[op_arg[i]]->Replace(mp); break;      // (src/LoopClosing.cc:615-621)
        default: break;
      }
    }
    const auto t1 = std::chrono::steady_clock::now();
    // what the table calls want from a host map: every observations_ flattened into CSR, in map order
    std::vector<int32_t> f_off(npts + 1, 0), f_kf, f_slot;
    f_kf.reserve(nobs + nops); f_slot.reserve(nobs + nops);
    for (int p = 0; p < npts; p++) {
      for (auto& kv : m.pts[p].observations_) { f_kf.push_back((int32_t)(kv.first - m.kfs.data())); f_slot.push_back((int32_t)kv.second); }
      f_off[p + 1] = (int32_t)f_kf.size();
    }
    const auto t2 = std::chrono::steady_clock::now();
    t_loop.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    t_flat.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    n_obs_out = (long)f_kf.size(); n_bad = 0;
    for (int p = 0; p < npts; p++) n_bad += m.pts[p].is_bad_;
  }
  std::printf("TIME loop_ms %.4f flatten_ms %.4f n_obs %ld n_bad %ld\n", median(t_loop), median(t_flat), n_obs_out, n_bad);
  return 0;
}
