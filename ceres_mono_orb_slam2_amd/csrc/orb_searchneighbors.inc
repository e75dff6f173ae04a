// orb_searchneighbors.inc -- LocalMapping::SearchInNeighbors (src/LocalMapping.cc:398-488) on the resident map tables: what a caller
// needs between orbl_apply_map_edits and orbl_update_map_points to run the whole function without a host copy of the map
// (orbl_fuse_targets*, orbl_fuse_rows*, orbl_fuse_candidates*, orbl_update_map_points_on_tables*).  Textually included by
// orb_localmap.hip.
//
// The loop stays exact because one keyframe's Fuse searches with the descriptors held at its entry (DESIGN.md section 2,
// "SearchInNeighbors on the tables"): per target keyframe the caller enqueues k_sn_rows (all points in parallel, FUSE rows out),
// orbl_apply_map_edits_device (the replay decides bad flags, IsInKeyFrame and the slots at each row's own turn) and
// orbl_update_map_points_on_tables_device (the descriptors of the touched points).  Launches:
//   k_sn_targets      ONE wave, one lane working: the target list of :400-431 in call order, the stamps written as the loop writes them.
//   k_sn_rows         one wave per point: the projection and its gates (src/ORBmatcher.cc:739-782) by every lane alike, then the lanes
//                     share the keyframe's slots.  No grid table: a keypoint's own cell (Frame::PosInGrid) is tested against the cell
//                     range of KeyFrame::GetFeaturesInArea, and the wave minimises (distance, cell x, cell y, index) - the order in
//                     which GetFeaturesInArea returns the keypoints, so the first of equal distances wins as `dist < bestDist` has it.
//   k_sn_cand_mark    one lane per slot of every listed target: atomicMin of (position in the list, slot) per point - a minimum, so the
//                     order of the atomics decides nothing.
//   k_sn_cand_scan    one workgroup per listed target, twice: the winners counted, then - after k_mt_scan_sums - placed by an ordered scan.
//   k_sn_mask_kf, k_sn_gather, k_sn_scatter   orbl_update_map_points_on_tables: the selection, the observations' descriptors gathered
//                     through (obs_kf, obs_slot), and the depth range moved from k_mp_prep's pair layout to the two point tables; the
//                     work between them is k_mp_prep / k_mp_desc of orb_mappoint.inc, unchanged.
// The tables a later kernel of the chain mutates (kf_slot_pt, pt_bad, pt_desc, the stamps) carry no __restrict__.  No atomic decides a
// position; outputs are vector stores; nothing is written beyond a count or a capacity.
#include "orb_maptable.h"

namespace orbhip {

#define SN_WG 256
#define SN_ST_OFFSETS 1u          /* *status bits of the device forms */
#define SN_ST_KF 2u
#define SN_ST_PT 4u
#define SN_ST_LEVEL 8u
#define SN_ST_CAP 16u
#define SN_ST_SLOT 32u
#define SN_TH_LOW 50              /* ORBmatcher::TH_LOW */
#define SN_CAND_BX 8              /* k_sn_cand_mark: workgroups per listed target */

// ------------------------------------------------------------------------------------------------------------------ the targets
struct SnTgtArgs {
  int cur_kf, cur_id, nkf, nord, nn, nn2, cap;
  const uint8_t* kf_bad; const int32_t *ord_off, *ord_kf; int32_t* stamp; int32_t *tgt, *counts; uint32_t* status;
};

__device__ __forceinline__ void sn_push(const SnTgtArgs& a, int k, int* n) { if (*n < a.cap) a.tgt[*n] = k; (*n)++; }

__global__ __launch_bounds__(64) void k_sn_targets(SnTgtArgs a) {
  if (threadIdx.x != 0) return;                                           // (at most nn * (1 + nn2) steps, each reading what the last wrote)
  int n_out = 0, n_first = 0, lo, hi;
  if (a.cur_kf < 0 || a.cur_kf >= a.nkf) mt_flag(a.status, SN_ST_KF);
  else if (!mt_range(a.ord_off, a.cur_kf, a.nord, &lo, &hi)) mt_flag(a.status, SN_ST_OFFSETS);
  else {
    const int e1 = hi - lo > a.nn ? lo + a.nn : hi;                       // GetBestCovisibilityKeyFrames(nn)
    for (int e = lo; e < e1; e++) {
      const int n = a.ord_kf[e];
      if (n < 0 || n >= a.nkf) { mt_flag(a.status, SN_ST_KF); continue; }
      if ((a.kf_bad && a.kf_bad[n]) || a.stamp[n] == a.cur_id) continue;  // (:409-413)
      sn_push(a, n, &n_out);
      a.stamp[n] = a.cur_id;
      n_first++;
      int l2, h2;
      if (!mt_range(a.ord_off, n, a.nord, &l2, &h2)) { mt_flag(a.status, SN_ST_OFFSETS); continue; }
      const int e2 = h2 - l2 > a.nn2 ? l2 + a.nn2 : h2;
      for (int f = l2; f < e2; f++) {
        const int k2 = a.ord_kf[f];
        if (k2 < 0 || k2 >= a.nkf) { mt_flag(a.status, SN_ST_KF); continue; }
        if ((a.kf_bad && a.kf_bad[k2]) || a.stamp[k2] == a.cur_id || k2 == a.cur_kf) continue;      // (:425-428)
        sn_push(a, k2, &n_out);                                           // (:429) no stamp: it may come again
      }
    }
  }
  a.counts[0] = n_out; a.counts[1] = n_first;
  if (n_out > a.cap) mt_flag(a.status, SN_ST_CAP);
}

// ------------------------------------------------------------------------------------------------------------------ the rows
struct SnRowArgs {
  int n, nkf, nslots, npts, n_levels; float log_scale, th;
  const int32_t *d_kf, *pts;
  const double *kf_Tcw, *kf_center; const float *kf_K4, *kf_bounds; const int32_t* slot_off; const float* slot_uv; const int32_t* slot_level; const uint32_t* slot_desc;
  const double *pt_Xw, *pt_normal; const float *pt_min, *pt_max; const uint32_t* pt_desc;
  const float *scale_factors, *inv_sigma2;
  int32_t *op_kind, *op_pt, *op_arg, *op_kf, *op_slot, *best_idx, *best_dist; float* q_uv; int32_t* q_level; uint32_t* status;
};

__global__ __launch_bounds__(SN_WG) void k_sn_rows(SnRowArgs a) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (SN_WG / 64) + (threadIdx.x >> 6);
  if (i >= a.n) return;                                                   // (wave-uniform, as everything up to the slot loop)
  const int K = a.d_kf[0], p = a.pts[i];
  const bool kf_ok = K >= 0 && K < a.nkf, pt_ok = p >= 0 && p < a.npts;
  int lo = 0, hi = 0, level = -1;
  float u = 0.f, v = 0.f;
  if (!kf_ok) mt_flag(a.status, SN_ST_KF);
  else if (!mt_range(a.slot_off, K, a.nslots, &lo, &hi)) mt_flag(a.status, SN_ST_OFFSETS);
  if (p < -1 || p >= a.npts) mt_flag(a.status, SN_ST_PT);
  unsigned long long best = ~0ull;
  if (kf_ok && pt_ok) {
    const double* X = a.pt_Xw + 3 * (size_t)p;
    const double* Pn = a.pt_normal + 3 * (size_t)p;
    const double* Ow = a.kf_center + 3 * (size_t)K;
    const float* K4 = a.kf_K4 + 4 * (size_t)K;
    const float* B = a.kf_bounds + 4 * (size_t)K;
    const float min_x = B[0], max_x = B[1], min_y = B[2], max_y = B[3];
    double c[3];
    mc_apply34(a.kf_Tcw + 12 * (size_t)K, X, c);                          // p3Dc = Rcw p3Dw + tcw (src/ORBmatcher.cc:750)
    bool ok = !(c[2] < 0.0);                                              // (:753)
    const float invz = (float)(1.0 / c[2]);
    const float x = (float)(c[0] * (double)invz), y = (float)(c[1] * (double)invz);
    u = K4[0] * x + K4[2]; v = K4[1] * y + K4[3];
    ok = ok && u >= min_x && u < max_x && v >= min_y && v < max_y;        // KeyFrame::IsInImage (src/KeyFrame.cc:624)
    const double POx = X[0] - Ow[0], POy = X[1] - Ow[1], POz = X[2] - Ow[2];
    const float dist = (float)sqrt((POx * POx + POy * POy) + POz * POz);
    const float max_d = a.pt_max[p];
    ok = ok && !(dist < 0.8f * a.pt_min[p] || dist > 1.2f * max_d);        // (:768-771)
    ok = ok && !((POx * Pn[0] + POy * Pn[1]) + POz * Pn[2] < 0.5 * (double)dist);          // (:774-777)
    if (ok) {
      const float ratio = max_d / dist;                                   // MapPoint::PredictScale, the project's one form (orb_frame.h)
      level = (int)ceilf(logf(ratio) / a.log_scale);
      if (level < 0) level = 0; else if (level >= a.n_levels) level = a.n_levels - 1;
      const float r = a.th * a.scale_factors[level];
      const float winv = (float)FRAME_GRID_COLS / (max_x - min_x), hinv = (float)FRAME_GRID_ROWS / (max_y - min_y);
      // KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:575-622): the cell range and its early-outs
      const int min_cx = max(0, (int)floorf((u - min_x - r) * winv)), max_cx = min(FRAME_GRID_COLS - 1, (int)ceilf((u - min_x + r) * winv));
      const int min_cy = max(0, (int)floorf((v - min_y - r) * hinv)), max_cy = min(FRAME_GRID_ROWS - 1, (int)ceilf((v - min_y + r) * hinv));
      if (!(min_cx >= FRAME_GRID_COLS || max_cx < 0 || min_cy >= FRAME_GRID_ROWS || max_cy < 0)) {
        uint32_t d1[8];
#pragma unroll
        for (int k = 0; k < 8; k++) d1[k] = a.pt_desc[8 * (size_t)p + k];
        for (int s = lo + lane; s < hi; s += 64) {
          const float kx = a.slot_uv[2 * (size_t)s], ky = a.slot_uv[2 * (size_t)s + 1];
          const int px = (int)roundf((kx - min_x) * winv), py = (int)roundf((ky - min_y) * hinv);     // Frame::PosInGrid (src/Frame.cc:309-320)
          if (px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS) continue;          // (the keypoint is in no cell)
          if (px < min_cx || px > max_cx || py < min_cy || py > max_cy) continue;
          if (!(fabsf(kx - u) < r && fabsf(ky - v) < r)) continue;        // (src/KeyFrame.cc:607-611)
          const int lvl = a.slot_level[s];
          if (lvl < level - 1 || lvl > level) continue;                    // (src/ORBmatcher.cc:781)
          if (lvl < 0) { mt_flag(a.status, SN_ST_LEVEL); continue; }
          const float ex = u - kx, ey = v - ky;
          const float e2 = ex * ex + ey * ey;
          if ((double)(e2 * a.inv_sigma2[lvl]) > 5.99) continue;            // (:789)
          int d = 0;
#pragma unroll
          for (int k = 0; k < 8; k++) d += __popc(d1[k] ^ a.slot_desc[8 * (size_t)s + k]);
          const unsigned long long key = ((unsigned long long)(unsigned)d << 44) | ((unsigned long long)(unsigned)px << 38) | ((unsigned long long)(unsigned)py << 32) |
                                         (unsigned long long)(unsigned)(s - lo);
          best = key < best ? key : best;
        }
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o < best ? o : best;
  }
  if (lane != 0) return;
  const int bi = best == ~0ull ? -1 : (int)(best & 0xFFFFFFFFull), bd = best == ~0ull ? 256 : (int)(best >> 44);
  const bool fuse = bd <= SN_TH_LOW;                                      // (:801)
  a.op_kind[i] = fuse ? 4 : 0; a.op_pt[i] = pt_ok ? p : -1; a.op_arg[i] = 0; a.op_kf[i] = K; a.op_slot[i] = fuse ? bi : -1;
  if (a.best_idx) a.best_idx[i] = bi;
  if (a.best_dist) a.best_dist[i] = bd;
  if (a.q_uv) { a.q_uv[2 * (size_t)i] = level >= 0 ? u : 0.f; a.q_uv[2 * (size_t)i + 1] = level >= 0 ? v : 0.f; }
  if (a.q_level) a.q_level[i] = level;
}

// ------------------------------------------------------------------------------------------------------------------ the candidates
struct SnCandArgs {
  int n_tgt, nkf, nslots, npts, cur_id, cap;
  const int32_t *tgt, *slot_off, *slot_pt; const uint8_t* pt_bad; int32_t* stamp; int32_t *cand, *counts; uint32_t* status;
  unsigned long long* first;      // workspace: first[npts], preset to ~0 | tcnt[n_tgt + 1]
  int32_t* tcnt;
};

// the slots of listed target t, empty when the entry names no keyframe
__device__ __forceinline__ bool sn_tgt_range(const SnCandArgs& a, int t, int* lo, int* hi, bool flag) {
  const int k = a.tgt[t];
  *lo = *hi = 0;
  if (k < 0 || k >= a.nkf) { if (flag) mt_flag(a.status, SN_ST_KF); return false; }
  if (!mt_range(a.slot_off, k, a.nslots, lo, hi)) { if (flag) mt_flag(a.status, SN_ST_OFFSETS); return false; }
  return true;
}

__global__ __launch_bounds__(SN_WG) void k_sn_cand_mark(SnCandArgs a) {
  const int t = blockIdx.x / SN_CAND_BX, b = blockIdx.x % SN_CAND_BX;
  int lo, hi;
  if (!sn_tgt_range(a, t, &lo, &hi, b == 0 && threadIdx.x == 0)) return;
  for (int s = b * SN_WG + (int)threadIdx.x; s < hi - lo; s += SN_CAND_BX * SN_WG) {
    const int p = a.slot_pt[lo + s];
    if (p < 0 || p >= a.npts) { if (p != -1) mt_flag(a.status, SN_ST_PT); continue; }
    if (a.pt_bad[p] || a.stamp[p] == a.cur_id) continue;                  // (:463-466), the stamps as they stand at entry
    atomicMin(&a.first[p], ((unsigned long long)(unsigned)t << 32) | (unsigned)s);
  }
}

template <bool EMIT>
__global__ __launch_bounds__(SN_WG) void k_sn_cand_scan(SnCandArgs a) {
  __shared__ int sw[SN_WG / 64];
  const int t = blockIdx.x;
  if (EMIT && t == a.n_tgt) {                                             // the last workgroup: the totals
    if (threadIdx.x == 0) {
      const int total = a.tcnt[a.n_tgt];
      a.counts[0] = total; a.counts[1] = a.n_tgt;
      if (total > a.cap) mt_flag(a.status, SN_ST_CAP);
    }
    return;
  }
  int lo, hi;
  sn_tgt_range(a, t, &lo, &hi, false);
  const int off = EMIT ? a.tcnt[t] : 0;
  int carry = 0;
  for (int s0 = 0; s0 < hi - lo; s0 += SN_WG) {                           // (workgroup-uniform)
    const int s = s0 + (int)threadIdx.x;
    const int p = s < hi - lo ? a.slot_pt[lo + s] : -1;
    const bool win = p >= 0 && p < a.npts && a.first[p] == (((unsigned long long)(unsigned)t << 32) | (unsigned)s);
    int tot;
    const int ex = mt_block_excl<SN_WG>(win ? 1 : 0, sw, &tot);
    if (EMIT && win && off + carry + ex < a.cap) {
      a.cand[off + carry + ex] = p;
      a.stamp[p] = a.cur_id;                                              // (:467)
    }
    carry += tot;
  }
  if (!EMIT && threadIdx.x == 0) a.tcnt[t] = carry;
}

struct SnCandWs { size_t first, tcnt, total; };
static SnCandWs sn_cand_workspace(int n_tgt, int npts) {
  SnCandWs w; Carve ws;
  w.first = ws.take(8 * (size_t)npts); w.tcnt = ws.take(4 * ((size_t)n_tgt + 1));
  w.total = ws.total;
  return w;
}

// ------------------------------------------------------------------------------------------------------------------ the point update
struct SnUpdArgs {
  int npts, nkf, nslots, nobs, mask_kf;
  const uint8_t *pt_mask, *pt_bad, *kf_bad; const int32_t *obs_off, *obs_kf, *obs_slot, *slot_off, *slot_pt, *slot_level, *pt_ref_kf; const uint32_t* slot_desc;
  uint8_t *sel, *good, *obs_good; int32_t* ref_level; uint32_t* obs_desc; uint32_t* status;
  const uint8_t* nd_written; const float* min_max; float *pt_min, *pt_max;
};

__device__ __forceinline__ int sn_slot_at(const int32_t* slot_off, int nkf, int nslots, int k, int s) {
  int lo, hi;
  if (k < 0 || k >= nkf || !mt_range(slot_off, k, nslots, &lo, &hi) || s < 0 || s >= hi - lo) return -1;
  return lo + s;
}

// "the non-null slots of keyframe mask_kf" (src/LocalMapping.cc:475-484); the stores of one point are equal
__global__ __launch_bounds__(SN_WG) void k_sn_mask_kf(SnUpdArgs a) {
  int lo, hi;
  if (!mt_range(a.slot_off, a.mask_kf, a.nslots, &lo, &hi)) { if (blockIdx.x == 0 && threadIdx.x == 0) mt_flag(a.status, SN_ST_OFFSETS); return; }
  for (int s = lo + blockIdx.x * SN_WG + (int)threadIdx.x; s < hi; s += gridDim.x * SN_WG) {
    const int p = a.slot_pt[s];
    if (p >= 0 && p < a.npts) a.sel[p] = 1;
    else if (p != -1) mt_flag(a.status, SN_ST_PT);
  }
}

// 8 lanes per point, lane r moving word r of every descriptor: what orbl_update_map_points takes as obs_desc / obs_kf_good / pt_good /
// ref_level, for the selected points only
__global__ __launch_bounds__(SN_WG) void k_sn_gather(SnUpdArgs a) {
  const int g = blockIdx.x * SN_WG + threadIdx.x, p = g >> 3, r = g & 7;
  if (p >= a.npts) return;
  int lo, hi;
  bool on = (a.sel[p] || (a.pt_mask && a.pt_mask[p])) && !a.pt_bad[p];
  if (on && !mt_range(a.obs_off, p, a.nobs, &lo, &hi)) { on = false; mt_flag(a.status, SN_ST_OFFSETS); }
  if (!on) { if (r == 0) { a.good[p] = 0; a.ref_level[p] = -1; } return; }
  const int ref = a.pt_ref_kf ? a.pt_ref_kf[p] : -1;
  int lvl = -1; bool found = false;
  for (int e = lo; e < hi; e++) {
    const int k = a.obs_kf[e], at = sn_slot_at(a.slot_off, a.nkf, a.nslots, k, a.obs_slot[e]);
    if (at < 0) {                                                         // an observation out of range is absent
      mt_flag(a.status, k < 0 || k >= a.nkf ? SN_ST_KF : SN_ST_SLOT);
      if (r == 0) a.obs_good[e] = 0;
      a.obs_desc[8 * (size_t)e + r] = 0u;
      continue;
    }
    if (r == 0) a.obs_good[e] = !(a.kf_bad && a.kf_bad[k]);
    a.obs_desc[8 * (size_t)e + r] = a.slot_desc[8 * (size_t)at + r];
    if (k == ref && !found) { found = true; lvl = a.slot_level ? a.slot_level[at] : -1; }
  }
  if (!found && a.slot_level) {                                           // std::map::operator[] on the local copy: keypoint 0 of the reference keyframe
    const int at = sn_slot_at(a.slot_off, a.nkf, a.nslots, ref, 0);
    if (at >= 0) lvl = a.slot_level[at];
  }
  if (r == 0) { a.good[p] = 1; a.ref_level[p] = lvl; }
}

__global__ __launch_bounds__(SN_WG) void k_sn_scatter(SnUpdArgs a) {
  const int p = blockIdx.x * SN_WG + threadIdx.x;
  if (p >= a.npts || !a.nd_written[p]) return;
  a.pt_min[p] = a.min_max[2 * (size_t)p]; a.pt_max[p] = a.min_max[2 * (size_t)p + 1];
}

// workspace sections, each rounded up to 256 bytes; [0, cleared) is zeroed by every call
struct SnUpdWs { size_t sel, cleared, good, ref_level, best_obs, nd_written, min_max, obs_good, obs_desc, mp, total; };
static SnUpdWs sn_upd_workspace(int npts, int nobs) {
  SnUpdWs w; Carve ws;
  const size_t np = (size_t)npts, no = (size_t)nobs;
  w.sel = ws.take(np);
  w.cleared = ws.total;
  w.good = ws.take(np); w.ref_level = ws.take(4 * np); w.best_obs = ws.take(4 * np); w.nd_written = ws.take(np); w.min_max = ws.take(8 * np);
  w.obs_good = ws.take(no); w.obs_desc = ws.take(32 * no); w.mp = ws.take(mp_workspace_bytes(npts));
  w.total = ws.total;
  return w;
}

}  // namespace orbhip

extern "C" {

// ================================================================================================================== orbl_fuse_targets
int orbl_fuse_targets_workspace(int nkf, size_t* bytes) {
  ORBHIP_REQUIRE(nkf >= 0 && bytes, ORBHIP_EINVAL, "orbl_fuse_targets_workspace: bad argument");
  *bytes = 0;                                                             // (one wave, no scratch: the form is kept for the siblings' sake)
  return 0;
}

int orbl_fuse_targets_device(int cur_kf, int cur_id, int nkf, const uint8_t* kf_bad, int nord, const int32_t* ord_off, const int32_t* ord_kf, int32_t* kf_fuse_target,
                             int nn, int nn2, int cap_tgt, int32_t* tgt_kf, int32_t* counts, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  (void)workspace;
  ORBHIP_REQUIRE(nkf >= 0 && nord >= 0 && nn >= 0 && nn2 >= 0 && cap_tgt >= 0, ORBHIP_EINVAL, "orbl_fuse_targets: negative count");
  ORBHIP_REQUIRE(counts && ord_off && kf_fuse_target && (nord == 0 || ord_kf) && (cap_tgt == 0 || tgt_kf), ORBHIP_EINVAL, "orbl_fuse_targets: NULL argument");
  const void* words[] = {ord_off, ord_kf, kf_fuse_target, tgt_kf, counts, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_fuse_targets: 32-bit arrays must be 4-byte aligned");
  SnTgtArgs A;
  A.cur_kf = cur_kf; A.cur_id = cur_id; A.nkf = nkf; A.nord = nord; A.nn = nn; A.nn2 = nn2; A.cap = cap_tgt;
  A.kf_bad = kf_bad; A.ord_off = ord_off; A.ord_kf = ord_kf; A.stamp = kf_fuse_target; A.tgt = tgt_kf; A.counts = counts; A.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  hipLaunchKernelGGL(k_sn_targets, dim3(1), dim3(64), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_fuse_targets(int cur_kf, int cur_id, int nkf, const uint8_t* kf_bad, const int32_t* ord_off, const int32_t* ord_kf, int32_t* kf_fuse_target, int nn, int nn2,
                      int cap_tgt, int32_t* tgt_kf, int32_t* counts) {
  using namespace orbhip;
  static const char E[] = "orbl_fuse_targets";
  ORBHIP_REQUIRE(nkf >= 0 && nn >= 0 && nn2 >= 0 && cap_tgt >= 0, ORBHIP_EINVAL, "orbl_fuse_targets: negative count");
  ORBHIP_REQUIRE(cur_kf >= 0 && cur_kf < nkf, ORBHIP_EINVAL, "orbl_fuse_targets: cur_kf is out of range");
  ORBHIP_REQUIRE(counts && ord_off && kf_fuse_target && (cap_tgt == 0 || tgt_kf), ORBHIP_EINVAL, "orbl_fuse_targets: NULL argument");
  int nord = 0;
  ORBHIP_ARG(check_csr(E, "ord_off", ord_off, nkf, &nord));
  ORBHIP_REQUIRE(nord == 0 || ord_kf, ORBHIP_EINVAL, "orbl_fuse_targets: NULL ord_kf");
  ORBHIP_ARG(check_index(E, "ord_kf", ord_kf, nord, nkf));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf;
  RoundTrip R(W);
  const HostIn<uint8_t> d_bad = R.in(kf_bad, nk);
  const HostIn<int32_t> d_off = R.csr(ord_off, nk), d_kf = R.in(ord_kf, (size_t)nord);
  const HostOut<int32_t> io_stamp = R.inout(kf_fuse_target, nk), o_tgt = R.out<int32_t>((size_t)cap_tgt), o_counts = R.out<int32_t>(2);
  const HostOut<uint32_t> o_bits = R.out<uint32_t>(1);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_fuse_targets_device(cur_kf, cur_id, nkf, d_bad.dev(), nord, d_off.dev(), d_kf.dev(), io_stamp.dev(), nn, nn2, cap_tgt, o_tgt.dev(), o_counts.dev(),
                                     o_bits.dev(), nullptr, R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 2);
  if (o_counts[0] > cap_tgt) {
    set_error("orbl_fuse_targets: wanted %d targets; capacity %d", o_counts[0], cap_tgt);
    return ORBHIP_ECAP;
  }
  R.copy_out(io_stamp, kf_fuse_target, nk); R.copy_out(o_tgt, tgt_kf, (size_t)o_counts[0]);
  return 0;
}

// ================================================================================================================== orbl_fuse_rows
int orbl_fuse_rows_workspace(int n, size_t* bytes) {
  ORBHIP_REQUIRE(n >= 0 && bytes, ORBHIP_EINVAL, "orbl_fuse_rows_workspace: bad argument");
  *bytes = 0;                                                             // (a wave scans the keyframe's slots: no grid, no scratch)
  return 0;
}

int orbl_fuse_rows_device(const int32_t* d_kf, int n, const int32_t* pts, int nkf, const double* kf_Tcw, const double* kf_center, const float* kf_K4,
                          const float* kf_bounds, const int32_t* kf_slot_off, int nslots, const float* kf_slot_uv, const int32_t* kf_slot_level,
                          const uint8_t* kf_slot_desc, int npts, const double* pt_Xw, const double* pt_normal, const float* pt_min_dist, const float* pt_max_dist,
                          const uint8_t* pt_desc, const float* scale_factors, const float* inv_level_sigma2, float log_scale_factor, int n_levels, float th,
                          int32_t* op_kind, int32_t* op_pt, int32_t* op_arg, int32_t* op_kf, int32_t* op_slot, int32_t* best_idx, int32_t* best_dist, float* q_uv,
                          int32_t* q_level, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  (void)workspace;
  ORBHIP_REQUIRE(n >= 0 && nkf >= 0 && nslots >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_fuse_rows: negative count");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_fuse_rows: n_levels out of range");
  ORBHIP_REQUIRE(log_scale_factor > 0.f && th > 0.f, ORBHIP_EINVAL, "orbl_fuse_rows: log_scale_factor and th must be positive");
  ORBHIP_REQUIRE(d_kf && kf_slot_off && scale_factors && inv_level_sigma2, ORBHIP_EINVAL, "orbl_fuse_rows: NULL keyframe index, offsets or level table");
  ORBHIP_REQUIRE(n == 0 || (pts && op_kind && op_pt && op_arg && op_kf && op_slot), ORBHIP_EINVAL, "orbl_fuse_rows: NULL point list or row output");
  ORBHIP_REQUIRE(nkf == 0 || (kf_Tcw && kf_center && kf_K4 && kf_bounds), ORBHIP_EINVAL, "orbl_fuse_rows: NULL keyframe table");
  ORBHIP_REQUIRE(nslots == 0 || (kf_slot_uv && kf_slot_level && kf_slot_desc), ORBHIP_EINVAL, "orbl_fuse_rows: NULL slot table");
  ORBHIP_REQUIRE(npts == 0 || (pt_Xw && pt_normal && pt_min_dist && pt_max_dist && pt_desc), ORBHIP_EINVAL, "orbl_fuse_rows: NULL point table");
  const void* words[] = {d_kf, pts, kf_K4, kf_bounds, kf_slot_off, kf_slot_uv, kf_slot_level, kf_slot_desc, pt_min_dist, pt_max_dist, pt_desc, scale_factors,
                         inv_level_sigma2, op_kind, op_pt, op_arg, op_kf, op_slot, best_idx, best_dist, q_uv, q_level, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_fuse_rows: 32-bit arrays and descriptor tables must be 4-byte aligned");
  const void* dwords[] = {kf_Tcw, kf_center, pt_Xw, pt_normal};
  for (const void* q : dwords) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_fuse_rows: 64-bit arrays must be 8-byte aligned");
  SnRowArgs A;
  A.n = n; A.nkf = nkf; A.nslots = nslots; A.npts = npts; A.n_levels = n_levels; A.log_scale = log_scale_factor; A.th = th;
  A.d_kf = d_kf; A.pts = pts; A.kf_Tcw = kf_Tcw; A.kf_center = kf_center; A.kf_K4 = kf_K4; A.kf_bounds = kf_bounds; A.slot_off = kf_slot_off; A.slot_uv = kf_slot_uv;
  A.slot_level = kf_slot_level; A.slot_desc = (const uint32_t*)kf_slot_desc; A.pt_Xw = pt_Xw; A.pt_normal = pt_normal; A.pt_min = pt_min_dist; A.pt_max = pt_max_dist;
  A.pt_desc = (const uint32_t*)pt_desc; A.scale_factors = scale_factors; A.inv_sigma2 = inv_level_sigma2;
  A.op_kind = op_kind; A.op_pt = op_pt; A.op_arg = op_arg; A.op_kf = op_kf; A.op_slot = op_slot; A.best_idx = best_idx; A.best_dist = best_dist; A.q_uv = q_uv;
  A.q_level = q_level; A.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  if (n > 0) hipLaunchKernelGGL(k_sn_rows, dim3((n + SN_WG / 64 - 1) / (SN_WG / 64)), dim3(SN_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_fuse_rows(int kf, int n, const int32_t* pts, int nkf, const double* kf_Tcw, const double* kf_center, const float* kf_K4, const float* kf_bounds,
                   const int32_t* kf_slot_off, const float* kf_slot_uv, const int32_t* kf_slot_level, const uint8_t* kf_slot_desc, int npts, const double* pt_Xw,
                   const double* pt_normal, const float* pt_min_dist, const float* pt_max_dist, const uint8_t* pt_desc, const float* scale_factors,
                   const float* inv_level_sigma2, float log_scale_factor, int n_levels, float th, int32_t* op_kind, int32_t* op_pt, int32_t* op_arg, int32_t* op_kf,
                   int32_t* op_slot, int32_t* best_idx, int32_t* best_dist, float* q_uv, int32_t* q_level) {
  using namespace orbhip;
  static const char E[] = "orbl_fuse_rows";
  ORBHIP_REQUIRE(n >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_fuse_rows: negative count");
  ORBHIP_REQUIRE(kf >= 0 && kf < nkf, ORBHIP_EINVAL, "orbl_fuse_rows: kf is out of range");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_fuse_rows: n_levels out of range");
  ORBHIP_REQUIRE(log_scale_factor > 0.f && th > 0.f, ORBHIP_EINVAL, "orbl_fuse_rows: log_scale_factor and th must be positive");
  ORBHIP_REQUIRE(kf_slot_off && scale_factors && inv_level_sigma2 && kf_Tcw && kf_center && kf_K4 && kf_bounds, ORBHIP_EINVAL, "orbl_fuse_rows: NULL keyframe table");
  ORBHIP_REQUIRE(n == 0 || (pts && op_kind && op_pt && op_arg && op_kf && op_slot), ORBHIP_EINVAL, "orbl_fuse_rows: NULL point list or row output");
  ORBHIP_REQUIRE(npts == 0 || (pt_Xw && pt_normal && pt_min_dist && pt_max_dist && pt_desc), ORBHIP_EINVAL, "orbl_fuse_rows: NULL point table");
  int nslots = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_REQUIRE(nslots == 0 || (kf_slot_uv && kf_slot_level && kf_slot_desc), ORBHIP_EINVAL, "orbl_fuse_rows: NULL slot table");
  ORBHIP_ARG(check_index(E, "pts", pts, n, npts, true));
  ORBHIP_ARG(check_index(E, "kf_slot_level", kf_slot_level + kf_slot_off[kf], kf_slot_off[kf + 1] - kf_slot_off[kf], n_levels));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nn = (size_t)n, nk = (size_t)nkf, ns = (size_t)nslots, np = (size_t)npts, nl = (size_t)n_levels;
  const int32_t kf_word = kf;
  RoundTrip R(W);
  const HostIn<int32_t> d_kf = R.in(&kf_word, 1), d_pts = R.in(pts, nn), d_off = R.csr(kf_slot_off, nk), d_lvl = R.in(kf_slot_level, ns);
  const HostIn<double> d_T = R.in(kf_Tcw, 12 * nk), d_ctr = R.in(kf_center, 3 * nk), d_X = R.in(pt_Xw, 3 * np), d_nrm = R.in(pt_normal, 3 * np);
  const HostIn<float> d_K4 = R.in(kf_K4, 4 * nk), d_bnd = R.in(kf_bounds, 4 * nk), d_uv = R.in(kf_slot_uv, 2 * ns), d_min = R.in(pt_min_dist, np), d_max = R.in(pt_max_dist, np);
  const HostIn<float> d_sf = R.in(scale_factors, nl), d_is2 = R.in(inv_level_sigma2, nl);
  const HostIn<uint8_t> d_sdesc = R.in(kf_slot_desc, 32 * ns), d_pdesc = R.in(pt_desc, 32 * np);
  const HostOut<int32_t> o_kind = R.out<int32_t>(nn), o_pt = R.out<int32_t>(nn), o_arg = R.out<int32_t>(nn), o_kf = R.out<int32_t>(nn), o_slot = R.out<int32_t>(nn);
  const HostOut<int32_t> o_bi = R.out<int32_t>(nn, best_idx != nullptr), o_bd = R.out<int32_t>(nn, best_dist != nullptr), o_ql = R.out<int32_t>(nn, q_level != nullptr);
  const HostOut<float> o_quv = R.out<float>(2 * nn, q_uv != nullptr);
  const HostOut<uint32_t> o_bits = R.out<uint32_t>(1);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_fuse_rows_device(d_kf.dev(), n, d_pts.dev(), nkf, d_T.dev(), d_ctr.dev(), d_K4.dev(), d_bnd.dev(), d_off.dev(), nslots, d_uv.dev(), d_lvl.dev(),
                                  d_sdesc.dev(), npts, d_X.dev(), d_nrm.dev(), d_min.dev(), d_max.dev(), d_pdesc.dev(), d_sf.dev(), d_is2.dev(), log_scale_factor, n_levels,
                                  th, o_kind.dev(), o_pt.dev(), o_arg.dev(), o_kf.dev(), o_slot.dev(), o_bi.dev(), o_bd.dev(), o_quv.dev(), o_ql.dev(), o_bits.dev(),
                                  nullptr, R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_kind, op_kind, nn); R.copy_out(o_pt, op_pt, nn); R.copy_out(o_arg, op_arg, nn); R.copy_out(o_kf, op_kf, nn); R.copy_out(o_slot, op_slot, nn);
  R.copy_out(o_bi, best_idx, nn); R.copy_out(o_bd, best_dist, nn); R.copy_out(o_ql, q_level, nn); R.copy_out(o_quv, q_uv, 2 * nn);
  return 0;
}

// ================================================================================================================== orbl_fuse_candidates
int orbl_fuse_candidates_workspace(int n_tgt, int npts, size_t* bytes) {
  ORBHIP_REQUIRE(n_tgt >= 0 && npts >= 0 && bytes, ORBHIP_EINVAL, "orbl_fuse_candidates_workspace: bad argument");
  *bytes = orbhip::sn_cand_workspace(n_tgt, npts).total;
  return 0;
}

int orbl_fuse_candidates_device(int n_tgt, const int32_t* tgt_kf, int nkf, const int32_t* kf_slot_off, int nslots, const int32_t* kf_slot_pt, int npts,
                                const uint8_t* pt_bad, int32_t* pt_fuse_cand, int cur_id, int cap_cand, int32_t* cand_pt, int32_t* counts, uint32_t* status,
                                void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(n_tgt >= 0 && nkf >= 0 && nslots >= 0 && npts >= 0 && cap_cand >= 0, ORBHIP_EINVAL, "orbl_fuse_candidates: negative count");
  ORBHIP_REQUIRE(n_tgt <= (1 << 24), ORBHIP_EINVAL, "orbl_fuse_candidates: more than 2^24 targets");
  ORBHIP_REQUIRE(workspace && counts && kf_slot_off, ORBHIP_EINVAL, "orbl_fuse_candidates: NULL workspace, counts or offsets");
  ORBHIP_REQUIRE((n_tgt == 0 || tgt_kf) && (nslots == 0 || kf_slot_pt) && (npts == 0 || (pt_bad && pt_fuse_cand)) && (cap_cand == 0 || cand_pt), ORBHIP_EINVAL,
                 "orbl_fuse_candidates: NULL argument");
  const void* words[] = {tgt_kf, kf_slot_off, kf_slot_pt, pt_fuse_cand, cand_pt, counts, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_fuse_candidates: 32-bit arrays must be 4-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)workspace % 8 == 0, ORBHIP_EINVAL, "orbl_fuse_candidates: the workspace must be 8-byte aligned");
  const SnCandWs ws = sn_cand_workspace(n_tgt, npts);
  uint8_t* wb = (uint8_t*)workspace;
  SnCandArgs A;
  A.n_tgt = n_tgt; A.nkf = nkf; A.nslots = nslots; A.npts = npts; A.cur_id = cur_id; A.cap = cap_cand;
  A.tgt = tgt_kf; A.slot_off = kf_slot_off; A.slot_pt = kf_slot_pt; A.pt_bad = pt_bad; A.stamp = pt_fuse_cand; A.cand = cand_pt; A.counts = counts; A.status = status;
  A.first = (unsigned long long*)(wb + ws.first); A.tcnt = (int32_t*)(wb + ws.tcnt);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  if (npts > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.first, 0xFF, 8 * (size_t)npts, st));
  if (n_tgt > 0) {
    hipLaunchKernelGGL(k_sn_cand_mark, dim3(n_tgt * SN_CAND_BX), dim3(SN_WG), 0, st, A);
    hipLaunchKernelGGL(k_sn_cand_scan<false>, dim3(n_tgt), dim3(SN_WG), 0, st, A);
  }
  hipLaunchKernelGGL(k_mt_scan_sums<int32_t>, dim3(1), dim3(MT_SUM_WG), 0, st, A.tcnt, n_tgt);
  hipLaunchKernelGGL(k_sn_cand_scan<true>, dim3(n_tgt + 1), dim3(SN_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_fuse_candidates(int n_tgt, const int32_t* tgt_kf, int nkf, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const uint8_t* pt_bad,
                         int32_t* pt_fuse_cand, int cur_id, int cap_cand, int32_t* cand_pt, int32_t* counts) {
  using namespace orbhip;
  static const char E[] = "orbl_fuse_candidates";
  ORBHIP_REQUIRE(n_tgt >= 0 && nkf >= 0 && npts >= 0 && cap_cand >= 0, ORBHIP_EINVAL, "orbl_fuse_candidates: negative count");
  ORBHIP_REQUIRE(n_tgt <= (1 << 24), ORBHIP_EINVAL, "orbl_fuse_candidates: more than 2^24 targets");
  ORBHIP_REQUIRE(counts && (nkf == 0 || kf_slot_off) && (n_tgt == 0 || tgt_kf) && (npts == 0 || (pt_bad && pt_fuse_cand)) && (cap_cand == 0 || cand_pt), ORBHIP_EINVAL,
                 "orbl_fuse_candidates: NULL argument");
  int nslots = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_REQUIRE(nslots == 0 || kf_slot_pt, ORBHIP_EINVAL, "orbl_fuse_candidates: NULL kf_slot_pt");
  ORBHIP_ARG(check_index(E, "tgt_kf", tgt_kf, n_tgt, nkf));
  ORBHIP_ARG(check_index(E, "kf_slot_pt", kf_slot_pt, nslots, npts, true));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nt = (size_t)n_tgt, nk = (size_t)nkf, np = (size_t)npts, cap = (size_t)cap_cand;
  RoundTrip R(W);
  const HostIn<int32_t> d_tgt = R.in(tgt_kf, nt), d_off = R.csr(kf_slot_off ? kf_slot_off : &R.zero, nk), d_spt = R.in(kf_slot_pt, (size_t)nslots);
  const HostIn<uint8_t> d_bad = R.in(pt_bad, np);
  const HostOut<int32_t> io_stamp = R.inout(pt_fuse_cand, np), o_cand = R.out<int32_t>(cap), o_counts = R.out<int32_t>(2);
  const HostOut<uint32_t> o_bits = R.out<uint32_t>(1);
  R.scratch(sn_cand_workspace(n_tgt, npts).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_fuse_candidates_device(n_tgt, d_tgt.dev(), nkf, d_off.dev(), nslots, d_spt.dev(), npts, d_bad.dev(), io_stamp.dev(), cur_id, cap_cand, o_cand.dev(),
                                        o_counts.dev(), o_bits.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 2);
  if (o_counts[0] > cap_cand) {
    set_error("orbl_fuse_candidates: wanted %d candidates; capacity %d", o_counts[0], cap_cand);
    return ORBHIP_ECAP;
  }
  R.copy_out(io_stamp, pt_fuse_cand, np); R.copy_out(o_cand, cand_pt, (size_t)o_counts[0]);
  return 0;
}

// ================================================================================================================== orbl_update_map_points_on_tables
int orbl_update_map_points_on_tables_workspace(int npts, int nobs, size_t* bytes) {
  ORBHIP_REQUIRE(npts >= 0 && nobs >= 0 && bytes, ORBHIP_EINVAL, "orbl_update_map_points_on_tables_workspace: bad argument");
  *bytes = orbhip::sn_upd_workspace(npts, nobs).total;
  return 0;
}

int orbl_update_map_points_on_tables_device(int what, const uint8_t* pt_mask, int mask_kf, int nkf, const uint8_t* kf_bad, const double* kf_center,
                                            const int32_t* kf_slot_off, int nslots, const int32_t* kf_slot_pt, const int32_t* kf_slot_level,
                                            const uint8_t* kf_slot_desc, int npts, const uint8_t* pt_bad, const double* pt_Xw, const int32_t* pt_ref_kf, int nobs,
                                            const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot, const float* scale_factors, int n_levels,
                                            uint8_t* pt_desc, double* pt_normal, float* pt_min_dist, float* pt_max_dist, int32_t* best_obs, uint8_t* nd_written,
                                            uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  static const char M[] = "orbl_update_map_points_on_tables: NULL argument";
  ORBHIP_REQUIRE(nkf >= 0 && nslots >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: negative count");
  ORBHIP_REQUIRE(what >= 1 && what <= (ORBL_MP_DESC | ORBL_MP_NORMAL_DEPTH), ORBHIP_EINVAL, "orbl_update_map_points_on_tables: `what` selects nothing known");
  ORBHIP_REQUIRE(mask_kf >= -1 && mask_kf < nkf, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: mask_kf is neither -1 nor a keyframe");
  ORBHIP_REQUIRE(pt_mask || mask_kf >= 0, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: neither pt_mask nor mask_kf selects a point");
  const bool desc = what & ORBL_MP_DESC, nd = what & ORBL_MP_NORMAL_DEPTH;
  ORBHIP_REQUIRE(workspace && obs_off && kf_slot_off, ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE((npts == 0 || pt_bad) && (nobs == 0 || (obs_kf && obs_slot)) && (nslots == 0 || kf_slot_desc) && (mask_kf < 0 || nslots == 0 || kf_slot_pt),
                 ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(!desc || npts == 0 || pt_desc, ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(!nd || ((npts == 0 || (pt_Xw && pt_ref_kf && pt_normal && pt_min_dist && pt_max_dist)) && (nkf == 0 || kf_center) && (nslots == 0 || kf_slot_level) &&
                         scale_factors),
                 ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_update_map_points_on_tables: n_levels out of range");
  const void* words[] = {kf_slot_off, kf_slot_pt, kf_slot_level, kf_slot_desc, pt_ref_kf, obs_off, obs_kf, obs_slot, scale_factors, pt_desc, pt_min_dist, pt_max_dist,
                         best_obs, status};
  for (const void* q : words)
    ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: 32-bit arrays and descriptor tables must be 4-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)workspace % 16 == 0, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  if (npts == 0) return 0;
  const SnUpdWs ws = sn_upd_workspace(npts, nobs);
  uint8_t* wb = (uint8_t*)workspace;
  SnUpdArgs U; std::memset(&U, 0, sizeof(U));
  U.npts = npts; U.nkf = nkf; U.nslots = nslots; U.nobs = nobs; U.mask_kf = mask_kf;
  U.pt_mask = pt_mask; U.pt_bad = pt_bad; U.kf_bad = kf_bad; U.obs_off = obs_off; U.obs_kf = obs_kf; U.obs_slot = obs_slot; U.slot_off = kf_slot_off; U.slot_pt = kf_slot_pt;
  U.slot_level = kf_slot_level; U.pt_ref_kf = pt_ref_kf; U.slot_desc = (const uint32_t*)kf_slot_desc;
  U.sel = wb + ws.sel; U.good = wb + ws.good; U.obs_good = wb + ws.obs_good; U.ref_level = (int32_t*)(wb + ws.ref_level); U.obs_desc = (uint32_t*)(wb + ws.obs_desc);
  U.status = status;
  uint8_t* wrote = nd_written ? nd_written : wb + ws.nd_written;
  U.nd_written = wrote; U.min_max = (const float*)(wb + ws.min_max); U.pt_min = pt_min_dist; U.pt_max = pt_max_dist;
  MpArgs A;
  A.npts = npts; A.nobs = nobs; A.nkf = nkf; A.n_levels = n_levels; A.what = what;
  A.obs_off = obs_off; A.X = pt_Xw; A.ref_kf = pt_ref_kf; A.ref_level = U.ref_level; A.pt_good = U.good;
  A.obs_kf = obs_kf; A.obs_desc = U.obs_desc; A.obs_good = U.obs_good; A.kf_center = kf_center; A.scale_factors = scale_factors;
  A.best_obs = best_obs ? best_obs : (int32_t*)(wb + ws.best_obs); A.desc_out = (uint32_t*)pt_desc; A.normal = pt_normal; A.min_max = (float*)(wb + ws.min_max);
  A.nd_written = wrote;
  A.cnt = (uint32_t*)(wb + ws.mp); A.list = A.cnt + 8;
  const int nb = (npts + SN_WG - 1) / SN_WG;
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0, ws.cleared, st));
  if (desc) ORBHIP_CHECK_HIP(hipMemsetAsync(A.cnt, 0, 32, st));
  if (mask_kf >= 0) hipLaunchKernelGGL(k_sn_mask_kf, dim3(SN_CAND_BX), dim3(SN_WG), 0, st, U);
  hipLaunchKernelGGL(k_sn_gather, dim3((int)(((size_t)npts * 8 + SN_WG - 1) / SN_WG)), dim3(SN_WG), 0, st, U);
  hipLaunchKernelGGL(k_mp_prep, dim3((npts + MP_WG - 1) / MP_WG), dim3(MP_WG), 0, st, A);
  if (desc) hipLaunchKernelGGL(k_mp_desc, dim3(std::min(npts, 2048)), dim3(MP_WG), 0, st, A);
  if (nd) hipLaunchKernelGGL(k_sn_scatter, dim3(nb), dim3(SN_WG), 0, st, U);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_update_map_points_on_tables(int what, const uint8_t* pt_mask, int mask_kf, int nkf, const uint8_t* kf_bad, const double* kf_center, const int32_t* kf_slot_off,
                                     const int32_t* kf_slot_pt, const int32_t* kf_slot_level, const uint8_t* kf_slot_desc, int npts, const uint8_t* pt_bad,
                                     const double* pt_Xw, const int32_t* pt_ref_kf, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot,
                                     const float* scale_factors, int n_levels, uint8_t* pt_desc, double* pt_normal, float* pt_min_dist, float* pt_max_dist,
                                     int32_t* best_obs, uint8_t* nd_written) {
  using namespace orbhip;
  static const char E[] = "orbl_update_map_points_on_tables";
  static const char M[] = "orbl_update_map_points_on_tables: NULL argument";
  ORBHIP_REQUIRE(nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: negative count");
  ORBHIP_REQUIRE(what >= 1 && what <= (ORBL_MP_DESC | ORBL_MP_NORMAL_DEPTH), ORBHIP_EINVAL, "orbl_update_map_points_on_tables: `what` selects nothing known");
  ORBHIP_REQUIRE(mask_kf >= -1 && mask_kf < nkf, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: mask_kf is neither -1 nor a keyframe");
  ORBHIP_REQUIRE(pt_mask || mask_kf >= 0, ORBHIP_EINVAL, "orbl_update_map_points_on_tables: neither pt_mask nor mask_kf selects a point");
  const bool desc = what & ORBL_MP_DESC, nd = what & ORBL_MP_NORMAL_DEPTH;
  ORBHIP_REQUIRE((nkf == 0 || kf_slot_off) && (npts == 0 || (obs_off && pt_bad)), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(!desc || npts == 0 || pt_desc, ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(!nd || ((npts == 0 || (pt_Xw && pt_ref_kf && pt_normal && pt_min_dist && pt_max_dist)) && (nkf == 0 || kf_center) && scale_factors), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_update_map_points_on_tables: n_levels out of range");
  int nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE((nobs == 0 || (obs_kf && obs_slot)) && (nslots == 0 || (kf_slot_desc && (mask_kf < 0 || kf_slot_pt) && (!nd || kf_slot_level))), ORBHIP_EINVAL, M);
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  for (int e = 0; e < nobs; e++)
    ORBHIP_REQUIRE(obs_slot[e] >= 0 && obs_slot[e] < kf_slot_off[obs_kf[e] + 1] - kf_slot_off[obs_kf[e]], ORBHIP_EINVAL,
                   "orbl_update_map_points_on_tables: an obs_slot lies outside its keyframe's slots");
  if (mask_kf >= 0) ORBHIP_ARG(check_index(E, "kf_slot_pt", kf_slot_pt + kf_slot_off[mask_kf], kf_slot_off[mask_kf + 1] - kf_slot_off[mask_kf], npts, true));
  if (nd) {
    ORBHIP_ARG(check_index(E, "pt_ref_kf", pt_ref_kf, npts, nkf, true));
    ORBHIP_ARG(check_index(E, "kf_slot_level", kf_slot_level, nslots, n_levels));
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nk = (size_t)nkf, ns = (size_t)nslots, np = (size_t)npts, no = (size_t)nobs;
  RoundTrip R(W);
  const HostIn<uint8_t> d_mask = R.in(pt_mask, np), d_kbad = R.in(kf_bad, nk), d_sdesc = R.in(kf_slot_desc, 32 * ns), d_pbad = R.in(pt_bad, np);
  const HostIn<double> d_ctr = R.in(nd ? kf_center : nullptr, 3 * nk), d_X = R.in(nd ? pt_Xw : nullptr, 3 * np);
  const HostIn<int32_t> d_soff = R.csr(kf_slot_off ? kf_slot_off : &R.zero, nk), d_spt = R.in(mask_kf >= 0 ? kf_slot_pt : nullptr, ns), d_lvl = R.in(nd ? kf_slot_level : nullptr, ns);
  const HostIn<int32_t> d_ref = R.in(nd ? pt_ref_kf : nullptr, np), d_off = R.csr(obs_off ? obs_off : &R.zero, np), d_okf = R.in(obs_kf, no), d_oslot = R.in(obs_slot, no);
  const HostIn<float> d_sf = R.in(nd ? scale_factors : nullptr, (size_t)n_levels);
  const HostOut<uint8_t> io_desc = R.inout(desc ? pt_desc : nullptr, 32 * np), o_wrote = R.out<uint8_t>(np, nd_written != nullptr);
  const HostOut<double> io_nrm = R.inout(nd ? pt_normal : nullptr, 3 * np);
  const HostOut<float> io_min = R.inout(nd ? pt_min_dist : nullptr, np), io_max = R.inout(nd ? pt_max_dist : nullptr, np);
  const HostOut<int32_t> o_best = R.out<int32_t>(np, best_obs != nullptr);
  const HostOut<uint32_t> o_bits = R.out<uint32_t>(1);
  R.scratch(sn_upd_workspace(npts, nobs).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_update_map_points_on_tables_device(what, d_mask.dev(), mask_kf, nkf, d_kbad.dev(), d_ctr.dev(), d_soff.dev(), nslots, d_spt.dev(), d_lvl.dev(),
                                                    d_sdesc.dev(), npts, d_pbad.dev(), d_X.dev(), d_ref.dev(), nobs, d_off.dev(), d_okf.dev(), d_oslot.dev(), d_sf.dev(),
                                                    n_levels, io_desc.dev(), io_nrm.dev(), io_min.dev(), io_max.dev(), o_best.dev(), o_wrote.dev(), o_bits.dev(),
                                                    R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(io_desc, pt_desc, 32 * np); R.copy_out(io_nrm, pt_normal, 3 * np); R.copy_out(io_min, pt_min_dist, np); R.copy_out(io_max, pt_max_dist, np);
  R.copy_out(o_best, best_obs, np); R.copy_out(o_wrote, nd_written, np);
  return 0;
}

}  // extern "C"
