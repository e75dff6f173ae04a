// orb_mapedit.inc -- an ordered list of map-point edits replayed on the map tables (orbl_apply_map_edits*): MapPoint::AddObservation,
// Replace and SetBadFlag (src/MapPoint.cc:133-138, :199-233, :174-191, monocular) as LocalMapping::ProcessNewKeyFrame / CreateNewMapPoints /
// MapPointCulling, ORBmatcher::Fuse (both forms) and LoopClosing::CorrectLoop / SearchAndFuse call them, and the rebuild of the WHOLE
// observation tables that no other entry does.  Textually included by orb_localmap.hip.
//
// This is the plain ordered replay (DESIGN.md section 2, "Map-point edits on the tables"): ONE wave walks the edit list in call order.
// The observation lists are never copied while it runs.  A point's list is its input row - until the point is EMPTIED (Replace takes a
// list whole, SetBadFlag clears it whole: a list grows or vanishes, it never loses a single entry) - plus a chain of the entries it
// received: head[p], next[entry].  An entry is an input observation e, or nobs + i for the one observation op i can create; a moved entry
// keeps its number, which is what oobs_src reports.  Every lane of the wave runs the same control flow on the same values and stores the
// same values, so a lane reads back its OWN stores and no fence is needed; only the scan of an input row (immutable) is split over the lanes.
// This rests on the mutated arrays being read with VECTOR loads, which the compiler emits because the MeArgs pointers may alias a store of
// the kernel: keep them free of __restrict__ and of const-noalias promises, or a uniform load could move to the scalar cache, which is
// not coherent with the vector stores.
// Launches, on one stream after the workspace is cleared, whatever the data:
//   k_me_init    one lane per observation / point / keyframe: which input observations are there (not dead, keyframe and slot in range),
//                the offset and rank checks, pt_touched = 0.
//   k_me_replay  ONE wave: the edits in order; op_status, op_found, the in/out tables, counts[1..4].
//   k_me_count   one lane per point: the length of its new list; a workgroup scan (mt_block_excl), n_touched and n_late_adds.
//   k_mt_scan_sums  the workgroup sums.
//   k_me_emit    one wave per point: its entries gathered (row by ballot prefix, chain by lane 0) and placed by COUNTING the smaller
//                kf_rank - the ranks inside a list are distinct; a last workgroup writes oobs_off[npts], counts[0, 5, 6, 7], the capacity bit.
// Outputs are written with vector stores only; no atomic decides a position; nothing is written beyond a count or a capacity.
#include "orb_maptable.h"

namespace orbhip {

#define ME_WG 256                 /* k_me_init, k_me_count */
#define ME_WAVE 64                /* k_me_replay, k_me_emit: one wave */
#define ME_ST_OFFSETS 1u          /* *status bits of the device form */
#define ME_ST_KF 2u
#define ME_ST_PT 4u
#define ME_ST_SLOT 8u
#define ME_ST_CAP 16u

struct MeArgs {
  int nops, nkf, npts, nslots, nobs, cap_obs;
  const int32_t *slot_off, *kf_rank, *obs_off, *obs_kf, *obs_slot; const uint8_t* obs_dead; const int32_t* slot_level; const float* slot_uv;
  int32_t* slot_pt; uint8_t* pt_bad; int32_t *pt_nobs, *pt_found, *pt_visible, *pt_replaced;
  const int32_t *op_kind, *op_pt, *op_arg, *op_kf, *op_slot;
  int32_t *op_status, *op_found; uint8_t* pt_touched;
  int32_t *oobs_off, *oobs_kf, *oobs_slot, *oobs_src, *oobs_level; float* oobs_uv; int32_t* counts; uint32_t* status;
  // workspace.  Cleared per call: emptied[npts] | late[npts] | rhit[nkf] | ctr[2] (n_touched, n_late_adds).  Preset to -1: head[npts].
  // Then next[nobs + nops], alive[nobs], cnt[npts], excl[npts], bsum[blocks + 1], gath[nobs + nops].
  uint8_t *emptied, *late, *alive; int32_t *rhit, *ctr, *head, *next, *cnt, *excl, *bsum, *gath;
};

// the index of slot s of keyframe k in kf_slot_pt, or -1 when the keyframe has no such slot (k is in range)
__device__ __forceinline__ int me_slot_at(const MeArgs& a, int k, int s) {
  int lo, hi;
  if (!mt_range(a.slot_off, k, a.nslots, &lo, &hi) || s < 0 || s >= hi - lo) return -1;
  return lo + s;
}
__device__ __forceinline__ int me_ent_kf(const MeArgs& a, int e) { return e < a.nobs ? a.obs_kf[e] : a.op_kf[e - a.nobs]; }
__device__ __forceinline__ int me_ent_slot(const MeArgs& a, int e) { return e < a.nobs ? a.obs_slot[e] : a.op_slot[e - a.nobs]; }
__device__ __forceinline__ uint32_t me_rank(const MeArgs& a, int k) { return (uint32_t)(a.kf_rank ? a.kf_rank[k] : k); }

__global__ __launch_bounds__(ME_WG) void k_me_init(MeArgs a) {
  const int i = blockIdx.x * ME_WG + threadIdx.x;
  int lo, hi;
  if (i < a.nobs) {
    bool there = !(a.obs_dead && a.obs_dead[i]);
    if (there) {
      const int k = a.obs_kf[i];
      if (k < 0 || k >= a.nkf) { there = false; mt_flag(a.status, ME_ST_KF); }
      else if (me_slot_at(a, k, a.obs_slot[i]) < 0) { there = false; mt_flag(a.status, ME_ST_SLOT); }
    }
    a.alive[i] = there;
  }
  if (i < a.npts) {
    a.pt_touched[i] = 0;
    if (!mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, ME_ST_OFFSETS);
  }
  if (i < a.nkf) {
    if (!mt_range(a.slot_off, i, a.nslots, &lo, &hi)) mt_flag(a.status, ME_ST_OFFSETS);
    if (a.kf_rank) {
      const int r = a.kf_rank[i];
      if (r < 0 || r >= a.nkf) mt_flag(a.status, ME_ST_KF);
      else if (atomicAdd(&a.rhit[r], 1) != 0) mt_flag(a.status, ME_ST_KF);          // (not a permutation)
    }
  }
}

// ---- the replay: every function below is called by the whole wave with the same arguments
// MapPoint::IsInKeyFrame: does p's list name keyframe K.  `chain` is where the walk of p's received entries starts: head[p], or - inside a
// Replace - the head p had when the Replace began: what it received since came from ONE list, whose keyframes are distinct
__device__ __forceinline__ bool me_names(const MeArgs& a, int p, int K, int chain) {
  bool hit = false;
  if (!a.emptied[p]) {
    int lo, hi;
    mt_range(a.obs_off, p, a.nobs, &lo, &hi);
    for (int e = lo + (int)threadIdx.x; e < hi; e += ME_WAVE) hit |= a.alive[e] && a.obs_kf[e] == K;
  }
  if (__any(hit)) return true;
  for (int e = chain; e >= 0; e = a.next[e])
    if (me_ent_kf(a, e) == K) return true;
  return false;
}

// MapPoint::AddObservation (:133-138) of entry `ent`, which is at (K, s)
__device__ __forceinline__ bool me_add_observation(const MeArgs& a, int p, int K, int ent, int chain) {
  if (me_names(a, p, K, chain)) return false;
  a.next[ent] = a.head[p];
  a.head[p] = ent;
  a.pt_nobs[p] = a.pt_nobs[p] + 1;
  return true;
}

__device__ __forceinline__ void me_touch(const MeArgs& a, int p) { a.pt_touched[p] = 1; a.late[p] = 0; }

// one taken observation of Replace (:218-226)
__device__ __forceinline__ void me_replace_entry(const MeArgs& a, int b, int ent, int chain) {
  const int k = me_ent_kf(a, ent), at = me_slot_at(a, k, me_ent_slot(a, ent));
  if (me_add_observation(a, b, k, ent, chain)) a.slot_pt[at] = b;             // KeyFrame::ReplaceMapPointMatch
  else a.slot_pt[at] = -1;                                             // KeyFrame::EraseMapPointMatch
}

// p's list is taken whole; returns the chain it had and whether its input row was still part of it
__device__ __forceinline__ int me_take(const MeArgs& a, int p, bool* row) {
  const int h = a.head[p];
  *row = !a.emptied[p];
  a.emptied[p] = 1;
  a.head[p] = -1;
  a.pt_bad[p] = 1;
  return h;
}

// MapPoint::Replace (:199-233)
__device__ __forceinline__ bool me_replace(const MeArgs& a, int pa, int pb) {
  if (pa == pb) return false;
  bool row;
  const int h = me_take(a, pa, &row);
  if (a.pt_replaced) a.pt_replaced[pa] = pb;
  const int chain = a.head[pb];
  if (row) {
    int lo, hi;
    mt_range(a.obs_off, pa, a.nobs, &lo, &hi);
    for (int e = lo; e < hi; e++)
      if (a.alive[e]) me_replace_entry(a, pb, e, chain);
  }
  for (int e = h; e >= 0;) { const int nx = a.next[e]; me_replace_entry(a, pb, e, chain); e = nx; }
  if (a.pt_found) { a.pt_found[pb] = a.pt_found[pb] + a.pt_found[pa]; a.pt_visible[pb] = a.pt_visible[pb] + a.pt_visible[pa]; }
  me_touch(a, pb);                                                     // ComputeDistinctiveDescriptors (:230), left to the caller
  return true;
}

// MapPoint::SetBadFlag (:174-191)
__device__ __forceinline__ void me_set_bad(const MeArgs& a, int p) {
  bool row;
  const int h = me_take(a, p, &row);
  if (row) {
    int lo, hi;
    mt_range(a.obs_off, p, a.nobs, &lo, &hi);
    for (int e = lo; e < hi; e++)
      if (a.alive[e]) a.slot_pt[me_slot_at(a, a.obs_kf[e], a.obs_slot[e])] = -1;
  }
  for (int e = h; e >= 0; e = a.next[e]) a.slot_pt[me_slot_at(a, me_ent_kf(a, e), me_ent_slot(a, e))] = -1;
}

// AddObservation + KeyFrame::AddMapPoint of op i: 5 when the observation is new, 6 when p's list named K already
__device__ __forceinline__ int me_add(const MeArgs& a, int i, int p, int K, int at, bool touch, int* n_added) {
  const bool ok = me_add_observation(a, p, K, a.nobs + i, a.head[p]);
  a.slot_pt[at] = p;
  if (ok) { (*n_added)++; if (a.pt_touched[p]) a.late[p] = 1; }
  if (touch) me_touch(a, p);
  return ok ? 5 : 6;
}

__global__ __launch_bounds__(ME_WAVE) void k_me_replay(MeArgs a) {
  int n_added = 0, n_replace = 0, n_set_bad = 0, n_fused = 0;
  for (int i = 0; i < a.nops; i++) {
    const int kind = a.op_kind[i], p = a.op_pt[i], arg = a.op_arg[i], K = a.op_kf[i], s = a.op_slot[i];
    int st = 0, found = -1, at = -1;
    uint32_t bits = 0;
    if (kind < 0 || kind > 6) bits = ME_ST_SLOT;
    else if (kind != 0) {
      if (p < 0 || p >= a.npts) bits |= ME_ST_PT;
      if (kind == 2 && (arg < 0 || arg >= a.npts)) bits |= ME_ST_PT;
      if (kind == 1 || kind == 4 || kind == 5) {
        if (K < 0 || K >= a.nkf) bits |= ME_ST_KF;
        else if ((at = me_slot_at(a, K, s)) < 0) bits |= ME_ST_SLOT;
      }
      if (kind == 6 && (arg < 0 || arg >= i || a.op_kind[arg] != 5)) bits |= ME_ST_SLOT;
    }
    if (bits) { mt_flag(a.status, bits); st = 10; }                     // an op out of range is absent
    else if (kind == 1) st = me_add(a, i, p, K, at, (arg & 1) != 0, &n_added);
    else if (kind == 2) { const bool ran = me_replace(a, p, arg); n_replace += ran; st = ran ? 8 : 1; }
    else if (kind == 3) { me_set_bad(a, p); n_set_bad++; st = 9; }
    else if (kind == 4) {                                               // ORBmatcher::Fuse (src/ORBmatcher.cc:746, :824-838)
      if (a.pt_bad[p] || me_names(a, p, K, a.head[p])) st = 1;
      else {
        const int q = a.slot_pt[at];
        if (q < 0 || q >= a.npts) st = me_add(a, i, p, K, at, false, &n_added);
        else if (a.pt_bad[q]) st = 2;
        else {
          found = q;
          if (a.pt_nobs[q] > a.pt_nobs[p]) { n_replace += me_replace(a, p, q); st = 3; }
          else { n_replace += me_replace(a, q, p); st = 4; }
        }
      }
    } else if (kind == 5) {                                             // the Sim3 form (src/ORBmatcher.cc:941-950)
      const int q = a.slot_pt[at];
      if (q < 0 || q >= a.npts) st = me_add(a, i, p, K, at, false, &n_added);
      else if (a.pt_bad[q]) st = 2;
      else { found = q; st = 7; }
    } else if (kind == 6) {                                             // LoopClosing::SearchAndFuse (src/LoopClosing.cc:615-621)
      const int q = a.op_found[arg];
      if (q < 0) st = 1;
      else { const bool ran = me_replace(a, q, p); n_replace += ran; st = ran ? 8 : 1; }
    }
    if ((kind == 4 || kind == 5) && (st == 2 || st == 3 || st == 4 || st == 5 || st == 7)) n_fused++;
    a.op_status[i] = st;
    a.op_found[i] = found;
  }
  a.counts[1] = n_added; a.counts[2] = n_replace; a.counts[3] = n_set_bad; a.counts[4] = n_fused;
}

__global__ __launch_bounds__(ME_WG) void k_me_count(MeArgs a) {
  __shared__ int sw[ME_WG / 64];
  const int p = blockIdx.x * ME_WG + threadIdx.x;
  int n = 0, touched = 0, late = 0;
  if (p < a.npts) {
    if (!a.emptied[p]) {
      int lo, hi;
      mt_range(a.obs_off, p, a.nobs, &lo, &hi);
      for (int e = lo; e < hi; e++) n += a.alive[e];
    }
    for (int e = a.head[p]; e >= 0; e = a.next[e]) n++;
    a.cnt[p] = n;
    touched = a.pt_touched[p]; late = a.late[p];
  }
  int tot;
  const int ex = mt_block_excl<ME_WG>(n, sw, &tot);
  if (p < a.npts) a.excl[p] = ex;
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = tot;
  touched = mt_wave_sum(touched); late = mt_wave_sum(late);
  if ((threadIdx.x & 63) == 0) {                                        // (integer sums: order-free)
    if (touched) atomicAdd(&a.ctr[0], touched);
    if (late) atomicAdd(&a.ctr[1], late);
  }
}

__global__ __launch_bounds__(ME_WAVE) void k_me_emit(MeArgs a) {
  __shared__ uint32_t s_rank[ME_WAVE];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int nb = (a.npts + ME_WG - 1) / ME_WG;
  if (p == a.npts) {                                                    // the last workgroup: the totals
    if (lane == 0) {
      const int total = a.bsum[nb];
      a.oobs_off[a.npts] = total;
      a.counts[0] = total; a.counts[5] = a.ctr[0]; a.counts[6] = a.ctr[1]; a.counts[7] = 0;
      if (total > a.cap_obs) mt_flag(a.status, ME_ST_CAP);
    }
    return;
  }
  const int n = a.cnt[p], off = a.bsum[p / ME_WG] + a.excl[p];
  if (lane == 0) a.oobs_off[p] = off;
  if (n == 0 || (long long)off + n > (long long)a.nobs + a.nops) return;        // (workgroup-uniform)
  int32_t* g = a.gath + off;                                            // this workgroup's own stretch
  int run = 0;
  if (!a.emptied[p]) {
    int lo, hi;
    mt_range(a.obs_off, p, a.nobs, &lo, &hi);
    for (int eb = lo; eb < hi; eb += ME_WAVE) {
      const int e = eb + lane;
      const bool keep = e < hi && a.alive[e];
      const mt_u64 m = __ballot(keep);
      const int at = run + __popcll(m & (((mt_u64)1 << lane) - 1));
      if (keep && at < n) g[at] = e;
      run += __popcll(m);
    }
  }
  if (lane == 0)
    for (int e = a.head[p]; e >= 0 && run < n; e = a.next[e]) g[run++] = e;
  __syncthreads();                                                      // (g is read back by this workgroup only)
  for (int ib = 0; ib < n; ib += ME_WAVE) {
    const int i = ib + lane;
    const int e = i < n ? g[i] : 0;
    const int k = i < n ? me_ent_kf(a, e) : 0;
    const uint32_t r = i < n ? me_rank(a, k) : 0u;
    int pos = 0;
    for (int jb = 0; jb < n; jb += ME_WAVE) {
      __syncthreads();
      if (jb + lane < n) s_rank[lane] = me_rank(a, me_ent_kf(a, g[jb + lane]));
      __syncthreads();
      const int m = min(ME_WAVE, n - jb);
      for (int j = 0; j < m; j++) pos += s_rank[j] < r;
    }
    if (i < n && off + pos < a.cap_obs) {
      const int o = off + pos, s = me_ent_slot(a, e);
      a.oobs_kf[o] = k; a.oobs_slot[o] = s;
      if (a.oobs_src) a.oobs_src[o] = e;
      if (a.slot_level) {
        const int at = me_slot_at(a, k, s);
        a.oobs_level[o] = a.slot_level[at]; a.oobs_uv[2 * (size_t)o] = a.slot_uv[2 * (size_t)at]; a.oobs_uv[2 * (size_t)o + 1] = a.slot_uv[2 * (size_t)at + 1];
      }
    }
  }
}

// workspace sections, each rounded up to 256 bytes; [0, cleared) is zeroed and head preset to -1 by every call
struct MeWs { size_t emptied, late, rhit, ctr, cleared, head, next, alive, cnt, excl, bsum, gath, total; };
static MeWs me_workspace(int nops, int nkf, int npts, int nobs) {
  MeWs w; Carve ws;
  const size_t np = (size_t)npts, ne = (size_t)nobs + (size_t)nops, nb = (np + ME_WG - 1) / ME_WG;
  w.emptied = ws.take(np); w.late = ws.take(np); w.rhit = ws.take(4 * (size_t)nkf); w.ctr = ws.take(8);
  w.cleared = ws.total;
  w.head = ws.take(4 * np); w.next = ws.take(4 * ne); w.alive = ws.take((size_t)nobs); w.cnt = ws.take(4 * np); w.excl = ws.take(4 * np);
  w.bsum = ws.take(4 * (nb + 1)); w.gath = ws.take(4 * ne);
  w.total = ws.total;
  return w;
}

}  // namespace orbhip

extern "C" {

int orbl_apply_map_edits_workspace(int nops, int nkf, int npts, int nslots, int nobs, size_t* bytes) {
  ORBHIP_REQUIRE(nops >= 0 && nkf >= 0 && npts >= 0 && nslots >= 0 && nobs >= 0 && bytes, ORBHIP_EINVAL, "orbl_apply_map_edits_workspace: bad argument");
  *bytes = orbhip::me_workspace(nops, nkf, npts, nobs).total;
  return 0;
}

int orbl_apply_map_edits_device(int nops, const int32_t* op_kind, const int32_t* op_pt, const int32_t* op_arg, const int32_t* op_kf, const int32_t* op_slot, int nkf,
                                const int32_t* kf_slot_off, const int32_t* kf_rank, int nslots, int32_t* kf_slot_pt, const int32_t* kf_slot_level,
                                const float* kf_slot_uv, int npts, uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_found, int32_t* pt_visible, int32_t* pt_replaced,
                                int nobs, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot, const uint8_t* obs_dead, int cap_obs,
                                int32_t* op_status, int32_t* op_found, uint8_t* pt_touched, int32_t* oobs_off, int32_t* oobs_kf, int32_t* oobs_slot, int32_t* oobs_src,
                                int32_t* oobs_level, float* oobs_uv, int32_t* counts, uint32_t* status, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(nops >= 0 && nkf >= 0 && nslots >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_apply_map_edits: negative count");
  ORBHIP_REQUIRE(cap_obs >= 0, ORBHIP_EINVAL, "orbl_apply_map_edits: negative capacity");
  ORBHIP_REQUIRE(workspace && counts && oobs_off && obs_off && kf_slot_off, ORBHIP_EINVAL, "orbl_apply_map_edits: NULL workspace, counts or offsets");
  ORBHIP_REQUIRE(nops == 0 || (op_kind && op_pt && op_arg && op_kf && op_slot && op_status && op_found), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL edit array");
  ORBHIP_REQUIRE(npts == 0 || (pt_bad && pt_nobs && pt_touched), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL point table");
  ORBHIP_REQUIRE((nslots == 0 || kf_slot_pt) && (nobs == 0 || (obs_kf && obs_slot)), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL table entries");
  ORBHIP_REQUIRE((pt_found != nullptr) == (pt_visible != nullptr), ORBHIP_EINVAL, "orbl_apply_map_edits: pt_found and pt_visible are given together or not at all");
  ORBHIP_REQUIRE((kf_slot_level != nullptr) == (kf_slot_uv != nullptr), ORBHIP_EINVAL,
                 "orbl_apply_map_edits: kf_slot_level and kf_slot_uv are given together or not at all");
  ORBHIP_REQUIRE(cap_obs == 0 || (oobs_kf && oobs_slot && (!kf_slot_level || (oobs_level && oobs_uv))), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL list output");
  const void* words[] = {op_kind, op_pt, op_arg, op_kf, op_slot, kf_slot_off, kf_rank, kf_slot_pt, kf_slot_level, kf_slot_uv, pt_nobs, pt_found, pt_visible, pt_replaced,
                         obs_off, obs_kf, obs_slot, op_status, op_found, oobs_off, oobs_kf, oobs_slot, oobs_src, oobs_level, oobs_uv, counts, status, workspace};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_apply_map_edits: 32-bit arrays and the workspace must be 4-byte aligned");
  const MeWs ws = me_workspace(nops, nkf, npts, nobs);
  uint8_t* wb = (uint8_t*)workspace;
  MeArgs A; std::memset(&A, 0, sizeof(A));
  A.nops = nops; A.nkf = nkf; A.npts = npts; A.nslots = nslots; A.nobs = nobs; A.cap_obs = cap_obs;
  A.slot_off = kf_slot_off; A.kf_rank = kf_rank; A.obs_off = obs_off; A.obs_kf = obs_kf; A.obs_slot = obs_slot; A.obs_dead = obs_dead;
  A.slot_level = kf_slot_level; A.slot_uv = kf_slot_uv; A.slot_pt = kf_slot_pt; A.pt_bad = pt_bad; A.pt_nobs = pt_nobs; A.pt_found = pt_found;
  A.pt_visible = pt_visible; A.pt_replaced = pt_replaced; A.op_kind = op_kind; A.op_pt = op_pt; A.op_arg = op_arg; A.op_kf = op_kf; A.op_slot = op_slot;
  A.op_status = op_status; A.op_found = op_found; A.pt_touched = pt_touched; A.oobs_off = oobs_off; A.oobs_kf = oobs_kf; A.oobs_slot = oobs_slot;
  A.oobs_src = oobs_src; A.oobs_level = oobs_level; A.oobs_uv = oobs_uv; A.counts = counts; A.status = status;
  A.emptied = wb + ws.emptied; A.late = wb + ws.late; A.rhit = (int32_t*)(wb + ws.rhit); A.ctr = (int32_t*)(wb + ws.ctr); A.head = (int32_t*)(wb + ws.head);
  A.next = (int32_t*)(wb + ws.next); A.alive = wb + ws.alive; A.cnt = (int32_t*)(wb + ws.cnt); A.excl = (int32_t*)(wb + ws.excl);
  A.bsum = (int32_t*)(wb + ws.bsum); A.gath = (int32_t*)(wb + ws.gath);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb, 0, ws.cleared, st));
  if (npts > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.head, 0xFF, 4 * (size_t)npts, st));
  const int n_init = std::max(std::max(nobs, npts), nkf), nb = (npts + ME_WG - 1) / ME_WG;
  if (n_init > 0) hipLaunchKernelGGL(k_me_init, dim3((n_init + ME_WG - 1) / ME_WG), dim3(ME_WG), 0, st, A);
  hipLaunchKernelGGL(k_me_replay, dim3(1), dim3(ME_WAVE), 0, st, A);
  if (nb > 0) hipLaunchKernelGGL(k_me_count, dim3(nb), dim3(ME_WG), 0, st, A);
  hipLaunchKernelGGL(k_mt_scan_sums<int32_t>, dim3(1), dim3(MT_SUM_WG), 0, st, A.bsum, nb);
  hipLaunchKernelGGL(k_me_emit, dim3(npts + 1), dim3(ME_WAVE), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_apply_map_edits(int nops, const int32_t* op_kind, const int32_t* op_pt, const int32_t* op_arg, const int32_t* op_kf, const int32_t* op_slot, int nkf,
                         const int32_t* kf_slot_off, const int32_t* kf_rank, int32_t* kf_slot_pt, const int32_t* kf_slot_level, const float* kf_slot_uv, int npts,
                         uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_found, int32_t* pt_visible, int32_t* pt_replaced, const int32_t* obs_off,
                         const int32_t* obs_kf, const int32_t* obs_slot, const uint8_t* obs_dead, int cap_obs, int32_t* op_status, int32_t* op_found,
                         uint8_t* pt_touched, int32_t* oobs_off, int32_t* oobs_kf, int32_t* oobs_slot, int32_t* oobs_src, int32_t* oobs_level, float* oobs_uv,
                         int32_t* counts) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  static const char E[] = "orbl_apply_map_edits";
  ORBHIP_REQUIRE(nops >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_apply_map_edits: negative count");
  ORBHIP_REQUIRE(cap_obs >= 0, ORBHIP_EINVAL, "orbl_apply_map_edits: negative capacity");
  ORBHIP_REQUIRE(counts && oobs_off, ORBHIP_EINVAL, "orbl_apply_map_edits: NULL counts or offset output");
  ORBHIP_REQUIRE(nops == 0 || (op_kind && op_pt && op_arg && op_kf && op_slot && op_status && op_found), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL edit array");
  ORBHIP_REQUIRE(nkf == 0 || kf_slot_off, ORBHIP_EINVAL, "orbl_apply_map_edits: NULL kf_slot_off");
  ORBHIP_REQUIRE(npts == 0 || (obs_off && pt_bad && pt_nobs && pt_touched), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL point table");
  ORBHIP_REQUIRE((pt_found != nullptr) == (pt_visible != nullptr), ORBHIP_EINVAL, "orbl_apply_map_edits: pt_found and pt_visible are given together or not at all");
  ORBHIP_REQUIRE((kf_slot_level != nullptr) == (kf_slot_uv != nullptr), ORBHIP_EINVAL,
                 "orbl_apply_map_edits: kf_slot_level and kf_slot_uv are given together or not at all");
  int nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE((nslots == 0 || kf_slot_pt) && (nobs == 0 || (obs_kf && obs_slot)), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL table entries");
  ORBHIP_REQUIRE(cap_obs == 0 || (oobs_kf && oobs_slot && (!kf_slot_level || (oobs_level && oobs_uv))), ORBHIP_EINVAL, "orbl_apply_map_edits: NULL list output");
  if (kf_rank) ORBHIP_ARG(check_permutation(E, "kf_rank", kf_rank, nkf));
  ORBHIP_ARG(check_index(E, "kf_slot_pt", kf_slot_pt, nslots, npts, true));
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  if (pt_replaced) ORBHIP_ARG(check_index(E, "pt_replaced", pt_replaced, npts, npts, true));
  {
    std::vector<int32_t> seen((size_t)nkf, -1);                       // (per point: the last point that named the keyframe)
    for (int p = 0; p < npts; p++)
      for (int e = obs_off[p]; e < obs_off[p + 1]; e++) {
        const int k = obs_kf[e], s = obs_slot[e];
        if (obs_dead && obs_dead[e]) continue;                            // (absent: nothing of it is read but obs_kf above)
        ORBHIP_REQUIRE(s >= 0 && s < kf_slot_off[k + 1] - kf_slot_off[k], ORBHIP_EINVAL, "orbl_apply_map_edits: an obs_slot lies outside its keyframe's slots");
        ORBHIP_REQUIRE(seen[k] != p, ORBHIP_EINVAL, "orbl_apply_map_edits: an observation list names a keyframe twice");
        ORBHIP_REQUIRE(kf_slot_pt[kf_slot_off[k] + s] == p, ORBHIP_EINVAL, "orbl_apply_map_edits: an observation's slot does not hold its point");
        seen[k] = p;
      }
  }
  for (int i = 0; i < nops; i++) {
    const int kind = op_kind[i];
    ORBHIP_REQUIRE(kind >= 0 && kind <= 6, ORBHIP_EINVAL, "orbl_apply_map_edits: an op_kind is out of range (0 to 6)");
    if (kind == 0) continue;
    ORBHIP_REQUIRE(op_pt[i] >= 0 && op_pt[i] < npts, ORBHIP_EINVAL, "orbl_apply_map_edits: an op_pt is out of range");
    if (kind == 2) ORBHIP_REQUIRE(op_arg[i] >= 0 && op_arg[i] < npts, ORBHIP_EINVAL, "orbl_apply_map_edits: the op_arg of a REPLACE is no point");
    if (kind == 1 || kind == 4 || kind == 5) {
      ORBHIP_REQUIRE(op_kf[i] >= 0 && op_kf[i] < nkf, ORBHIP_EINVAL, "orbl_apply_map_edits: an op_kf is out of range");
      ORBHIP_REQUIRE(op_slot[i] >= 0 && op_slot[i] < kf_slot_off[op_kf[i] + 1] - kf_slot_off[op_kf[i]], ORBHIP_EINVAL,
                     "orbl_apply_map_edits: an op_slot lies outside its keyframe's slots");
    }
    if (kind == 6)
      ORBHIP_REQUIRE(op_arg[i] >= 0 && op_arg[i] < i && op_kind[op_arg[i]] == 5, ORBHIP_EINVAL,
                     "orbl_apply_map_edits: the op_arg of a REPLACE_FOUND names no earlier FIND_OR_ADD");
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t no = (size_t)nops, nk = (size_t)nkf, np = (size_t)npts, ns = (size_t)nslots, nb = (size_t)nobs, cap = (size_t)cap_obs;
  const bool attrs = kf_slot_level != nullptr;
  RoundTrip R(W);
  const HostIn<int32_t> d_kind = R.in(op_kind, no), d_pt = R.in(op_pt, no), d_arg = R.in(op_arg, no), d_kf = R.in(op_kf, no), d_slot = R.in(op_slot, no);
  const HostIn<int32_t> d_slot_off = R.csr(kf_slot_off ? kf_slot_off : &R.zero, nk), d_rank = R.in(kf_rank, nk), d_level = R.in(kf_slot_level, ns);
  const HostIn<float> d_uv = R.in(kf_slot_uv, 2 * ns);
  const HostIn<int32_t> d_obs_off = R.csr(obs_off ? obs_off : &R.zero, np), d_obs_kf = R.in(obs_kf, nb), d_obs_slot = R.in(obs_slot, nb);
  const HostIn<uint8_t> d_dead = R.in(obs_dead, nb);
  const HostOut<int32_t> io_slot_pt = R.inout(kf_slot_pt, ns), io_nobs = R.inout(pt_nobs, np), io_found = R.inout(pt_found, np), io_visible = R.inout(pt_visible, np);
  const HostOut<int32_t> io_replaced = R.inout(pt_replaced, np);
  const HostOut<uint8_t> io_bad = R.inout(pt_bad, np);
  const HostOut<int32_t> o_counts = R.out<int32_t>(8), o_status = R.out<int32_t>(no), o_found = R.out<int32_t>(no), o_off = R.out<int32_t>(np + 1);
  const HostOut<uint8_t> o_touched = R.out<uint8_t>(np);
  const HostOut<int32_t> o_kf = R.out<int32_t>(cap), o_slot = R.out<int32_t>(cap), o_src = R.out<int32_t>(cap, oobs_src != nullptr), o_level = R.out<int32_t>(cap, attrs);
  const HostOut<float> o_uv = R.out<float>(2 * cap, attrs);
  const HostOut<uint32_t> o_bits = R.out<uint32_t>(1);
  R.scratch(me_workspace(nops, nkf, npts, nobs).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_apply_map_edits_device(nops, d_kind.dev(), d_pt.dev(), d_arg.dev(), d_kf.dev(), d_slot.dev(), nkf, d_slot_off.dev(), d_rank.dev(), nslots,
                                        io_slot_pt.dev(), d_level.dev(), d_uv.dev(), npts, io_bad.dev(), io_nobs.dev(), io_found.dev(), io_visible.dev(),
                                        io_replaced.dev(), nobs, d_obs_off.dev(), d_obs_kf.dev(), d_obs_slot.dev(), d_dead.dev(), cap_obs, o_status.dev(), o_found.dev(),
                                        o_touched.dev(), o_off.dev(), o_kf.dev(), o_slot.dev(), o_src.dev(), o_level.dev(), o_uv.dev(), o_counts.dev(), o_bits.dev(),
                                        R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 8);
  const size_t n_out = (size_t)o_counts[0];
  if (n_out > cap) {
    set_error("orbl_apply_map_edits: wanted %d observations; capacity %d", o_counts[0], cap_obs);
    return ORBHIP_ECAP;
  }
  R.copy_out(io_slot_pt, kf_slot_pt, ns); R.copy_out(io_bad, pt_bad, np); R.copy_out(io_nobs, pt_nobs, np); R.copy_out(io_found, pt_found, np);
  R.copy_out(io_visible, pt_visible, np); R.copy_out(io_replaced, pt_replaced, np);
  R.copy_out(o_status, op_status, no); R.copy_out(o_found, op_found, no); R.copy_out(o_touched, pt_touched, np); R.copy_out(o_off, oobs_off, np + 1);
  R.copy_out(o_kf, oobs_kf, n_out); R.copy_out(o_slot, oobs_slot, n_out); R.copy_out(o_src, oobs_src, n_out); R.copy_out(o_level, oobs_level, n_out);
  R.copy_out(o_uv, oobs_uv, 2 * n_out);
  return 0;
}

}  // extern "C"
