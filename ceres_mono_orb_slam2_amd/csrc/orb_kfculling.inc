// orb_kfculling.inc -- LocalMapping::KeyFrameCulling (src/LocalMapping.cc:576-637) for the whole candidate list in one call
// (orbl_keyframe_culling*), with the state changes of KeyFrame::SetBadFlag (src/KeyFrame.cc:460-480: every map point of the culled
// keyframe loses its observation) and MapPoint::EraseObservation (src/MapPoint.cc:140-162: a point left with <= 2 observations turns
// bad) applied between candidates, as the reference's loop does.  Textually included by orb_localmap.hip.
//
// The loop is ORDER-DEPENDENT: what candidate c counts depends on which of the candidates before it were culled.  The work that
// does not depend on the order is done grid-wide first, the ordered part touches only what a cull changes.  Four launches on one
// stream, no waiting between workgroups:
//   k_cull_init     one lane per point / observation / candidate: the mutable state (bad, nobs per point, dead per observation),
//                   the input checks of the device form (an out-of-range entry is treated as absent and flagged in *status).
//   k_cull_count    one lane group per slot (8, 16 or 32 lanes by the mean list length, several slots per wave; a list longer than a
//                   wave is walked by the whole wave afterwards): cnt[s] = the UNCAPPED number of other observers of the slot's point
//                   at level <= slot_level + 1 under the initial state (the reference's `break` at th_obs is only a cap), and the cross
//                   index: sobs[s] = the keyframe's own observation of the point, and through ohead[e] / snext[s] the slots an
//                   observation belongs to (a chain: one slot on a consistent map, more when a point is listed twice in a keyframe).
//   k_cull_resolve  ONE workgroup of 1024 walks the candidates in order: n_redundant / n_map_points re-derived from cnt, nobs and bad
//                   by a block reduction, the decision (one IEEE double multiply, as the reference's int > 0.9 * int), and on a cull
//                   the incremental update: per point of the culled keyframe dead[e] = 1, nobs--, bad when <= 2; for every other
//                   live observer's slots s', cnt[s']-- when the erased observation's level <= slot_level[s'] + 1.
//   k_cull_export   the final state into the caller's arrays.
// Inside k_cull_resolve every word of the mutable state has ONE writer per phase (a point is handled by the one slot that claimed
// it), all accesses are plain loads and stores, and phases are separated by workgroup barriers: no atomics on global memory there.
#include "orb_maptable.h"

namespace orbhip {

#define KC_WG 256
#define KC_RWG 1024               /* k_cull_resolve: one workgroup */
#define KC_LONG 32                /* k_cull_resolve: a culled point with a longer list is walked by a wave, not by one lane */
#define KC_DEFER 1024             /* capacity of the list of such points (beyond it the owning lane walks the list itself) */
#define KC_NONE 0x7FFFFFFF        /* "no entry of the keyframe itself in this list" while scanning */
#define KC_ST_OFFSETS 1u          /* *status bits of the device form */
#define KC_ST_INDEX 2u
#define KC_ST_LEVEL 4u

struct CullArgs {
  int ncand, nslots, nkf, npts, nobs, th_obs; double ratio;
  const int32_t* cand_kf; const uint8_t* cand_flags; const int32_t* slot_off; const int32_t* slot_pt; const int32_t* slot_level;
  const int32_t* obs_off; const int32_t* obs_kf; const int32_t* obs_level; const uint8_t* pt_bad; const int32_t* pt_nobs;
  uint8_t* culled; int32_t* n_red; int32_t* n_mp; uint8_t* pt_bad_out; int32_t* pt_nobs_out; uint8_t* obs_erased; uint32_t* status;
  // workspace: cnt | spt | sobs | snext [nslots], ohead | dead [nobs], bad | ncur | claim [npts]
  int32_t *cnt, *spt, *sobs, *snext, *ohead, *dead, *bad, *ncur, *claim;
};

__global__ __launch_bounds__(KC_WG) void k_cull_init(CullArgs a) {
  const int i = blockIdx.x * KC_WG + threadIdx.x;
  if (i < a.npts) {
    int lo, hi;
    if (!mt_range(a.obs_off, i, a.nobs, &lo, &hi)) mt_flag(a.status, KC_ST_OFFSETS);
    a.bad[i] = a.pt_bad ? (a.pt_bad[i] != 0) : 0;
    a.ncur[i] = a.pt_nobs ? a.pt_nobs[i] : hi - lo;
    a.claim[i] = -1;
  }
  if (i < a.nobs) {
    const int k = a.obs_kf[i];
    if (k < 0 || k >= a.nkf) mt_flag(a.status, KC_ST_INDEX);
    if (a.obs_level[i] < 0) mt_flag(a.status, KC_ST_LEVEL);
    a.dead[i] = 0; a.ohead[i] = -1;
  }
  if (i < a.ncand) {
    int lo, hi;
    if (!mt_range(a.slot_off, i, a.nslots, &lo, &hi)) mt_flag(a.status, KC_ST_OFFSETS);
    const int k = a.cand_kf[i];
    if (k < 0 || k >= a.nkf) mt_flag(a.status, KC_ST_INDEX);
  }
}

// entries [lo, hi) of one point's list, taken `stride` apart from lo + first: the observers other than k at level <= l + 1 (count), and the
// first entry of keyframe k itself (mine).  Entries the device form could not accept (keyframe out of range, negative level) are absent.
__device__ __forceinline__ void kc_scan(const CullArgs& a, int lo, int hi, int first, int stride, int k, int l, int* count, int* mine) {
  for (int e = lo + first; e < hi; e += stride) {
    const int kf = a.obs_kf[e], le = a.obs_level[e];
    if (kf < 0 || kf >= a.nkf || le < 0) continue;
    if (kf == k) *mine = min(*mine, e);
    else *count += le - 1 <= l;                                      // (scaleLeveli <= scaleLevel + 1, :620)
  }
}

__device__ __forceinline__ void kc_store_slot(const CullArgs& a, int s, int p, int count, int mine) {
  a.spt[s] = p; a.cnt[s] = count;
  const bool own = mine != KC_NONE;
  a.sobs[s] = own ? mine : -1;
  a.snext[s] = own ? atomicExch(&a.ohead[mine], s) : -1;             // (push the slot on its observation's chain)
}

// A group of G lanes per slot, 64 / G slots per wave, 4 waves per workgroup.
template <int G>
__global__ __launch_bounds__(KC_WG) void k_cull_count(CullArgs a) {
  constexpr int PW = 64 / G;
  const int lane = threadIdx.x & 63, g = lane / G, r = lane % G;
  const int s = (blockIdx.x * (KC_WG / 64) + (threadIdx.x >> 6)) * PW + g;
  const bool act = s < a.nslots;
  // the candidate that owns the slot: the last c with slot_off[c] <= s
  int c = -1;
  if (act) {
    int b = 0, t = a.ncand;
    while (b < t) { const int m = (b + t) >> 1; if (a.slot_off[m] <= s) b = m + 1; else t = m; }
    c = b - 1;
    if (c >= 0 && !(a.slot_off[c] <= s && s < a.slot_off[c + 1])) c = -1;      // (offsets that do not ascend: nobody's slot)
  }
  const int k = c >= 0 ? a.cand_kf[c] : -1;
  const int p = c >= 0 ? a.slot_pt[s] : -1, l = c >= 0 ? a.slot_level[s] : 0;
  const bool kok = k >= 0 && k < a.nkf, pok = p >= 0 && p < a.npts;
  if (kok && r == 0) {
    if (!pok) mt_flag(a.status, KC_ST_INDEX);
    if (l < 0) mt_flag(a.status, KC_ST_LEVEL);
  }
  const bool ok = kok && pok && l >= 0;
  int lo = 0, hi = 0;
  if (ok) mt_range(a.obs_off, p, a.nobs, &lo, &hi);
  const bool is_long = hi - lo > 64;
  int count = 0, mine = KC_NONE;
  if (!is_long) kc_scan(a, lo, hi, r, G, k, l, &count, &mine);
#pragma unroll
  for (int m = 1; m < G; m <<= 1) { count += __shfl_xor(count, m); mine = min(mine, __shfl_xor(mine, m)); }
  if (act && r == 0 && !is_long) kc_store_slot(a, s, ok ? p : -1, count, mine);
  // lists longer than a wave: one after the other, all 64 lanes lane-strided
  uint64_t todo = __ballot(is_long && r == 0);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const int ws = __shfl(s, src), wp = __shfl(p, src), wk = __shfl(k, src), wl = __shfl(l, src), wlo = __shfl(lo, src), whi = __shfl(hi, src);
    int wc = 0, wm = KC_NONE;
    kc_scan(a, wlo, whi, lane, 64, wk, wl, &wc, &wm);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { wc += __shfl_xor(wc, m); wm = min(wm, __shfl_xor(wm, m)); }
    if (lane == 0) kc_store_slot(a, ws, wp, wc, wm);
  }
}

// The part of one cull that belongs to point p, whose observation by keyframe k (level `lvl`) has just died: entries first, first + stride, ...
// of its list.  now_bad: the point turned bad - all its observations die (MapPoint::SetBadFlag, :174-191).  Otherwise every other live
// observer's slots lose one from their count when the erased level is within their reach.
__device__ __forceinline__ void kc_walk(const CullArgs& a, int p, int k, int lvl, bool now_bad, int first, int stride) {
  int lo, hi;
  mt_range(a.obs_off, p, a.nobs, &lo, &hi);
  for (int e = lo + first; e < hi; e += stride) {
    if (now_bad) { a.dead[e] = 1; continue; }
    if (a.dead[e] || a.obs_kf[e] == k) continue;
    for (int s = a.ohead[e]; s >= 0; s = a.snext[s])
      if (lvl - 1 <= a.slot_level[s]) a.cnt[s] -= 1;
  }
}

__global__ __launch_bounds__(KC_RWG) void k_cull_resolve(CullArgs a) {
  __shared__ int s_red[KC_RWG / 64], s_mp[KC_RWG / 64];
  __shared__ int s_def[KC_DEFER];
  __shared__ int s_ndef;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int c = 0; c < a.ncand; c++) {
    const int k = a.cand_kf[c];
    const int flags = a.cand_flags ? a.cand_flags[c] : 0;
    if ((flags & 1) || k < 0 || k >= a.nkf) {                       // (:588) id_ == 0, or a keyframe the device form could not accept
      if (tid == 0) { a.culled[c] = 0; a.n_red[c] = 0; a.n_mp[c] = 0; }
      continue;
    }
    int lo, hi;
    mt_range(a.slot_off, c, a.nslots, &lo, &hi);
    int red = 0, mp = 0;
    for (int s = lo + tid; s < hi; s += KC_RWG) {                   // (:595-631) under the state the culls so far have left
      const int p = a.spt[s];
      if (p < 0 || a.bad[p]) continue;
      mp++;
      red += a.ncur[p] > a.th_obs && a.cnt[s] >= a.th_obs;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { red += __shfl_xor(red, m); mp += __shfl_xor(mp, m); }
    if (lane == 0) { s_red[w] = red; s_mp[w] = mp; }
    if (tid == 0) s_ndef = 0;
    __syncthreads();
    red = 0; mp = 0;
#pragma unroll
    for (int i = 0; i < KC_RWG / 64; i++) { red += s_red[i]; mp += s_mp[i]; }
    const bool cull = (double)red > a.ratio * (double)mp;           // (:633)
    if (tid == 0) { a.culled[c] = cull; a.n_red[c] = red; a.n_mp[c] = mp; }
    if (cull && !(flags & 2)) {                                     // KeyFrame::SetBadFlag; do_not_erase_ (bit 1): nothing changes
      // a point listed in several slots of this keyframe is handled once: by the slot whose claim survives
      for (int s = lo + tid; s < hi; s += KC_RWG) {
        const int p = a.spt[s];
        if (p >= 0 && !a.bad[p] && a.sobs[s] >= 0 && !a.dead[a.sobs[s]]) a.claim[p] = s;
      }
      __syncthreads();
      for (int s = lo + tid; s < hi; s += KC_RWG) {
        const int p = a.spt[s];
        if (p < 0 || a.bad[p]) continue;
        const int e = a.sobs[s];
        if (e < 0 || a.dead[e] || a.claim[p] != s) continue;
        a.dead[e] = 1;                                              // MapPoint::EraseObservation (:140-162)
        const int n = a.ncur[p] - 1;
        a.ncur[p] = n;
        if (n <= 2) a.bad[p] = 1;
        if (a.obs_off[p + 1] - a.obs_off[p] > KC_LONG) {
          const int at = atomicAdd(&s_ndef, 1);
          if (at < KC_DEFER) { s_def[at] = s; continue; }
        }
        kc_walk(a, p, k, a.obs_level[e], n <= 2, 0, 1);
      }
      __syncthreads();
      const int nd = min(s_ndef, KC_DEFER);
      for (int i = w; i < nd; i += KC_RWG / 64) {                    // long lists: a wave each, lane-strided
        const int s = s_def[i], p = a.spt[s];
        kc_walk(a, p, k, a.obs_level[a.sobs[s]], a.bad[p] != 0, lane, 64);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(KC_WG) void k_cull_export(CullArgs a) {
  const int i = blockIdx.x * KC_WG + threadIdx.x;
  if (i < a.npts) {
    if (a.pt_bad_out) a.pt_bad_out[i] = a.bad[i] != 0;
    if (a.pt_nobs_out) a.pt_nobs_out[i] = a.ncur[i];
  }
  if (i < a.nobs && a.obs_erased) a.obs_erased[i] = a.dead[i] != 0;
}

// workspace sections, each rounded up to 256 bytes
struct CullWs { size_t cnt, spt, sobs, snext, ohead, dead, bad, ncur, claim, total; };
static CullWs cull_workspace(int nslots, int npts, int nobs) {
  CullWs w; Carve ws;
  const size_t slots = 4 * (size_t)nslots, obs = 4 * (size_t)nobs, pts = 4 * (size_t)npts;      // (every section holds 4-byte entries)
  w.cnt = ws.take(slots); w.spt = ws.take(slots); w.sobs = ws.take(slots); w.snext = ws.take(slots);
  w.ohead = ws.take(obs); w.dead = ws.take(obs); w.bad = ws.take(pts); w.ncur = ws.take(pts); w.claim = ws.take(pts);
  w.total = ws.total > 0 ? ws.total : 256;
  return w;
}

}  // namespace orbhip

extern "C" {

int orbl_keyframe_culling_workspace(int ncand, int nslots, int npts, int nobs, size_t* bytes) {
  ORBHIP_REQUIRE(ncand >= 0 && nslots >= 0 && npts >= 0 && nobs >= 0 && bytes, ORBHIP_EINVAL, "orbl_keyframe_culling_workspace: bad argument");
  *bytes = orbhip::cull_workspace(nslots, npts, nobs).total;
  return 0;
}

int orbl_keyframe_culling_device(int ncand, const int32_t* cand_kf, const uint8_t* cand_flags, int nslots, const int32_t* slot_off, const int32_t* slot_pt,
                                 const int32_t* slot_level, int nkf, int npts, int nobs, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_level,
                                 const uint8_t* pt_bad, const int32_t* pt_nobs, int th_obs, double ratio, uint8_t* culled, int32_t* n_redundant,
                                 int32_t* n_map_points, uint8_t* pt_bad_out, int32_t* pt_nobs_out, uint8_t* obs_erased, uint32_t* status, void* workspace,
                                 void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(ncand >= 0 && nslots >= 0 && nkf >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_keyframe_culling: negative count");
  ORBHIP_REQUIRE(th_obs >= 1 && std::isfinite(ratio), ORBHIP_EINVAL, "orbl_keyframe_culling: th_obs must be >= 1 and ratio finite");
  ORBHIP_REQUIRE(workspace, ORBHIP_EINVAL, "orbl_keyframe_culling: NULL workspace");
  ORBHIP_REQUIRE(ncand == 0 || (cand_kf && slot_off && culled && n_redundant && n_map_points), ORBHIP_EINVAL, "orbl_keyframe_culling: NULL candidate argument");
  ORBHIP_REQUIRE(nslots == 0 || (ncand > 0 && slot_pt && slot_level), ORBHIP_EINVAL, "orbl_keyframe_culling: NULL slot argument");
  ORBHIP_REQUIRE(npts == 0 || obs_off, ORBHIP_EINVAL, "orbl_keyframe_culling: NULL obs_off");
  ORBHIP_REQUIRE(nobs == 0 || (npts > 0 && obs_kf && obs_level), ORBHIP_EINVAL, "orbl_keyframe_culling: NULL observation argument");
  const void* words[] = {cand_kf, slot_off, slot_pt, slot_level, obs_off, obs_kf, obs_level, pt_nobs, n_redundant, n_map_points, pt_nobs_out, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_keyframe_culling: 32-bit arrays must be 4-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)workspace % 4 == 0, ORBHIP_EINVAL, "orbl_keyframe_culling: workspace must be 4-byte aligned");
  const CullWs ws = cull_workspace(nslots, npts, nobs);
  uint8_t* wb = (uint8_t*)workspace;
  CullArgs A;
  A.ncand = ncand; A.nslots = nslots; A.nkf = nkf; A.npts = npts; A.nobs = nobs; A.th_obs = th_obs; A.ratio = ratio;
  A.cand_kf = cand_kf; A.cand_flags = cand_flags; A.slot_off = slot_off; A.slot_pt = slot_pt; A.slot_level = slot_level;
  A.obs_off = obs_off; A.obs_kf = obs_kf; A.obs_level = obs_level; A.pt_bad = pt_bad; A.pt_nobs = pt_nobs;
  A.culled = culled; A.n_red = n_redundant; A.n_mp = n_map_points; A.pt_bad_out = pt_bad_out; A.pt_nobs_out = pt_nobs_out; A.obs_erased = obs_erased;
  A.status = status;
  A.cnt = (int32_t*)(wb + ws.cnt); A.spt = (int32_t*)(wb + ws.spt); A.sobs = (int32_t*)(wb + ws.sobs); A.snext = (int32_t*)(wb + ws.snext);
  A.ohead = (int32_t*)(wb + ws.ohead); A.dead = (int32_t*)(wb + ws.dead);
  A.bad = (int32_t*)(wb + ws.bad); A.ncur = (int32_t*)(wb + ws.ncur); A.claim = (int32_t*)(wb + ws.claim);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  const int n_init = std::max(std::max(npts, nobs), ncand), n_state = std::max(npts, nobs);
  if (n_init > 0) hipLaunchKernelGGL(k_cull_init, dim3((n_init + KC_WG - 1) / KC_WG), dim3(KC_WG), 0, st, A);
  if (nslots > 0) {
    // lanes per slot by the mean list length
    const int mean = npts > 0 ? nobs / npts : 0;
    const int G = mean <= 6 ? 8 : mean <= 12 ? 16 : 32;
    const int per_wg = (KC_WG / 64) * (64 / G);
    const dim3 grid((nslots + per_wg - 1) / per_wg), wg(KC_WG);
    if (G == 8) hipLaunchKernelGGL(k_cull_count<8>, grid, wg, 0, st, A);
    else if (G == 16) hipLaunchKernelGGL(k_cull_count<16>, grid, wg, 0, st, A);
    else hipLaunchKernelGGL(k_cull_count<32>, grid, wg, 0, st, A);
  }
  if (ncand > 0) hipLaunchKernelGGL(k_cull_resolve, dim3(1), dim3(KC_RWG), 0, st, A);
  if (n_state > 0 && (pt_bad_out || pt_nobs_out || obs_erased)) hipLaunchKernelGGL(k_cull_export, dim3((n_state + KC_WG - 1) / KC_WG), dim3(KC_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_keyframe_culling(int ncand, const int32_t* cand_kf, const uint8_t* cand_flags, const int32_t* slot_off, const int32_t* slot_pt, const int32_t* slot_level,
                          int nkf, int npts, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_level, const uint8_t* pt_bad,
                          const int32_t* pt_nobs, int th_obs, double ratio, uint8_t* culled, int32_t* n_redundant, int32_t* n_map_points, uint8_t* pt_bad_out,
                          int32_t* pt_nobs_out, uint8_t* obs_erased) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(ncand >= 0 && nkf >= 0 && npts >= 0, ORBHIP_EINVAL, "orbl_keyframe_culling: negative count");
  ORBHIP_REQUIRE(th_obs >= 1, ORBHIP_EINVAL, "orbl_keyframe_culling: th_obs must be >= 1");
  ORBHIP_REQUIRE(std::isfinite(ratio), ORBHIP_EINVAL, "orbl_keyframe_culling: ratio is not finite");
  ORBHIP_REQUIRE(ncand == 0 || (cand_kf && slot_off && culled && n_redundant && n_map_points), ORBHIP_EINVAL, "orbl_keyframe_culling: NULL candidate argument");
  ORBHIP_REQUIRE(npts == 0 || obs_off, ORBHIP_EINVAL, "orbl_keyframe_culling: NULL obs_off");
  static const char E[] = "orbl_keyframe_culling";
  int nslots = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "slot_off", slot_off, ncand, &nslots));
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE(nslots == 0 || (slot_pt && slot_level), ORBHIP_EINVAL, "orbl_keyframe_culling: NULL slot argument");
  ORBHIP_REQUIRE(nobs == 0 || (obs_kf && obs_level), ORBHIP_EINVAL, "orbl_keyframe_culling: NULL observation argument");
  ORBHIP_ARG(check_index(E, "cand_kf", cand_kf, ncand, nkf));
  ORBHIP_ARG(check_index(E, "slot_pt", slot_pt, nslots, npts));
  ORBHIP_ARG(check_not_negative(E, "slot_level", slot_level, nslots));
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  ORBHIP_ARG(check_not_negative(E, "obs_level", obs_level, nobs));
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nc = (size_t)ncand, ns = (size_t)nslots, np = (size_t)npts, no = (size_t)nobs;
  RoundTrip R(W);
  const HostIn<int32_t> d_cand = R.in(cand_kf, nc), d_slot_off = R.csr(slot_off, nc), d_slot_pt = R.in(slot_pt, ns), d_slot_level = R.in(slot_level, ns);
  const HostIn<int32_t> d_obs_off = R.csr(obs_off, np), d_obs_kf = R.in(obs_kf, no), d_obs_level = R.in(obs_level, no), d_nobs = R.in(pt_nobs, np);
  const HostIn<uint8_t> d_flags = R.in(cand_flags, nc), d_bad = R.in(pt_bad, np);
  const HostOut<uint8_t> o_culled = R.out<uint8_t>(nc), o_bad = R.out<uint8_t>(np, pt_bad_out != nullptr), o_erased = R.out<uint8_t>(no, obs_erased != nullptr);
  const HostOut<int32_t> o_red = R.out<int32_t>(nc), o_mp = R.out<int32_t>(nc), o_nobs = R.out<int32_t>(np, pt_nobs_out != nullptr);
  R.scratch(cull_workspace(nslots, npts, nobs).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_keyframe_culling_device(ncand, d_cand.dev(), d_flags.dev(), nslots, d_slot_off.dev(), d_slot_pt.dev(), d_slot_level.dev(), nkf, npts, nobs,
                                         d_obs_off.dev(), d_obs_kf.dev(), d_obs_level.dev(), d_bad.dev(), d_nobs.dev(), th_obs, ratio, o_culled.dev(), o_red.dev(),
                                         o_mp.dev(), o_bad.dev(), o_nobs.dev(), o_erased.dev(), nullptr, R.scratch_dev(), R.stream()))) return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_culled, culled, nc); R.copy_out(o_red, n_redundant, nc); R.copy_out(o_mp, n_map_points, nc);
  R.copy_out(o_bad, pt_bad_out, np); R.copy_out(o_nobs, pt_nobs_out, np); R.copy_out(o_erased, obs_erased, no);
  return 0;
}

}  // extern "C"
