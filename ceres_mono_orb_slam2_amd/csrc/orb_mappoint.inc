// orb_mappoint.inc -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:256-315) and MapPoint::UpdateNormalAndDepth
// (:335-378) for a BATCH of map points (orbl_update_map_points*).  Textually included by orb_localmap.hip.
//
// Every point is independent of every other one; only the order inside one point's observation list matters (the caller's
// std::map<KeyFrame*, size_t> iteration order).  Two launches per call:
//   k_mp_prep   one lane per point: the normal / depth walk over the whole list (bad keyframes included, as the reference),
//               the count N of observations from good keyframes, N <= 1 resolved on the spot, the rest appended to one of five
//               buckets by N (<= 8, 16, 32, 64: lane groups of that size, several points per wave; > 64: one workgroup per point).
//               The buckets are filled on the device, so the device entry point needs no host copy of the CSR offsets.
//   k_mp_desc   the distinctive descriptor of every bucketed point: grid-stride over work units, the workgroup points first.
//               Descriptors staged in LDS, distances as 32-bit xor + popcount, the median (sorted_row[(N - 1) / 2], the row's own
//               zero included) by a 9-step bitwise search on the value 0..256 (lane groups) or a per-wave 257-bin histogram
//               (workgroup points), the argmin as a min of (median, row): ties go to the lowest row, as `median < best_median`.
// Rows are numbered by LIST position (bad-keyframe entries skipped): the reference's index among the good descriptors is monotone
// in it, so the first-minimum rule picks the same entry, and the result IS the list position the caller needs.
#include "orb_maptable.h"

namespace orbhip {

#define MP_WG 256
#define MP_NB 5                   /* buckets: N <= 8, <= 16, <= 32, <= 64, > 64 */
#define MP_STAGE 512              /* workgroup points: lists up to this many entries are staged in LDS, longer ones read from global */
#define MP_HIST 260               /* per-wave histogram bins (257 used) */

struct MpArgs {
  int npts, nobs, nkf, n_levels, what;
  const int32_t* obs_off; const double* X; const int32_t* ref_kf; const int32_t* ref_level; const uint8_t* pt_good;
  const int32_t* obs_kf; const uint32_t* obs_desc; const uint8_t* obs_good; const double* kf_center; const float* scale_factors;
  int32_t* best_obs; uint32_t* desc_out; double* normal; float* min_max; uint8_t* nd_written;
  uint32_t* cnt;                  // workspace: cnt[8] (MP_NB used) | list[MP_NB][npts]
  uint32_t* list;
};

__device__ __forceinline__ bool mp_good(const MpArgs& a, int e) { return !a.obs_good || a.obs_good[e]; }

__device__ __forceinline__ int mp_ham(const uint32_t (&own)[8], const uint32_t* __restrict__ q) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d += __popc(own[k] ^ q[k]);
  return d;
}

__global__ __launch_bounds__(MP_WG) void k_mp_prep(MpArgs a) {
  const int p = blockIdx.x * MP_WG + threadIdx.x;
  if (p >= a.npts) return;
  // empty list, bad point, or offsets the device entry point could not check: the point is left unchanged
  int lo, hi;
  const bool live = mt_range(a.obs_off, p, a.nobs, &lo, &hi) && lo < hi && (!a.pt_good || a.pt_good[p]);
  if (a.what & ORBL_MP_NORMAL_DEPTH) {                               // the walk covers the whole list, bad keyframes included, as the reference's
    uint8_t wrote = 0;
    const int r = live ? a.ref_kf[p] : -1, lvl = live ? a.ref_level[p] : -1;
    if (r >= 0 && r < a.nkf && lvl >= 0 && lvl < a.n_levels)
      wrote = mt_normal_depth(a.obs_kf, lo, hi, a.nkf, a.kf_center, a.X[3 * (size_t)p], a.X[3 * (size_t)p + 1], a.X[3 * (size_t)p + 2], r, lvl, a.scale_factors,
                              a.n_levels, a.normal + 3 * (size_t)p, a.min_max + 2 * (size_t)p) == MT_ND_OK;
    a.nd_written[p] = wrote;
  }
  if (a.what & ORBL_MP_DESC) {
    int n = 0, first = -1;
    if (live)
      for (int e = lo; e < hi; e++)
        if (mp_good(a, e)) { if (n == 0) first = e; n++; }
    if (n >= 2) {
      const int b = n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : 4;
      const uint32_t at = atomicAdd(&a.cnt[b], 1u);
      a.list[(size_t)b * a.npts + at] = (uint32_t)p;
      return;
    }
    if (n == 1)                                                    // one descriptor: the 1 x 1 matrix picks it
      for (int k = 0; k < 8; k++) a.desc_out[8 * (size_t)p + k] = a.obs_desc[8 * (size_t)first + k];
    a.best_obs[p] = n == 1 ? first - lo : -1;
  }
}

// Points with 2 <= N <= G: a group of G lanes per point, 64 / G points per wave, lane r owns row r of the N x N matrix.
// unit = one workgroup's share: 4 waves x (64 / G) consecutive entries of the bucket list.
template <int G>
__device__ void mp_desc_groups(const MpArgs& a, const uint32_t* __restrict__ lst, int count, int unit, uint32_t* sd, int* spos) {
  constexpr int PW = 64 / G;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane / G, r = lane % G;
  const int q = (unit * 4 + w) * PW + g;
  const bool act = q < count;
  const int p = act ? (int)lst[q] : 0;
  const int lo = act ? a.obs_off[p] : 0, hi = act ? a.obs_off[p + 1] : 0;
  uint32_t* D = sd + 8 * (w * 64 + g * G);
  int* P = spos + w * 64 + g * G;
  // stage the good-keyframe descriptors in list order: a chunk of G entries per step, compacted by a ballot of the group's lanes
  int n = 0;
  for (int c = lo; c < hi; c += G) {
    const int e = c + r;
    const bool good = e < hi && mp_good(a, e);
    const uint64_t m = __ballot(good);
    uint64_t gm = m;
    if constexpr (G < 64) gm = (m >> (g * G)) & ((1ull << G) - 1);
    const int slot = n + __popcll(gm & ((1ull << r) - 1));
    if (good && slot < G) {
      const uint4* s = (const uint4*)(a.obs_desc + 8 * (size_t)e);
      const uint4 v0 = s[0], v1 = s[1];
      uint32_t* o = D + 8 * slot;
      o[0] = v0.x; o[1] = v0.y; o[2] = v0.z; o[3] = v0.w; o[4] = v1.x; o[5] = v1.y; o[6] = v1.z; o[7] = v1.w;
      P[slot] = e - lo;
    }
    n += __popcll(gm);
  }
  __syncthreads();
  const int N = n < G ? n : G;
  unsigned key = 0xFFFFFFFFu;
  if (act && r < N) {
    uint32_t own[8];
#pragma unroll
    for (int k = 0; k < 8; k++) own[k] = D[8 * r + k];
    int d[G];
#pragma unroll
    for (int j = 0; j < G; j++) d[j] = j < N ? mp_ham(own, D + 8 * j) : 512;     // (512: never <= a candidate, which stays < 512)
    // smallest v with #{d <= v} >= t, t = (N - 1) / 2 + 1: bit by bit from 256 down
    const int t = (N - 1) / 2 + 1;
    int med = 0;
#pragma unroll
    for (int b = 8; b >= 0; b--) {
      const int c = med + (1 << b) - 1;
      int k = 0;
#pragma unroll
      for (int j = 0; j < G; j++) k += d[j] <= c;
      if (k < t) med += 1 << b;
    }
    key = ((unsigned)med << 16) | (unsigned)r;
  }
#pragma unroll
  for (int m = 1; m < G; m <<= 1) key = min(key, (unsigned)__shfl_xor((int)key, m));
  if (act && N >= 1) {
    const int best = (int)(key & 0xFFFFu);
    if (r < 8) a.desc_out[8 * (size_t)p + r] = D[8 * best + r];
    if (r == 0) a.best_obs[p] = P[best];
  }
  __syncthreads();
}

// the rows of one workgroup point that wave w owns (w, w + 4, ...): per row a 257-bin histogram of its distances (LDS adds), the
// median from a wave scan of the bins.  Returns the wave's min of (median << 32 | row).
template <bool STAGED>
__device__ unsigned long long mp_large_rows(const MpArgs& a, int lo, int L, int N, const uint32_t* sd, const uint8_t* sg, uint32_t* H) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = (N - 1) / 2 + 1;
  const uint32_t* gd = a.obs_desc + 8 * (size_t)lo;
  unsigned long long best = ~0ull;
  for (int r = w; r < L; r += 4) {
    if (!(STAGED ? sg[r] != 0 : mp_good(a, lo + r))) continue;  // (wave-uniform)
    uint32_t own[8];
#pragma unroll
    for (int k = 0; k < 8; k++) own[k] = STAGED ? sd[8 * r + k] : gd[8 * r + k];
    for (int j = lane; j < L; j += 64) {
      if (!(STAGED ? sg[j] != 0 : mp_good(a, lo + j))) continue;
      const int d = mp_ham(own, STAGED ? sd + 8 * j : gd + 8 * (size_t)j);
      atomicAdd(&H[d], 1u);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t c0 = H[4 * lane], c1 = H[4 * lane + 1], c2 = H[4 * lane + 2], c3 = H[4 * lane + 3];
    const uint32_t s = c0 + c1 + c2 + c3;
    uint32_t incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= o) incl += v; }
    const uint64_t hit = __ballot(incl >= (uint32_t)t);
    int med = 256;                                                  // (no bin below 256 reaches t: the median is 256)
    if (hit) {
      const uint32_t ex = incl - s;
      const int mine = 4 * lane + (ex + c0 >= (uint32_t)t ? 0 : ex + c0 + c1 >= (uint32_t)t ? 1 : ex + c0 + c1 + c2 >= (uint32_t)t ? 2 : 3);
      med = __shfl(mine, __ffsll((unsigned long long)hit) - 1);
    }
    best = min(best, ((unsigned long long)med << 32) | (unsigned)r);
    H[4 * lane] = 0; H[4 * lane + 1] = 0; H[4 * lane + 2] = 0; H[4 * lane + 3] = 0;     // (each lane clears the bins it read)
    if (lane == 0) H[256] = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  return best;
}

// one point with N > 64: the whole workgroup, rows dealt to the four waves
__device__ void mp_desc_large(const MpArgs& a, int p, uint32_t* sd, uint8_t* sg, uint32_t* hist, unsigned long long* sbest, int* sn) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lo = a.obs_off[p], L = a.obs_off[p + 1] - lo;
  const bool staged = L <= MP_STAGE;
  int cnt = 0;
  for (int e = tid; e < L; e += MP_WG) {
    const bool gd = mp_good(a, lo + e);
    cnt += gd;
    if (staged) {
      sg[e] = gd;
      const uint4* s = (const uint4*)(a.obs_desc + 8 * ((size_t)lo + e));
      const uint4 v0 = s[0], v1 = s[1];
      uint32_t* o = sd + 8 * e;
      o[0] = v0.x; o[1] = v0.y; o[2] = v0.z; o[3] = v0.w; o[4] = v1.x; o[5] = v1.y; o[6] = v1.z; o[7] = v1.w;
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
  if (lane == 0) sn[w] = cnt;
  for (int i = tid; i < 4 * MP_HIST; i += MP_WG) hist[i] = 0;
  __syncthreads();
  const int N = sn[0] + sn[1] + sn[2] + sn[3];
  const unsigned long long b = staged ? mp_large_rows<true>(a, lo, L, N, sd, sg, hist + w * MP_HIST)
                                      : mp_large_rows<false>(a, lo, L, N, sd, sg, hist + w * MP_HIST);
  if (lane == 0) sbest[w] = b;
  __syncthreads();
  const unsigned long long k = min(min(sbest[0], sbest[1]), min(sbest[2], sbest[3]));
  const int e = (int)(k & 0xFFFFFFFFull);
  if (tid < 8) a.desc_out[8 * (size_t)p + tid] = staged ? sd[8 * e + tid] : a.obs_desc[8 * ((size_t)lo + e) + tid];
  if (tid == 0) a.best_obs[p] = e;
  __syncthreads();
}

__global__ __launch_bounds__(MP_WG) void k_mp_desc(MpArgs a) {
  __shared__ uint32_t sd[8 * MP_STAGE];          // staged descriptors (lane groups use the first 4 x 64)
  __shared__ int spos[256];
  __shared__ uint8_t sg[MP_STAGE];
  __shared__ uint32_t hist[4 * MP_HIST];
  __shared__ unsigned long long sbest[4];
  __shared__ int sn[4];
  const int c8 = (int)a.cnt[0], c16 = (int)a.cnt[1], c32 = (int)a.cnt[2], c64 = (int)a.cnt[3], cL = (int)a.cnt[4];
  const int u64 = (c64 + 3) / 4, u32 = (c32 + 7) / 8, u16 = (c16 + 15) / 16, u8 = (c8 + 31) / 32;
  const int total = cL + u64 + u32 + u16 + u8;
  const size_t np = (size_t)a.npts;
  for (int u = blockIdx.x; u < total; u += gridDim.x) {          // (u is workgroup-uniform: the barriers inside are reached by all)
    int v = u;
    if (v < cL) { mp_desc_large(a, (int)a.list[4 * np + v], sd, sg, hist, sbest, sn); continue; }
    v -= cL;
    if (v < u64) { mp_desc_groups<64>(a, a.list + 3 * np, c64, v, sd, spos); continue; }
    v -= u64;
    if (v < u32) { mp_desc_groups<32>(a, a.list + 2 * np, c32, v, sd, spos); continue; }
    v -= u32;
    if (v < u16) { mp_desc_groups<16>(a, a.list + np, c16, v, sd, spos); continue; }
    v -= u16;
    mp_desc_groups<8>(a, a.list, c8, v, sd, spos);
  }
}

static size_t mp_workspace_bytes(int npts) { return 32 + 4 * (size_t)MP_NB * (size_t)(npts > 0 ? npts : 0); }

}  // namespace orbhip

extern "C" {

int orbl_update_map_points_workspace(int npts, size_t* bytes) {
  ORBHIP_REQUIRE(npts >= 0 && bytes, ORBHIP_EINVAL, "orbl_update_map_points_workspace: bad argument");
  *bytes = orbhip::mp_workspace_bytes(npts);
  return 0;
}

int orbl_update_map_points_device(int npts, const int32_t* obs_off, const double* X, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* pt_good,
                                  int nobs, const int32_t* obs_kf, const uint8_t* obs_desc, const uint8_t* obs_kf_good, int nkf, const double* kf_center,
                                  const float* scale_factors, int n_levels, int what, int32_t* best_obs, uint8_t* desc_out, double* normal, float* min_max,
                                  uint8_t* nd_written, void* workspace, void* stream) {
  using namespace orbhip;
  ORBHIP_REQUIRE(npts >= 0 && nobs >= 0 && nkf >= 0, ORBHIP_EINVAL, "orbl_update_map_points: negative count");
  ORBHIP_REQUIRE(what >= 1 && what <= (ORBL_MP_DESC | ORBL_MP_NORMAL_DEPTH), ORBHIP_EINVAL, "orbl_update_map_points: `what` selects nothing known");
  if (npts == 0) return 0;
  const bool desc = what & ORBL_MP_DESC, nd = what & ORBL_MP_NORMAL_DEPTH;
  ORBHIP_REQUIRE(obs_off && workspace, ORBHIP_EINVAL, "orbl_update_map_points: NULL argument");
  ORBHIP_REQUIRE(!desc || ((nobs == 0 || obs_desc) && best_obs && desc_out), ORBHIP_EINVAL, "orbl_update_map_points: NULL descriptor argument");
  ORBHIP_REQUIRE(!desc || ((uintptr_t)obs_desc % 16 == 0 && (uintptr_t)desc_out % 4 == 0), ORBHIP_EINVAL,
                 "orbl_update_map_points: obs_desc must be 16-byte and desc_out 4-byte aligned");
  ORBHIP_REQUIRE(!nd || (X && ref_kf && ref_level && (nobs == 0 || obs_kf) && (nkf == 0 || kf_center) && scale_factors && normal && min_max && nd_written),
                 ORBHIP_EINVAL, "orbl_update_map_points: NULL normal / depth argument");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_update_map_points: n_levels out of range");
  MpArgs A;
  A.npts = npts; A.nobs = nobs; A.nkf = nkf; A.n_levels = n_levels; A.what = what;
  A.obs_off = obs_off; A.X = X; A.ref_kf = ref_kf; A.ref_level = ref_level; A.pt_good = pt_good;
  A.obs_kf = obs_kf; A.obs_desc = (const uint32_t*)obs_desc; A.obs_good = obs_kf_good; A.kf_center = kf_center; A.scale_factors = scale_factors;
  A.best_obs = best_obs; A.desc_out = (uint32_t*)desc_out; A.normal = normal; A.min_max = min_max; A.nd_written = nd_written;
  A.cnt = (uint32_t*)workspace; A.list = A.cnt + 8;
  hipStream_t st = (hipStream_t)stream;
  if (desc) ORBHIP_CHECK_HIP(hipMemsetAsync(A.cnt, 0, 32, st));
  hipLaunchKernelGGL(k_mp_prep, dim3((npts + MP_WG - 1) / MP_WG), dim3(MP_WG), 0, st, A);
  if (desc) hipLaunchKernelGGL(k_mp_desc, dim3(std::min(npts, 2048)), dim3(MP_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_update_map_points(int npts, const int32_t* obs_off, const double* X, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* pt_good,
                           int nobs, const int32_t* obs_kf, const uint8_t* obs_desc, const uint8_t* obs_kf_good, int nkf, const double* kf_center,
                           const float* scale_factors, int n_levels, int what, int32_t* best_obs, uint8_t* desc_out, double* normal, float* min_max,
                           uint8_t* nd_written) {
  using namespace orbhip;
  // every argument and every index is checked here, before any device work
  ORBHIP_REQUIRE(npts >= 0 && nobs >= 0 && nkf >= 0, ORBHIP_EINVAL, "orbl_update_map_points: negative count");
  ORBHIP_REQUIRE(what >= 1 && what <= (ORBL_MP_DESC | ORBL_MP_NORMAL_DEPTH), ORBHIP_EINVAL, "orbl_update_map_points: `what` selects nothing known");
  if (npts == 0) return 0;
  const bool desc = what & ORBL_MP_DESC, nd = what & ORBL_MP_NORMAL_DEPTH;
  ORBHIP_REQUIRE(obs_off, ORBHIP_EINVAL, "orbl_update_map_points: NULL obs_off");
  ORBHIP_REQUIRE(!desc || ((nobs == 0 || obs_desc) && best_obs && desc_out), ORBHIP_EINVAL, "orbl_update_map_points: NULL descriptor argument");
  ORBHIP_REQUIRE(!nd || (X && ref_kf && ref_level && (nobs == 0 || obs_kf) && (nkf == 0 || kf_center) && scale_factors && normal && min_max && nd_written),
                 ORBHIP_EINVAL, "orbl_update_map_points: NULL normal / depth argument");
  ORBHIP_REQUIRE(!nd || (n_levels > 0 && n_levels <= 64), ORBHIP_EINVAL, "orbl_update_map_points: n_levels out of range");
  static const char E[] = "orbl_update_map_points";
  int total = 0;
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &total));
  ORBHIP_REQUIRE(total == nobs, ORBHIP_EINVAL, "orbl_update_map_points: obs_off must run from 0 to nobs");
  if (nd) {
    ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
    const auto read = [&](int p) { return obs_off[p] != obs_off[p + 1] && !(pt_good && !pt_good[p]); };      // (a point left unchanged: its reference keyframe is not read)
    ORBHIP_ARG(check_index_if(E, "ref_kf", ref_kf, npts, nkf, read));
    ORBHIP_ARG(check_index_if(E, "ref_level", ref_level, npts, n_levels, read));
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t np = (size_t)npts, no = (size_t)nobs;
  RoundTrip R(W);
  const HostIn<int32_t> d_off = R.csr(obs_off, np), d_ref = R.in(nd ? ref_kf : nullptr, np), d_lvl = R.in(nd ? ref_level : nullptr, np), d_kf = R.in(nd ? obs_kf : nullptr, no);
  const HostIn<uint8_t> d_good = R.in(pt_good, np), d_desc = R.in(desc ? obs_desc : nullptr, 32 * no), d_kf_good = R.in(desc ? obs_kf_good : nullptr, no);
  const HostIn<double> d_X = R.in(nd ? X : nullptr, 3 * np), d_ctr = R.in(nd ? kf_center : nullptr, 3 * (size_t)nkf);
  const HostIn<float> d_sf = R.in(nd ? scale_factors : nullptr, (size_t)n_levels);
  const HostOut<int32_t> o_best = R.out<int32_t>(np);
  const HostOut<uint8_t> o_desc = R.out<uint8_t>(32 * np), o_wrote = R.out<uint8_t>(np);
  const HostOut<double> o_normal = R.out<double>(3 * np);
  const HostOut<float> o_mm = R.out<float>(2 * np);
  R.scratch(mp_workspace_bytes(npts));
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_update_map_points_device(npts, d_off.dev(), d_X.dev(), d_ref.dev(), d_lvl.dev(), d_good.dev(), nobs, d_kf.dev(), d_desc.dev(), d_kf_good.dev(), nkf,
                                          d_ctr.dev(), d_sf.dev(), n_levels, what, o_best.dev(), o_desc.dev(), o_normal.dev(), o_mm.dev(), o_wrote.dev(),
                                          R.scratch_dev(), R.stream()))) return rc;
  if ((rc = R.finish())) return rc;
  // only what the call wrote reaches the caller's buffers: unchanged points keep their bytes
  if (desc) {
    R.copy_out(o_best, best_obs, np);
    for (size_t p = 0; p < np; p++)
      if (o_best[p] >= 0) std::copy_n(&o_desc[32 * p], 32, desc_out + 32 * p);
  }
  if (nd) {
    R.copy_out(o_wrote, nd_written, np);
    for (size_t p = 0; p < np; p++)
      if (o_wrote[p]) { std::copy_n(&o_normal[3 * p], 3, normal + 3 * p); std::copy_n(&o_mm[2 * p], 2, min_max + 2 * p); }
  }
  return 0;
}

}  // extern "C"
