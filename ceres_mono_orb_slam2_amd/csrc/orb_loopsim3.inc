// orb_loopsim3.inc -- the front of LoopClosing::ComputeSim3 (src/LoopClosing.cc:250-277) on the resident map tables, for every candidate
// in one call (orbl_loop_sim3_candidates*): SearchByBoW(current keyframe, candidate) (src/ORBmatcher.cc:470-580), the `nmatches < 20`
// gate and what Sim3Solver's constructor builds (src/Sim3Solver.cc:73-109), packed as orbt_sim3_iterate_batch_device takes it.
// Textually included by orb_localmap.hip.
//
// SearchByBoW is sequential only inside one vocabulary node: the current keyframe's entries of the node, in list order, each take the
// closest entry of the candidate's list of that node which no earlier one took.  A keypoint stands in one node, so the (node,
// candidate) pairs are independent.  Three memsets and four kernels, the same whatever the sizes:
//   k_ls_bow      one wave per (node of the current keyframe, candidate), the nodes strided over LS_BOW_GX waves per candidate.  The wave
//                 finds the node in the candidate's ascending list by binary search (what the lower_bound merge of :498-560 arrives at)
//                 and walks as k_trf_bow (orb_track.hip) does: the candidate's first 256 entries in registers, four per lane, a tail
//                 beyond them from memory; every distance of a 64-entry slice of the current keyframe first, then the walk with a mask,
//                 two wave minima and the decision.  Distances are kept as 16-bit fields, so 256 stays 256 and the ratio test is exact
//                 for every nnratio.  The matches, their rotation bins and the bin counts (integer atomics: a sum) go out behind a slice.
//   k_ls_filter   one workgroup per candidate: ComputeThreeMaxima, the filter, nmatches, the gate, K1 / K2; for a kept candidate the
//                 constructor's row test per i1 - GetIndexInKeyFrame as a loop over the point's observation list - and the row count.
//   k_mt_scan_sums   the candidates' row counts -> off[].
//   k_ls_pack     one workgroup per candidate: the rows placed by an ordered scan over i1; a further workgroup writes off[n_cand] and
//                 counts[], the rest zero the rows behind the last one, so that every element of every output is written.
// No atomic decides a position; outputs are vector stores; nothing is written beyond cap1 or cap_rows.
#include "orb_maptable.h"

namespace orbhip {

#define LS_WG 256
#define LS_ST_OFFSETS 1u          /* *status bits of the device form */
#define LS_ST_KF 2u
#define LS_ST_PT 4u
#define LS_ST_LEVEL 8u
#define LS_ST_CAP 16u
#define LS_ST_SLOT 32u
#define LS_TH_LOW 50              /* ORBmatcher::TH_LOW */
#define LS_HISTO 30               /* ORBmatcher::HISTO_LENGTH */
#define LS_MAX_CAND 1024
#define LS_MAX_SLOTS ORBT_SIM3_MAX_N   /* slots of a keyframe that takes part: the rows of one candidate are at most that many */
#define LS_BOW_GX 128             /* k_ls_bow: waves per candidate */
#define LS_FILL_BX 32             /* k_ls_pack: workgroups that zero the unused rows */
#define LS_NOKEY 0xFFFFFFFFu

struct LsArgs {
  int cur_kf, n_cand, nkf, nslots, nfv, nent, npts, nobs, n_levels, check_ori, min_matches, cap1, cap_rows; float nnratio;
  const int32_t* cand_kf; const uint8_t* kf_bad; const double* kf_Tcw; const float* kf_K4;
  const int32_t *slot_off, *slot_pt, *slot_level; const float* slot_angle; const uint32_t* slot_desc;
  const int32_t* kf_fv_off; const uint32_t* fv_node; const int32_t *fv_ent_off, *fv_ent;
  const uint8_t* pt_bad; const double* pt_Xw; const int32_t *obs_off, *obs_kf, *obs_slot; const float* level_sigma2;
  int32_t *match12, *nmatches, *cand_status; float *K1, *K2; int32_t* off; double *X1c, *X2c; float *max_err1, *max_err2;
  int32_t *row_i1, *row_pt1, *row_pt2, *counts; uint32_t* status;
  int32_t* hist; uint8_t* bin; int32_t *ix1, *ix2, *cnt;         // workspace: [n_cand][32] | [n_cand][cap1] | 2 x [n_cand][cap1] | [n_cand + 1]
};

// the slots of keyframe k; false and no slots when k is no keyframe, its offsets are not usable or it has more than LS_MAX_SLOTS slots
__device__ __forceinline__ bool ls_slots(const LsArgs& a, int k, int* lo, int* n) {
  int hi;
  *lo = 0; *n = 0;
  if (k < 0 || k >= a.nkf) { mt_flag(a.status, LS_ST_KF); return false; }
  if (!mt_range(a.slot_off, k, a.nslots, lo, &hi)) { mt_flag(a.status, LS_ST_OFFSETS); return false; }
  if (hi - *lo > LS_MAX_SLOTS) { mt_flag(a.status, LS_ST_CAP); *lo = 0; return false; }
  *n = hi - *lo;
  return true;
}

// the current keyframe: its slots must fit a row of match12 as well
__device__ __forceinline__ bool ls_current(const LsArgs& a, int* lo, int* n) {
  if (!ls_slots(a, a.cur_kf, lo, n)) return false;
  if (*n > a.cap1) { mt_flag(a.status, LS_ST_CAP); *lo = 0; *n = 0; return false; }
  return true;
}

// candidate c: the keyframe that is searched, or -1 for one that is bad (src/LoopClosing.cc:257-260) or not usable
__device__ __forceinline__ int ls_candidate(const LsArgs& a, int c, int* lo, int* n) {
  const int k = a.cand_kf[c];
  if (!ls_slots(a, k, lo, n)) return -1;
  if (a.kf_bad && a.kf_bad[k]) { *lo = 0; *n = 0; return -1; }
  return k;
}

// the point of slot s (an index into the slot tables) when it takes part: in range and not bad (src/ORBmatcher.cc:503-505, :516-520)
__device__ __forceinline__ int ls_slot_point(const LsArgs& a, int s) {
  const int p = a.slot_pt[s];
  if (p < 0 || p >= a.npts) { if (p != -1) mt_flag(a.status, LS_ST_PT); return -1; }
  return a.pt_bad[p] ? -1 : p;
}

__device__ __forceinline__ bool ls_table_range(const LsArgs& a, const int32_t* off, int i, int total, int* lo, int* hi) {
  if (mt_range(off, i, total, lo, hi)) return true;
  mt_flag(a.status, LS_ST_OFFSETS);
  return false;
}

__device__ __forceinline__ unsigned ls_hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) +
         __popc(a1.w ^ b1.w);
}

__device__ __forceinline__ void ls_load_desc(const uint32_t* d, uint4* lo, uint4* hi) {        // (the table is 4-byte aligned, no more)
  lo->x = d[0]; lo->y = d[1]; lo->z = d[2]; lo->w = d[3]; hi->x = d[4]; hi->y = d[5]; hi->z = d[6]; hi->w = d[7];
}

__device__ __forceinline__ uint4 ls_readlane4(const uint4& v, int j) {
  uint4 r;
  r.x = __builtin_amdgcn_readlane(v.x, j); r.y = __builtin_amdgcn_readlane(v.y, j); r.z = __builtin_amdgcn_readlane(v.z, j); r.w = __builtin_amdgcn_readlane(v.w, j);
  return r;
}

// the smallest value of the wave on DPP alone (no LDS crossbar on the sequential path); the result leaves through lane 63
__device__ __forceinline__ unsigned ls_wave_min(unsigned v) {
  auto dpp = [](unsigned x, auto ctrl) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, 0xF, 0xF, false); };
  v = min(v, dpp(v, std::integral_constant<int, 0xB1>()));         // quad_perm [1,0,3,2]
  v = min(v, dpp(v, std::integral_constant<int, 0x4E>()));         // quad_perm [2,3,0,1]
  v = min(v, dpp(v, std::integral_constant<int, 0x141>()));        // row_half_mirror
  v = min(v, dpp(v, std::integral_constant<int, 0x140>()));        // row_mirror: every lane of a row holds the row's minimum
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)LS_NOKEY, (int)v, 0x142, 0xA, 0xF, false));        // row_bcast15 into rows 1 and 3
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)LS_NOKEY, (int)v, 0x143, 0xC, 0xF, false));        // row_bcast31 into rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ mt_u64 ls_wave_min64(mt_u64 v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const mt_u64 o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
  return v;
}

#define LS_LDS_FENCE() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)

// ------------------------------------------------------------------------------------------------------------------ the search
__global__ __launch_bounds__(64) void k_ls_bow(LsArgs a) {
  __shared__ uint2 s_dj[64][64];                                  // [entry of the slice][lane]: four distances, 16 bits each
  __shared__ int s_m2[64], s_mb[64];                              // per entry of the slice: the matched slot of the candidate (or -1), its rotation bin
  __shared__ uint32_t s_taken[LS_MAX_SLOTS / 32];                 // vbMatched2 of the entries behind the first 256, by slot
  const int lane = threadIdx.x, c = blockIdx.y;
  int s1lo, n1, s2lo, n2, f1lo, f1hi, f2lo, f2hi;
  if (!ls_current(a, &s1lo, &n1)) return;                         // (wave-uniform, as everything up to the loads of a slice)
  const int k2 = ls_candidate(a, c, &s2lo, &n2);
  if (k2 < 0) return;
  if (!ls_table_range(a, a.kf_fv_off, a.cur_kf, a.nfv, &f1lo, &f1hi) || !ls_table_range(a, a.kf_fv_off, k2, a.nfv, &f2lo, &f2hi)) return;
  int32_t* m_out = a.match12 + (size_t)c * a.cap1;
  uint8_t* b_out = a.bin + (size_t)c * a.cap1;
  int32_t* hist = a.hist + 32 * c;
  const float nnratio = a.nnratio;
  const int check_ori = a.check_ori;
  for (int m = blockIdx.x; m < f1hi - f1lo; m += gridDim.x) {
    const uint32_t node = a.fv_node[f1lo + m];
    int bl = f2lo, bh = f2hi - 1, m2 = -1;                        // the candidate's list of the same node (ascending node ids)
    while (bl <= bh) { const int q = (bl + bh) >> 1; const uint32_t v = a.fv_node[q]; if (v == node) { m2 = q; break; } if (v < node) bl = q + 1; else bh = q - 1; }
    if (m2 < 0) continue;
    int e1lo, e1hi, e2lo, e2hi;
    if (!ls_table_range(a, a.fv_ent_off, f1lo + m, a.nent, &e1lo, &e1hi) || !ls_table_range(a, a.fv_ent_off, m2, a.nent, &e2lo, &e2hi)) continue;
    const int cnt2 = e2hi - e2lo;
    if (cnt2 == 0 || e1hi == e1lo) continue;
    // the candidate's first 256 entries of the node stay in registers, four per lane (list positions lane, lane + 64, ...), with their
    // slots and angles and their vbMatched2 bits; an entry that cannot match (no point, a bad point, out of range) is never offered
    uint4 c0[4], c1[4];
    float a2_l[4]; int i2_l[4];
    unsigned have = 0, taken = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      c0[t] = make_uint4(0, 0, 0, 0); c1[t] = c0[t]; a2_l[t] = 0.f; i2_l[t] = -1;
      const int p = lane + 64 * t;
      if (p < cnt2) {
        const int i2 = a.fv_ent[e2lo + p];
        if (i2 < 0 || i2 >= n2) mt_flag(a.status, LS_ST_SLOT);
        else if (ls_slot_point(a, s2lo + i2) >= 0) {
          have |= 1u << t; i2_l[t] = i2; a2_l[t] = a.slot_angle[s2lo + i2];
          ls_load_desc(a.slot_desc + 8 * (size_t)(s2lo + i2), &c0[t], &c1[t]);
        }
      }
    }
    if (cnt2 > 256)
      for (int w = lane; w < LS_MAX_SLOTS / 32; w += 64) s_taken[w] = 0u;
    for (int e0 = e1lo; e0 < e1hi; e0 += 64) {
      const int ne = min(64, e1hi - e0);
      int q_l = -1;
      uint4 k0 = make_uint4(0, 0, 0, 0), k1v = k0;
      float ka_l = 0.f;
      if (lane < ne) {
        const int i1 = a.fv_ent[e0 + lane];
        if (i1 < 0 || i1 >= n1) mt_flag(a.status, LS_ST_SLOT);
        else if (ls_slot_point(a, s1lo + i1) >= 0) { q_l = i1; ka_l = a.slot_angle[s1lo + i1]; ls_load_desc(a.slot_desc + 8 * (size_t)(s1lo + i1), &k0, &k1v); }
      }
      s_m2[lane] = -1;
      // (A) every distance of the slice first: 64 independent entries, throughput-bound
      for (int j = 0; j < ne; j++) {
        if (__builtin_amdgcn_readlane(q_l, j) < 0) continue;
        const uint4 q0 = ls_readlane4(k0, j), q1 = ls_readlane4(k1v, j);
        unsigned d[4];
#pragma unroll
        for (int t = 0; t < 4; t++) d[t] = ls_hamming(q0, q1, c0[t], c1[t]);
        s_dj[j][lane] = make_uint2(d[0] | (d[1] << 16), d[2] | (d[3] << 16));
      }
      LS_LDS_FENCE();
      // (B) the walk, sequential by definition: per entry a mask, two wave minima, the decision
      for (int j = 0; j < ne; j++) {
        const int q = __builtin_amdgcn_readlane(q_l, j);
        if (q < 0) continue;
        const uint2 dq = s_dj[j][lane];
        const unsigned dd[4] = {dq.x & 0xFFFFu, dq.x >> 16, dq.y & 0xFFFFu, dq.y >> 16};
        unsigned k1 = 256u << 16, k2 = 256u << 16;                 // (distance << 16 | list position): the first minimum in list order
        const unsigned avail = have & ~taken;
#pragma unroll
        for (int t = 0; t < 4; t++) {                             // (selects, no branches)
          const unsigned key = ((avail >> t) & 1u) ? ((dd[t] << 16) | (unsigned)(lane + 64 * t)) : LS_NOKEY;
          const unsigned lo = min(key, k1), hi = max(key, k1);
          k1 = lo; k2 = min(k2, hi);
        }
        // the smallest key, then the smallest of what every lane has left without it (keys are unique: the position is part of them)
        const unsigned K1 = ls_wave_min(k1);
        const unsigned K2 = ls_wave_min(k1 == K1 ? k2 : k1);
        int best1 = (int)(K1 >> 16), best2 = (int)(K2 >> 16), pos1 = (int)(K1 & 0xFFFFu);
        bool in_tail = false;
        if (cnt2 > 256) {                                         // (a node with more than 256 entries on the candidate's side: the rest from memory)
          const uint4 q0 = ls_readlane4(k0, j), q1 = ls_readlane4(k1v, j);
          mt_u64 t1 = ~0ull, t2 = ~0ull;
          for (int p = lane + 256; p < cnt2; p += 64) {
            const int i2 = a.fv_ent[e2lo + p];
            if (i2 < 0 || i2 >= n2) { mt_flag(a.status, LS_ST_SLOT); continue; }
            if ((s_taken[i2 >> 5] >> (i2 & 31)) & 1u) continue;
            if (ls_slot_point(a, s2lo + i2) < 0) continue;
            uint4 b0, b1;
            ls_load_desc(a.slot_desc + 8 * (size_t)(s2lo + i2), &b0, &b1);
            const mt_u64 key = ((mt_u64)ls_hamming(q0, q1, b0, b1) << 32) | (mt_u64)(unsigned)p;
            if (key < t1) { t2 = t1; t1 = key; } else if (key < t2) t2 = key;
          }
          const mt_u64 T1 = ls_wave_min64(t1);
          const mt_u64 T2 = ls_wave_min64(t1 == T1 ? t2 : t1);
          const int td1 = T1 == ~0ull ? 256 : (int)(T1 >> 32), td2 = T2 == ~0ull ? 256 : (int)(T2 >> 32);
          if (td1 < best1) { best2 = min(best1, td2); best1 = td1; pos1 = (int)(unsigned)(T1 & 0xFFFFFFFFull); in_tail = true; }      // (equal: the earlier position, in the registers, wins)
          else best2 = min(best2, td1);
        }
        if (best1 < LS_TH_LOW && (float)best1 < nnratio * (float)best2) {     // (:535-537)
          const float ka = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ka_l), j));
          float a2; int i2;
          if (!in_tail) {
            const int t = pos1 >> 6, l = pos1 & 63;
            const float v = t == 0 ? a2_l[0] : (t == 1 ? a2_l[1] : (t == 2 ? a2_l[2] : a2_l[3]));
            const int vi = t == 0 ? i2_l[0] : (t == 1 ? i2_l[1] : (t == 2 ? i2_l[2] : i2_l[3]));
            a2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
            i2 = __builtin_amdgcn_readlane(vi, l);
            if (lane == l) taken |= 1u << t;
          } else {
            i2 = a.fv_ent[e2lo + pos1];
            a2 = a.slot_angle[s2lo + i2];
            if (lane == 0) s_taken[i2 >> 5] |= 1u << (i2 & 31);
          }
          if (lane == 0) {                                        // (recorded in LDS, written out behind the walk)
            int b = 0;
            if (check_ori) {                                      // (:541-548)
              float rot = ka - a2;
              if (rot < 0.0) rot += 360.0f;
              b = (int)roundf(rot * (1.0f / LS_HISTO));
              if (!(b >= 0 && b < LS_HISTO)) b = 0;                // (30 -> 0; an angle that is no angle lands there too)
            }
            s_m2[j] = i2; s_mb[j] = b;
          }
          LS_LDS_FENCE();
        }
      }
      LS_LDS_FENCE();
      if (lane < ne && q_l >= 0) {                                // the slice's matches, one lane each
        const int i2 = s_m2[lane];
        if (i2 >= 0) {
          m_out[q_l] = i2;
          if (check_ori) { const int b = s_mb[lane]; b_out[q_l] = (uint8_t)b; atomicAdd(&hist[b], 1); }
        }
      }
      LS_LDS_FENCE();
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ filter, gate, rows
// MapPoint::GetIndexInKeyFrame on the observation tables: obs_slot of the first entry of p's list that names keyframe k, a slot of
// k's row; -1 when there is none.  An entry out of range is absent.
__device__ __forceinline__ int ls_index_in_keyframe(const LsArgs& a, int p, int k, int nk) {
  int lo, hi;
  if (!ls_table_range(a, a.obs_off, p, a.nobs, &lo, &hi)) return -1;
  for (int e = lo; e < hi; e++) {
    const int ok = a.obs_kf[e];
    if (ok < 0 || ok >= a.nkf) { mt_flag(a.status, LS_ST_KF); continue; }
    if (ok != k) continue;
    const int s = a.obs_slot[e];
    if (s < 0 || s >= nk) { mt_flag(a.status, LS_ST_SLOT); continue; }
    return s;
  }
  return -1;
}

__global__ __launch_bounds__(LS_WG) void k_ls_filter(LsArgs a) {
  __shared__ int sw[LS_WG / 64];
  __shared__ int s_top[3];
  const int c = blockIdx.x, tid = threadIdx.x;
  int s1lo, n1, s2lo, n2;
  const bool cur_ok = ls_current(a, &s1lo, &n1);
  const int k2 = ls_candidate(a, c, &s2lo, &n2);
  int32_t* m12 = a.match12 + (size_t)c * a.cap1;
  const uint8_t* bins = a.bin + (size_t)c * a.cap1;
  int32_t* ix1 = a.ix1 + (size_t)c * a.cap1;
  int32_t* ix2 = a.ix2 + (size_t)c * a.cap1;
  if (tid < 4) {
    a.K1[4 * (size_t)c + tid] = cur_ok ? a.kf_K4[4 * (size_t)a.cur_kf + tid] : 0.f;
    a.K2[4 * (size_t)c + tid] = k2 >= 0 ? a.kf_K4[4 * (size_t)k2 + tid] : 0.f;
  }
  if (tid == 0) {                                                 // ComputeThreeMaxima (src/ORBmatcher.cc:1386-1418): strict '>', the earlier bin wins ties
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    const int32_t* h = a.hist + 32 * c;
    for (int i = 0; i < LS_HISTO; i++) {
      const int s = h[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
      else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
    s_top[0] = i1; s_top[1] = i2; s_top[2] = i3;
  }
  __syncthreads();
  const int t0 = s_top[0], t1 = s_top[1], t2 = s_top[2];
  int nm = 0;
  for (int i0 = 0; i0 < n1; i0 += LS_WG) {                         // (:570-576) the matches of the other bins are cleared; their vbMatched2 stayed set
    const int i = i0 + tid;
    bool on = false;
    if (i < n1 && m12[i] >= 0) {
      const int b = bins[i];
      if (a.check_ori && b != t0 && b != t1 && b != t2) m12[i] = -1; else on = true;
    }
    int tot;
    mt_block_excl<LS_WG>(on ? 1 : 0, sw, &tot);
    nm += tot;
  }
  const int st = k2 < 0 ? 1 : (nm < a.min_matches ? 2 : 0);       // (src/LoopClosing.cc:257-267)
  int rows = 0;
  if (st == 0) {
    const int lvl_max = a.n_levels;
    for (int i0 = 0; i0 < n1; i0 += LS_WG) {                       // (src/Sim3Solver.cc:73-85) which i1 become rows, and with which keypoints
      const int i = i0 + tid;
      int x1 = -1, x2 = -1;
      if (i < n1 && m12[i] >= 0) {
        const int p1 = ls_slot_point(a, s1lo + i), p2 = m12[i] < n2 ? ls_slot_point(a, s2lo + m12[i]) : -1;
        if (p1 >= 0 && p2 >= 0) {
          x1 = ls_index_in_keyframe(a, p1, a.cur_kf, n1);
          x2 = ls_index_in_keyframe(a, p2, k2, n2);
          if (x1 >= 0 && x2 >= 0) {
            const int l1 = a.slot_level[s1lo + x1], l2 = a.slot_level[s2lo + x2];
            if (l1 < 0 || l1 >= lvl_max || l2 < 0 || l2 >= lvl_max) { mt_flag(a.status, LS_ST_LEVEL); x1 = -1; }
          }
        }
      }
      const bool row = x1 >= 0 && x2 >= 0;
      if (i < n1) { ix1[i] = row ? x1 : -1; ix2[i] = row ? x2 : -1; }
      int tot;
      mt_block_excl<LS_WG>(row ? 1 : 0, sw, &tot);
      rows += tot;
    }
  }
  if (tid == 0) { a.nmatches[c] = k2 < 0 ? 0 : nm; a.cand_status[c] = st; a.cnt[c] = rows; }
}

// max_errors_1_ / _2_ (src/Sim3Solver.cc:93-94): the double product in a std::vector<size_t>, read back as float
__device__ __forceinline__ float ls_max_err(float sigma2) { return (float)(unsigned long long)(9.210 * (double)sigma2); }

__global__ __launch_bounds__(LS_WG) void k_ls_pack(LsArgs a) {
  __shared__ int sw[LS_WG / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int total = a.cnt[a.n_cand];
  if (c == a.n_cand) {                                            // the totals
    if (tid == 0) {
      int kept = 0;
      for (int q = 0; q < a.n_cand; q++) kept += a.cand_status[q] == 0 ? 1 : 0;
      a.off[a.n_cand] = total; a.counts[0] = total; a.counts[1] = kept;
      if (total > a.cap_rows) mt_flag(a.status, LS_ST_CAP);
    }
    return;
  }
  if (c > a.n_cand) {                                             // the rows nobody fills
    for (size_t r = (size_t)total + (size_t)(c - a.n_cand - 1) * LS_WG + tid; r < (size_t)a.cap_rows; r += (size_t)LS_FILL_BX * LS_WG) {
      for (int q = 0; q < 3; q++) { a.X1c[3 * r + q] = 0.0; a.X2c[3 * r + q] = 0.0; }
      a.max_err1[r] = 0.f; a.max_err2[r] = 0.f; a.row_i1[r] = -1; a.row_pt1[r] = -1; a.row_pt2[r] = -1;
    }
    return;
  }
  const int base = a.cnt[c];
  if (tid == 0) a.off[c] = base;
  if (a.cand_status[c] != 0) return;                              // (workgroup-uniform)
  int s1lo, n1, s2lo, n2;
  ls_current(a, &s1lo, &n1);
  const int k2 = ls_candidate(a, c, &s2lo, &n2);
  const int32_t* m12 = a.match12 + (size_t)c * a.cap1;
  const int32_t* ix1 = a.ix1 + (size_t)c * a.cap1;
  const int32_t* ix2 = a.ix2 + (size_t)c * a.cap1;
  int carry = 0;
  for (int i0 = 0; i0 < n1; i0 += LS_WG) {                         // (workgroup-uniform) rows in the order of i1 (:73)
    const int i = i0 + tid;
    const bool row = i < n1 && ix1[i] >= 0;
    int tot;
    const int ex = mt_block_excl<LS_WG>(row ? 1 : 0, sw, &tot);
    const size_t r = (size_t)base + (size_t)(carry + ex);
    if (row && r < (size_t)a.cap_rows) {
      const int p1 = a.slot_pt[s1lo + i], p2 = a.slot_pt[s2lo + m12[i]];
      double X[3];
      mc_apply34(a.kf_Tcw + 12 * (size_t)a.cur_kf, a.pt_Xw + 3 * (size_t)p1, X);      // (:100-104) Rcw X + tcw
      for (int q = 0; q < 3; q++) a.X1c[3 * r + q] = X[q];
      mc_apply34(a.kf_Tcw + 12 * (size_t)k2, a.pt_Xw + 3 * (size_t)p2, X);
      for (int q = 0; q < 3; q++) a.X2c[3 * r + q] = X[q];
      a.max_err1[r] = ls_max_err(a.level_sigma2[a.slot_level[s1lo + ix1[i]]]);
      a.max_err2[r] = ls_max_err(a.level_sigma2[a.slot_level[s2lo + ix2[i]]]);
      a.row_i1[r] = i; a.row_pt1[r] = p1; a.row_pt2[r] = p2;
    }
    carry += tot;
  }
}

// workspace sections, each rounded up to 256 bytes; [0, hist_end) is zeroed by every call
struct LsWs { size_t hist, hist_end, bin, ix1, ix2, cnt, total; };
static LsWs ls_workspace(int n_cand, int cap1) {
  LsWs w; Carve ws;
  const size_t nc = (size_t)n_cand, rows = nc * (size_t)cap1;
  w.hist = ws.take(4 * 32 * nc);
  w.hist_end = ws.total;
  w.bin = ws.take(rows); w.ix1 = ws.take(4 * rows); w.ix2 = ws.take(4 * rows); w.cnt = ws.take(4 * (nc + 1));
  w.total = ws.total;
  return w;
}

static int ls_check_sizes(int n_cand, int cap1, int cap_rows) {
  ORBHIP_REQUIRE(n_cand >= 1 && n_cand <= LS_MAX_CAND, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: n_cand must be in [1, 1024]");
  ORBHIP_REQUIRE(cap1 >= 0 && cap1 <= LS_MAX_SLOTS, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: cap1 must be in [0, 32768]");
  ORBHIP_REQUIRE(cap_rows >= 0 && (long long)cap_rows <= (long long)LS_MAX_SLOTS * n_cand, ORBHIP_EINVAL,
                 "orbl_loop_sim3_candidates: cap_rows must be in [0, 32768 n_cand]");
  return 0;
}

}  // namespace orbhip

extern "C" {

int orbl_loop_sim3_candidates_workspace(int n_cand, int cap1, size_t* bytes) {
  using namespace orbhip;
  ORBHIP_REQUIRE(bytes, ORBHIP_EINVAL, "orbl_loop_sim3_candidates_workspace: NULL bytes");
  if (int rc = ls_check_sizes(n_cand, cap1, 0)) return rc;
  *bytes = ls_workspace(n_cand, cap1).total;
  return 0;
}

int orbl_loop_sim3_candidates_device(int cur_kf, int n_cand, const int32_t* cand_kf, int nkf, const uint8_t* kf_bad, const double* kf_Tcw, const float* kf_K4, int nslots,
                                     const int32_t* kf_slot_off, const int32_t* kf_slot_pt, const int32_t* kf_slot_level, const float* kf_slot_angle,
                                     const uint8_t* kf_slot_desc, int nfv, const int32_t* kf_fv_off, const uint32_t* fv_node, int nent, const int32_t* fv_ent_off,
                                     const int32_t* fv_ent, int npts, const uint8_t* pt_bad, const double* pt_Xw, int nobs, const int32_t* obs_off, const int32_t* obs_kf,
                                     const int32_t* obs_slot, const float* level_sigma2, int n_levels, float nnratio, int check_ori, int min_matches, int cap1, int cap_rows,
                                     int32_t* match12, int32_t* nmatches, int32_t* cand_status, float* K1, float* K2, int32_t* off, double* X1c, double* X2c,
                                     float* max_err1, float* max_err2, int32_t* row_i1, int32_t* row_pt1, int32_t* row_pt2, int32_t* counts, uint32_t* status,
                                     void* workspace, void* stream) {
  using namespace orbhip;
  static const char M[] = "orbl_loop_sim3_candidates: NULL argument";
  if (int rc = ls_check_sizes(n_cand, cap1, cap_rows)) return rc;
  ORBHIP_REQUIRE(nkf >= 0 && nslots >= 0 && nfv >= 0 && nent >= 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: negative count");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: n_levels out of range");
  ORBHIP_REQUIRE(nnratio > 0.f, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: nnratio must be positive");
  ORBHIP_REQUIRE(workspace && cand_kf && kf_slot_off && kf_fv_off && fv_ent_off && obs_off && level_sigma2, ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(nkf == 0 || (kf_Tcw && kf_K4), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(nslots == 0 || (kf_slot_pt && kf_slot_level && kf_slot_angle && kf_slot_desc), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE((nfv == 0 || fv_node) && (nent == 0 || fv_ent) && (npts == 0 || (pt_bad && pt_Xw)) && (nobs == 0 || (obs_kf && obs_slot)), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(nmatches && cand_status && K1 && K2 && off && counts && (cap1 == 0 || match12), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(cap_rows == 0 || (X1c && X2c && max_err1 && max_err2 && row_i1 && row_pt1 && row_pt2), ORBHIP_EINVAL, M);
  const void* words[] = {cand_kf, kf_K4, kf_slot_off, kf_slot_pt, kf_slot_level, kf_slot_angle, kf_slot_desc, kf_fv_off, fv_node, fv_ent_off, fv_ent, obs_off, obs_kf,
                         obs_slot, level_sigma2, match12, nmatches, cand_status, K1, K2, off, max_err1, max_err2, row_i1, row_pt1, row_pt2, counts, status};
  for (const void* q : words) ORBHIP_REQUIRE((uintptr_t)q % 4 == 0, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: 32-bit arrays and the descriptor table must be 4-byte aligned");
  const void* dwords[] = {kf_Tcw, pt_Xw, X1c, X2c};
  for (const void* q : dwords) ORBHIP_REQUIRE((uintptr_t)q % 8 == 0, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: 64-bit arrays must be 8-byte aligned");
  ORBHIP_REQUIRE((uintptr_t)workspace % 8 == 0, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: the workspace must be 8-byte aligned");
  const LsWs ws = ls_workspace(n_cand, cap1);
  uint8_t* wb = (uint8_t*)workspace;
  LsArgs A;
  A.cur_kf = cur_kf; A.n_cand = n_cand; A.nkf = nkf; A.nslots = nslots; A.nfv = nfv; A.nent = nent; A.npts = npts; A.nobs = nobs; A.n_levels = n_levels;
  A.check_ori = check_ori; A.min_matches = min_matches; A.cap1 = cap1; A.cap_rows = cap_rows; A.nnratio = nnratio;
  A.cand_kf = cand_kf; A.kf_bad = kf_bad; A.kf_Tcw = kf_Tcw; A.kf_K4 = kf_K4; A.slot_off = kf_slot_off; A.slot_pt = kf_slot_pt; A.slot_level = kf_slot_level;
  A.slot_angle = kf_slot_angle; A.slot_desc = (const uint32_t*)kf_slot_desc; A.kf_fv_off = kf_fv_off; A.fv_node = fv_node; A.fv_ent_off = fv_ent_off; A.fv_ent = fv_ent;
  A.pt_bad = pt_bad; A.pt_Xw = pt_Xw; A.obs_off = obs_off; A.obs_kf = obs_kf; A.obs_slot = obs_slot; A.level_sigma2 = level_sigma2;
  A.match12 = match12; A.nmatches = nmatches; A.cand_status = cand_status; A.K1 = K1; A.K2 = K2; A.off = off; A.X1c = X1c; A.X2c = X2c; A.max_err1 = max_err1;
  A.max_err2 = max_err2; A.row_i1 = row_i1; A.row_pt1 = row_pt1; A.row_pt2 = row_pt2; A.counts = counts; A.status = status;
  A.hist = (int32_t*)(wb + ws.hist); A.bin = wb + ws.bin; A.ix1 = (int32_t*)(wb + ws.ix1); A.ix2 = (int32_t*)(wb + ws.ix2); A.cnt = (int32_t*)(wb + ws.cnt);
  hipStream_t st = (hipStream_t)stream;
  if (status) ORBHIP_CHECK_HIP(hipMemsetAsync(status, 0, 4, st));
  ORBHIP_CHECK_HIP(hipMemsetAsync(wb + ws.hist, 0, ws.hist_end - ws.hist, st));
  if (cap1 > 0) ORBHIP_CHECK_HIP(hipMemsetAsync(match12, 0xFF, 4 * (size_t)n_cand * (size_t)cap1, st));        // (-1: no match)
  hipLaunchKernelGGL(k_ls_bow, dim3(LS_BOW_GX, n_cand), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_ls_filter, dim3(n_cand), dim3(LS_WG), 0, st, A);
  hipLaunchKernelGGL(k_mt_scan_sums<int32_t>, dim3(1), dim3(MT_SUM_WG), 0, st, A.cnt, n_cand);
  hipLaunchKernelGGL(k_ls_pack, dim3(n_cand + 1 + LS_FILL_BX), dim3(LS_WG), 0, st, A);
  ORBHIP_CHECK_HIP(hipGetLastError());
  return 0;
}

int orbl_loop_sim3_candidates(int cur_kf, int n_cand, const int32_t* cand_kf, int nkf, const uint8_t* kf_bad, const double* kf_Tcw, const float* kf_K4,
                              const int32_t* kf_slot_off, const int32_t* kf_slot_pt, const int32_t* kf_slot_level, const float* kf_slot_angle, const uint8_t* kf_slot_desc,
                              const int32_t* kf_fv_off, const uint32_t* fv_node, const int32_t* fv_ent_off, const int32_t* fv_ent, int npts, const uint8_t* pt_bad,
                              const double* pt_Xw, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot, const float* level_sigma2, int n_levels,
                              float nnratio, int check_ori, int min_matches, int cap1, int cap_rows, int32_t* match12, int32_t* nmatches, int32_t* cand_status, float* K1,
                              float* K2, int32_t* off, double* X1c, double* X2c, float* max_err1, float* max_err2, int32_t* row_i1, int32_t* row_pt1, int32_t* row_pt2,
                              int32_t* counts) {
  using namespace orbhip;
  static const char E[] = "orbl_loop_sim3_candidates";
  static const char M[] = "orbl_loop_sim3_candidates: NULL argument";
  if (int rc = ls_check_sizes(n_cand, cap1, cap_rows)) return rc;
  ORBHIP_REQUIRE(nkf >= 1 && npts >= 0, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: nkf must be positive and npts not negative");
  ORBHIP_REQUIRE(cur_kf >= 0 && cur_kf < nkf, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: cur_kf is out of range");
  ORBHIP_REQUIRE(n_levels > 0 && n_levels <= 64, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: n_levels out of range");
  ORBHIP_REQUIRE(nnratio > 0.f, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: nnratio must be positive");
  ORBHIP_REQUIRE(cand_kf && kf_Tcw && kf_K4 && kf_slot_off && kf_fv_off && level_sigma2 && (npts == 0 || (pt_bad && pt_Xw && obs_off)), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(nmatches && cand_status && K1 && K2 && off && counts && (cap1 == 0 || match12), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(cap_rows == 0 || (X1c && X2c && max_err1 && max_err2 && row_i1 && row_pt1 && row_pt2), ORBHIP_EINVAL, M);
  ORBHIP_ARG(check_index(E, "cand_kf", cand_kf, n_cand, nkf));
  int nslots = 0, nfv = 0, nent = 0, nobs = 0;
  ORBHIP_ARG(check_csr(E, "kf_slot_off", kf_slot_off, nkf, &nslots));
  ORBHIP_ARG(check_csr(E, "kf_fv_off", kf_fv_off, nkf, &nfv));
  ORBHIP_REQUIRE(nslots == 0 || (kf_slot_pt && kf_slot_level && kf_slot_angle && kf_slot_desc), ORBHIP_EINVAL, M);
  ORBHIP_REQUIRE(nfv == 0 || (fv_node && fv_ent_off), ORBHIP_EINVAL, M);
  ORBHIP_ARG(check_csr(E, "fv_ent_off", fv_ent_off, nfv, &nent));
  ORBHIP_ARG(check_csr(E, "obs_off", obs_off, npts, &nobs));
  ORBHIP_REQUIRE((nent == 0 || fv_ent) && (nobs == 0 || (obs_kf && obs_slot)), ORBHIP_EINVAL, M);
  ORBHIP_ARG(check_index(E, "kf_slot_pt", kf_slot_pt, nslots, npts, true));
  ORBHIP_ARG(check_index(E, "kf_slot_level", kf_slot_level, nslots, n_levels));
  ORBHIP_ARG(check_index(E, "obs_kf", obs_kf, nobs, nkf));
  for (int e = 0; e < nobs; e++)
    ORBHIP_REQUIRE(obs_slot[e] >= 0 && obs_slot[e] < kf_slot_off[obs_kf[e] + 1] - kf_slot_off[obs_kf[e]], ORBHIP_EINVAL,
                   "orbl_loop_sim3_candidates: an obs_slot lies outside its keyframe's slots");
  // a keyframe's feature vector: node ids ascending, every entry a slot of the keyframe, named once (a keypoint stands in one node)
  std::vector<uint8_t> seen;
  for (int k = 0; k < nkf; k++) {
    const int ns = kf_slot_off[k + 1] - kf_slot_off[k];
    seen.assign((size_t)ns, 0);
    for (int m = kf_fv_off[k]; m < kf_fv_off[k + 1]; m++) {
      ORBHIP_REQUIRE(m == kf_fv_off[k] || fv_node[m - 1] < fv_node[m], ORBHIP_EINVAL, "orbl_loop_sim3_candidates: fv_node must ascend inside a keyframe");
      for (int e = fv_ent_off[m]; e < fv_ent_off[m + 1]; e++) {
        ORBHIP_REQUIRE(fv_ent[e] >= 0 && fv_ent[e] < ns, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: an fv_ent lies outside its keyframe's slots");
        ORBHIP_REQUIRE(!seen[fv_ent[e]], ORBHIP_EINVAL, "orbl_loop_sim3_candidates: a feature vector names a keypoint twice");
        seen[fv_ent[e]] = 1;
      }
    }
  }
  const int n1 = kf_slot_off[cur_kf + 1] - kf_slot_off[cur_kf];
  ORBHIP_REQUIRE(n1 <= LS_MAX_SLOTS, ORBHIP_EINVAL, "orbl_loop_sim3_candidates: the current keyframe has more than 32768 slots");
  for (int c = 0; c < n_cand; c++)
    ORBHIP_REQUIRE(kf_slot_off[cand_kf[c] + 1] - kf_slot_off[cand_kf[c]] <= LS_MAX_SLOTS, ORBHIP_EINVAL,
                   "orbl_loop_sim3_candidates: a candidate keyframe has more than 32768 slots");
  if (n1 > cap1) {
    counts[0] = 0; counts[1] = 0;
    set_error("orbl_loop_sim3_candidates: the current keyframe has %d slots; cap1 is %d", n1, cap1);
    return ORBHIP_ECAP;
  }
  ThreadWs& W = thread_ws();
  int rc = W.begin();
  if (rc) return rc;
  const size_t nc = (size_t)n_cand, nk = (size_t)nkf, ns = (size_t)nslots, nf = (size_t)nfv, ne = (size_t)nent, np = (size_t)npts, no = (size_t)nobs;
  const size_t c1 = (size_t)cap1, cr = (size_t)cap_rows;
  RoundTrip R(W);
  const HostIn<int32_t> d_cand = R.in(cand_kf, nc), d_soff = R.csr(kf_slot_off, nk), d_spt = R.in(kf_slot_pt, ns), d_lvl = R.in(kf_slot_level, ns);
  const HostIn<int32_t> d_foff = R.csr(kf_fv_off, nk), d_eoff = R.csr(fv_ent_off ? fv_ent_off : &R.zero, nf), d_ent = R.in(fv_ent, ne);
  const HostIn<int32_t> d_ooff = R.csr(obs_off ? obs_off : &R.zero, np), d_okf = R.in(obs_kf, no), d_oslot = R.in(obs_slot, no);
  const HostIn<uint32_t> d_node = R.in(fv_node, nf);
  const HostIn<uint8_t> d_kbad = R.in(kf_bad, nk), d_desc = R.in(kf_slot_desc, 32 * ns), d_pbad = R.in(pt_bad, np);
  const HostIn<double> d_T = R.in(kf_Tcw, 12 * nk), d_X = R.in(pt_Xw, 3 * np);
  const HostIn<float> d_K4 = R.in(kf_K4, 4 * nk), d_ang = R.in(kf_slot_angle, ns), d_sig = R.in(level_sigma2, (size_t)n_levels);
  const HostOut<int32_t> o_m12 = R.out<int32_t>(nc * c1), o_nm = R.out<int32_t>(nc), o_st = R.out<int32_t>(nc), o_off = R.out<int32_t>(nc + 1), o_counts = R.out<int32_t>(2);
  const HostOut<int32_t> o_i1 = R.out<int32_t>(cr), o_p1 = R.out<int32_t>(cr), o_p2 = R.out<int32_t>(cr);
  const HostOut<float> o_K1 = R.out<float>(4 * nc), o_K2 = R.out<float>(4 * nc), o_e1 = R.out<float>(cr), o_e2 = R.out<float>(cr);
  const HostOut<double> o_X1 = R.out<double>(3 * cr), o_X2 = R.out<double>(3 * cr);
  const HostOut<uint32_t> o_bits = R.out<uint32_t>(1);
  R.scratch(ls_workspace(n_cand, cap1).total);
  if ((rc = R.commit())) return rc;
  if ((rc = orbl_loop_sim3_candidates_device(cur_kf, n_cand, d_cand.dev(), nkf, d_kbad.dev(), d_T.dev(), d_K4.dev(), nslots, d_soff.dev(), d_spt.dev(), d_lvl.dev(),
                                             d_ang.dev(), d_desc.dev(), nfv, d_foff.dev(), d_node.dev(), nent, d_eoff.dev(), d_ent.dev(), npts, d_pbad.dev(), d_X.dev(), nobs,
                                             d_ooff.dev(), d_okf.dev(), d_oslot.dev(), d_sig.dev(), n_levels, nnratio, check_ori, min_matches, cap1, cap_rows, o_m12.dev(),
                                             o_nm.dev(), o_st.dev(), o_K1.dev(), o_K2.dev(), o_off.dev(), o_X1.dev(), o_X2.dev(), o_e1.dev(), o_e2.dev(), o_i1.dev(),
                                             o_p1.dev(), o_p2.dev(), o_counts.dev(), o_bits.dev(), R.scratch_dev(), R.stream())))
    return rc;
  if ((rc = R.finish())) return rc;
  R.copy_out(o_counts, counts, 2);
  if (o_counts[0] > cap_rows) {
    set_error("orbl_loop_sim3_candidates: wanted %d rows; capacity %d", o_counts[0], cap_rows);
    return ORBHIP_ECAP;
  }
  R.copy_out(o_m12, match12, nc * c1); R.copy_out(o_nm, nmatches, nc); R.copy_out(o_st, cand_status, nc); R.copy_out(o_off, off, nc + 1);
  R.copy_out(o_K1, K1, 4 * nc); R.copy_out(o_K2, K2, 4 * nc); R.copy_out(o_X1, X1c, 3 * cr); R.copy_out(o_X2, X2c, 3 * cr); R.copy_out(o_e1, max_err1, cr);
  R.copy_out(o_e2, max_err2, cr); R.copy_out(o_i1, row_i1, cr); R.copy_out(o_p1, row_pt1, cr); R.copy_out(o_p2, row_pt2, cr);
  return 0;
}

}  // extern "C"
