// ============================================================================
// orb_relocrefine.inc -- part of the translation unit orb_track.hip (textually included there; not compiled on its own).
// Tracking::Relocalization behind a PnP pose (reference src/Tracking.cc:1056-1126) for every candidate of a `while` round in one
// call on the resident frame: orbt_relocalization_refine (include/orbslam_hip.h).
//
//   PoseOptimization -> [nGood < 10: out] -> outlier slots cleared -> [nGood >= 50: matched]
//   -> SearchByProjection(F, KF, found = the PnP inliers, 10, 100) -> [nadditional + nGood < 50: out] -> PoseOptimization
//   -> [nGood >= 50: matched] [nGood <= 30: out] -> SearchByProjection(F, KF, found, 3, 64) inside the loop over the slots
//   -> [nGood + nadditional < 50: out] -> PoseOptimization -> outlier slots cleared -> matched iff nGood >= 50
//
// The launches, the same 14 for any number of candidates, features and keyframe points:
//   k_rr_step<0>  one workgroup per candidate: the slots, the first problem's row count
//   k_rr_gather   one workgroup per candidate: the rows of ALL candidates' problems side by side (k_pose_lm reads them as CSR)
//   k_pose_lm     one workgroup per candidate (ba_solver.hip); a candidate that is out has no rows, its pose is left alone
//   k_rr_project  one lane per (candidate, keyframe point): projection with the solved pose, the gates of :1296-1321, PredictScale
//   k_trk_windows one wave per (candidate, keyframe point): window candidates on the resident grid, distances, compacted lists
//   k_rr_step<1>  the gates behind the first solve, the wide search's order-dependent pass, rotation check, the second row count
//   k_rr_gather, k_pose_lm, k_rr_project (th 3), k_trk_windows (64)
//   k_rr_step<2>  the gates behind the second solve, the narrow search's passes (below), the third row count
//   k_rr_gather, k_pose_lm
//   k_rr_step<3>  the outlier slots cleared behind the third solve, the final stage
//
// The order-dependent pass (src/ORBmatcher.cc:1289-1363).  The keyframe's points are walked in index order; point q takes the closest
// feature of its window whose slot is empty (first minimum in candidate order) if that distance is <= ORBdist, and every assignment
// closes the feature.  What q decides depends only on EARLIER points that list one of q's acceptable candidates, so - as in
// k_tlm_greedy - every round each feature records the smallest unsettled point that lists it and a point is settled when it is that
// smallest point for every feature on its list; the earliest unsettled point always is.  Only candidates within ORBdist are listed
// (k_trk_windows' dmax): the minimum over the free features is <= ORBdist iff a free listed one exists, and it is the same feature.
//
// The narrow search inside the loop (:1097-1104).  The pose is fixed there, so a pass reads only the slots and `found`: a pass that
// assigns nothing leaves the slots alone and returns 0, and every later pass - `found` only grows - is empty too.  The passes are
// run in order, each with `found` as it stands at its ip, up to the first empty one; nadditional is the net count of pass N_ - 1 if
// that pass ran, else 0.  A non-empty pass keeps at least one match (ComputeThreeMaxima always keeps the first fullest bin), so at
// most as many passes run as there are empty slots.
// ============================================================================

namespace orbhip {

struct RrIn { float K4[4], bounds[4], scale[16], inv_sigma2[16]; float log_scale; int nlevels, check_ori, narrow_in_loop, n_cand, n_kp, icap, ntot; };
struct RrCand { int off, n, has_pose, pad; double pose7[7]; double pad2; };      // off: the candidate's first row in the concatenated keyframe arrays
// per candidate, part of the download block.  live: the row count of the solve that is pending (-1: none - the candidate is out or matched)
struct RrState { int stage, matched, narrow_passes, live; int n_good[3], n_add[2], n_corr[3]; };
#define RR_RUNNING (-1)
// Full window lists (k_trk_windows writes one for a point with more than TRK_LMAX acceptable candidates) need more than 16 features of
// three pyramid levels inside a window of at most 10 scale pixels: the extractor spreads its features evenly, so only a small image
// with thousands of look-alike features has such windows.  Nothing is reserved for them up front; a frame that has some raises the
// thread's high-water mark and the call runs once more.
#define RR_PAIRS_PER_QUERY 0u

// PoseOptimization's return value: 0 below 3 correspondences (src/CeresOptimizer.cc:330)
__device__ __forceinline__ int rr_ngood(int n_corr, int n_inl) { return n_corr < 3 ? 0 : n_inl; }
// whether the search behind solve k (0: wide, 1: narrow) runs: the gates of :1076, :1084 and :1095
__device__ __forceinline__ bool rr_search_runs(const RrState& S, int k, int n_inl) {
  if (S.stage != RR_RUNNING || S.live < 0) return false;
  const int g = rr_ngood(S.live, n_inl);
  return k == 0 ? (S.live >= 3 && g >= 10 && g < 50) : (g > 30 && g < 50);
}

// inclusive scan over the 1024 threads of a workgroup (s_w: 16 ints; ends with every thread past the last read of s_w)
__device__ __forceinline__ int rr_scan1024(int v, int* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
  __syncthreads();
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; k++) base += s_w[k];
  return inc + base;
}

// Matrix_7_1_ToMatrix4d (ba_pose7_to_matrix4d, the same operations in the same order): R, t of the pose the solver left
__device__ __forceinline__ void rr_pose_to_Rt(const double* p, double* R, double* t) {
  const double n = sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]);
  const double q[4] = {p[3] / n, p[4] / n, p[5] / n, p[6] / n};
  quat_to_R(q, R);
  t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
}

// one lane per (candidate, keyframe point): src/ORBmatcher.cc:1292-1321 without the `found` test (the pass applies it: the windows do
// not depend on it, so the narrow loop's passes share one set of lists)
__global__ __launch_bounds__(256) void k_rr_project(const RrIn* __restrict__ in, const RrCand* __restrict__ cand, const RrState* __restrict__ state,
                                                    const int32_t* __restrict__ n_inl, const double* __restrict__ poses, const int32_t* __restrict__ rep,
                                                    const double* __restrict__ Xw, const float* __restrict__ mind, const float* __restrict__ maxd, const int which,
                                                    const float th, float* __restrict__ q_uv, float* __restrict__ q_r, int32_t* __restrict__ q_lo,
                                                    int32_t* __restrict__ q_hi, uint8_t* __restrict__ q_valid, uint32_t* __restrict__ list_total) {
  const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (c == 0 && i == 0) *list_total = 0u;
  const RrCand C = cand[c];
  if (i >= C.n) return;
  const int g = C.off + i;
  float u = 0.f, v = 0.f, r = 0.f; int lvl = 0; bool ok = false;
  if (rep[g] >= 0 && rr_search_runs(state[c], which, n_inl[c])) {
    double R[9], t[3];
    rr_pose_to_Rt(poses + 7 * c, R, t);
    const double X = Xw[3 * (size_t)g], Y = Xw[3 * (size_t)g + 1], Z = Xw[3 * (size_t)g + 2];
    const double cx3 = (R[0] * X + R[1] * Y + R[2] * Z) + t[0], cy3 = (R[3] * X + R[4] * Y + R[5] * Z) + t[1], cz3 = (R[6] * X + R[7] * Y + R[8] * Z) + t[2];
    const float xc = (float)cx3, yc = (float)cy3;
    const float invzc = (float)(1.0 / cz3);
    u = in->K4[0] * xc * invzc + in->K4[2];
    v = in->K4[1] * yc * invzc + in->K4[3];
    ok = !(u < in->bounds[0] || u > in->bounds[1]) && !(v < in->bounds[2] || v > in->bounds[3]);
    // Ow = -Rcw^T tcw (:1280), dist3D = |x3Dw - Ow| narrowed to float (:1309-1310)
    const double Ox = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), Oy = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]), Oz = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
    const double Px = X - Ox, Py = Y - Oy, Pz = Z - Oz;
    const float dist = (float)sqrt(Px * Px + Py * Py + Pz * Pz);
    const float maxD = 1.2f * maxd[g], minD = 0.8f * mind[g];
    if (dist < minD || dist > maxD) ok = false;
    const float ratio = maxd[g] / dist;                          // MapPoint::PredictScale (src/MapPoint.cc:406-420)
    lvl = (int)ceilf(logf(ratio) / in->log_scale);
    if (!(lvl >= 0)) lvl = 0; else if (lvl >= in->nlevels) lvl = in->nlevels - 1;
    r = th * in->scale[lvl];
  }
  q_uv[2 * (size_t)g] = u; q_uv[2 * (size_t)g + 1] = v; q_r[g] = ok ? r : 0.f; q_lo[g] = lvl - 1; q_hi[g] = lvl + 1; q_valid[g] = ok ? 1 : 0;
}

// one workgroup per candidate: PoseOptimization's rows of the pending solve - the slots that hold a point, in feature order
// (src/CeresOptimizer.cc:305-328) - behind the rows of the candidates before it
__global__ __launch_bounds__(1024) void k_rr_gather(const RrIn* __restrict__ in, const RrCand* __restrict__ cand, const RrState* __restrict__ state,
                                                    const int32_t* __restrict__ slots, const double* __restrict__ Xw, const float* __restrict__ kps4,
                                                    double* __restrict__ obs_Xw, double* __restrict__ obs_uv, float* __restrict__ obs_w, int32_t* __restrict__ obs_off) {
  __shared__ int s_w[16];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int n_kp = in->n_kp, icap = in->icap;
  int base = 0;
  for (int j = 0; j < c; j++) base += max(state[j].live, 0);
  const int mine = max(state[c].live, 0);
  if (tid == 0) { obs_off[c] = base; if (c == in->n_cand - 1) obs_off[c + 1] = base + mine; }
  const int32_t* S = slots + (size_t)c * icap;
  const int koff = cand[c].off;
  constexpr int FPT = TRK_MAXKP / 1024;
  int sl[FPT], cnt = 0;
#pragma unroll
  for (int k = 0; k < FPT; k++) { const int f = FPT * tid + k; sl[k] = (mine > 0 && f < n_kp) ? S[f] : -1; cnt += sl[k] >= 0 ? 1 : 0; }
  int pos = base + rr_scan1024(cnt, s_w) - cnt;
#pragma unroll
  for (int k = 0; k < FPT; k++) {
    if (sl[k] < 0) continue;
    const int f = FPT * tid + k;
    const double* X = Xw + 3 * (size_t)(koff + sl[k]);
    const float4 kp = ((const float4*)kps4)[f];
    obs_Xw[3 * (size_t)pos] = X[0]; obs_Xw[3 * (size_t)pos + 1] = X[1]; obs_Xw[3 * (size_t)pos + 2] = X[2];
    obs_uv[2 * (size_t)pos] = (double)kp.x; obs_uv[2 * (size_t)pos + 1] = (double)kp.y;
    obs_w[pos] = in->inv_sigma2[min(max((int)kp.z, 0), 15)];
    pos++;
  }
}

// one workgroup per candidate: what lies between two solves.  STEP 0: the slots as the caller gave them.  STEP 1 .. 3: the flags of
// solve STEP - 1, its gates, the search behind it (1: wide, 2: narrow) and the row count of the next solve.
template <int STEP>
__global__ __launch_bounds__(1024) void k_rr_step(const RrIn* __restrict__ in, const RrCand* __restrict__ cand, RrState* __restrict__ state, double* __restrict__ poses,
                                                  const int32_t* __restrict__ slot_in, int32_t* __restrict__ slots, uint8_t* __restrict__ outl,
                                                  const int32_t* __restrict__ rep, const float* __restrict__ q_angle, const float* __restrict__ kps4,
                                                  const int32_t* __restrict__ obs_off, const uint8_t* __restrict__ row_outl, const int32_t* __restrict__ n_inl,
                                                  const uint8_t* __restrict__ q_valid, const uint32_t* __restrict__ acc, const int32_t* __restrict__ acc_n,
                                                  const uint32_t* __restrict__ off, const uint32_t* __restrict__ off_total_p, const uint2* __restrict__ pairs,
                                                  const uint32_t cand_cap, const int orb_dist) {
  __shared__ int s_S[TRK_MAXKP];                                // map_points_[f] as a keyframe feature, -1 empty
  __shared__ int s_minu[TRK_MAXKP];                             // smallest unsettled point that lists the feature (this round)
  __shared__ unsigned char s_found[TRK_MAXKP];                  // sAlreadyFound, by the first feature that holds the point (rep)
  __shared__ unsigned char s_new[TRK_MAXKP];                    // 1 + rotation bin of the assignment THIS pass made to the feature, 0 none
  __shared__ unsigned short s_wl[2][TRK_MAXKP];                 // work lists of the unsettled points
  __shared__ int s_hist[TRK_HISTO], s_keep[TRK_HISTO], s_n[2], s_cnt[2], s_w[16];
  const int c = blockIdx.x, tid = threadIdx.x;
  const RrCand C = cand[c];
  const int n_kp = in->n_kp, icap = in->icap, nq = C.n, check_ori = in->check_ori;
  int32_t* S_g = slots + (size_t)c * icap;
  uint8_t* outl_g = outl + (size_t)c * icap;
  constexpr int FPT = TRK_MAXKP / 1024;
  RrState st = state[c];

  if (STEP == 0) {
    for (int f = tid; f < n_kp; f += 1024) { S_g[f] = C.has_pose ? slot_in[(size_t)c * n_kp + f] : -1; outl_g[f] = 0; }
    int cnt = 0;
    if (C.has_pose) for (int f = tid; f < n_kp; f += 1024) cnt += slot_in[(size_t)c * n_kp + f] >= 0 ? 1 : 0;
    const int total = rr_scan1024(cnt, s_w);                   // (inclusive: thread 1023 holds the workgroup's total)
    if (tid == 1023) {
      st.stage = C.has_pose ? RR_RUNNING : ORBT_RR_NO_POSE; st.matched = 0; st.narrow_passes = 0; st.live = C.has_pose ? total : -1;
      for (int k = 0; k < 3; k++) { st.n_good[k] = -1; st.n_corr[k] = -1; }
      st.n_add[0] = -1; st.n_add[1] = -1;
      if (C.has_pose) st.n_corr[0] = total;
      state[c] = st;
    }
    return;
  }
  if (st.stage != RR_RUNNING) return;                           // out or matched: its slots and flags stay as they are
  const uint32_t off_total = (STEP == 1 || STEP == 2) ? *off_total_p : 0u;
  const bool overflow = off_total > cand_cap;                   // (the host runs the call again with larger lists: what follows is discarded)

  // ---- the solve that just ran: is_outliers_ of its rows (false for all of them below 3 correspondences), nGood
  const int n_corr = st.live, nGood = rr_ngood(n_corr, n_inl[c]);
  {
    int sl[FPT], cnt = 0;
#pragma unroll
    for (int k = 0; k < FPT; k++) { const int f = FPT * tid + k; sl[k] = f < n_kp ? S_g[f] : -1; s_S[f] = sl[k]; cnt += sl[k] >= 0 ? 1 : 0; }
    int pos = obs_off[c] + rr_scan1024(cnt, s_w) - cnt;
#pragma unroll
    for (int k = 0; k < FPT; k++) {
      if (sl[k] < 0) continue;
      const int f = FPT * tid + k;
      const uint8_t o = n_corr < 3 ? (uint8_t)0 : row_outl[pos];
      outl_g[f] = o;
      // outlier slots are cleared behind the first (:1078-1080) and the third solve (:1110-1114), not behind the second
      if (o && ((STEP == 1 && nGood >= 10) || STEP == 3)) { s_S[f] = -1; S_g[f] = -1; }
      pos++;
    }
  }
  __syncthreads();
  st.n_good[STEP > 0 ? STEP - 1 : 0] = nGood;
  st.live = -1;
  int stage = RR_RUNNING;
  if (STEP == 1) { if (n_corr < 3) stage = ORBT_RR_NO_POSE; else if (nGood < 10) stage = ORBT_RR_FEW_INLIERS; else if (nGood >= 50) stage = ORBT_RR_MATCH_FIRST; }
  if (STEP == 2) { if (nGood >= 50) stage = ORBT_RR_MATCH_SECOND; else if (!(nGood > 30)) stage = ORBT_RR_FAIL_SECOND; }
  if (STEP == 3) stage = nGood >= 50 ? ORBT_RR_MATCH_THIRD : ORBT_RR_FAIL_THIRD;
  if (stage != RR_RUNNING) {
    if (tid == 0) { st.stage = stage; st.matched = nGood >= 50 ? 1 : 0; state[c] = st; }
    return;
  }

  // ---- the search: ONE pass of src/ORBmatcher.cc:1289-1381 over the points that are not in s_found; returns the assignments made
  // before the rotation check in s_cnt[0] and the ones it removed in s_cnt[1]
  const int koff = C.off;
  auto for_each = [&](int q, auto&& f) {                         // the acceptable candidates of point q in window order
    const int g = koff + q, na = acc_n[g];
    if (na <= TRK_LMAX) { for (int e = 0; e < na; e++) { const uint32_t v = acc[(size_t)g * TRK_LMAX + e]; f((int)(v & 0xFFFFu), (int)(v >> 16)); } }
    else { for (uint32_t e = off[2 * g]; e < off[2 * g + 1] && e < cand_cap; e++) { const uint2 pr = pairs[e]; if ((int)pr.y <= orb_dist) f((int)pr.x, (int)pr.y); } }
  };
  auto run_pass = [&]() {
    for (int t = tid; t < TRK_MAXKP; t += 1024) s_new[t] = 0;
    if (tid < TRK_HISTO) s_hist[tid] = 0;
    if (tid == 0) { s_n[0] = 0; s_n[1] = 0; s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    for (int q0 = 0; q0 < nq; q0 += 1024) {
      const int q = q0 + tid;
      bool act = false;
      if (q < nq && !overflow) { const int r = rep[koff + q]; act = r >= 0 && q_valid[koff + q] != 0 && !s_found[r] && acc_n[koff + q] > 0; }
      const unsigned long long m = __ballot(act);
      int base = 0;
      if ((tid & 63) == 0 && m) base = atomicAdd(&s_n[0], __popcll(m));
      base = __shfl(base, 0);
      if (act) s_wl[0][base + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = (unsigned short)q;
    }
    __syncthreads();
    int cur = 0;
    while (true) {
      const int nw = s_n[cur];
      if (nw == 0) break;
      for (int t = tid; t < TRK_MAXKP; t += 1024) s_minu[t] = INT_MAX;
      __syncthreads();
      if (tid == 0) s_n[cur ^ 1] = 0;
      for (int i = tid; i < nw; i += 1024) { const int q = s_wl[cur][i]; for_each(q, [&](int t, int) { atomicMin(&s_minu[t], q); }); }
      __syncthreads();
      for (int i0 = 0; i0 < nw; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false; int q = 0;
        if (i < nw) {
          q = s_wl[cur][i];
          bool first = true;
          for_each(q, [&](int t, int) { first = first && s_minu[t] == q; });
          if (!first) keep = true;
          else {
            int best = 256, bi = -1;
            for_each(q, [&](int t, int d) { if (s_S[t] < 0 && d < best) { best = d; bi = t; } });      // (:1336: a feature that holds a point is skipped; first minimum)
            if (bi >= 0 && best <= orb_dist) {
              s_S[bi] = q;
              int b = 0;
              if (check_ori) {
                float rot = q_angle[koff + q] - kps4[4 * bi + 3];
                if (rot < 0.0) rot += 360.0f;
                b = (int)roundf(rot * (1.0f / TRK_HISTO));
                if (b == TRK_HISTO) b = 0;
                b = min(max(b, 0), TRK_HISTO - 1);
                atomicAdd(&s_hist[b], 1);
              }
              s_new[bi] = (unsigned char)(1 + b);
              atomicAdd(&s_cnt[0], 1);
            }
          }
        }
        const unsigned long long m = __ballot(keep);
        int base = 0;
        if ((tid & 63) == 0 && m) base = atomicAdd(&s_n[cur ^ 1], __popcll(m));
        base = __shfl(base, 0);
        if (keep) s_wl[cur ^ 1][base + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = (unsigned short)q;
      }
      __syncthreads();
      cur ^= 1;
    }
    if (check_ori) {                                             // (uniform: every thread left the loop on the same s_n)
      if (tid == 0) {
        int top[3] = {-1, -1, -1}, pop[3] = {0, 0, 0};
        for (int b = 0; b < TRK_HISTO; b++) {                    // strict '>': the earlier bin wins ties (ComputeThreeMaxima :1386-1418)
          int r = 3;
          while (r > 0 && s_hist[b] > pop[r - 1]) r--;
          if (r == 3) continue;
          for (int m = 2; m > r; m--) { top[m] = top[m - 1]; pop[m] = pop[m - 1]; }
          top[r] = b; pop[r] = s_hist[b];
        }
        if ((float)pop[1] < 0.1f * (float)pop[0]) { top[1] = -1; top[2] = -1; }
        else if ((float)pop[2] < 0.1f * (float)pop[0]) { top[2] = -1; }
        for (int b = 0; b < TRK_HISTO; b++) s_keep[b] = (b == top[0] || b == top[1] || b == top[2]) ? 1 : 0;
      }
      __syncthreads();
      for (int t = tid; t < TRK_MAXKP; t += 1024) {
        const int b = s_new[t];
        if (b && !s_keep[b - 1]) { s_S[t] = -1; atomicAdd(&s_cnt[1], 1); }      // (:1373-1379: a removed match leaves its slot empty)
      }
    }
    __syncthreads();
  };

  int nadd = 0;
  if (STEP == 1) {
    // `found` is the PnP inlier set (:1062-1069): the slots the caller gave, whatever was cleared since
    for (int t = tid; t < TRK_MAXKP; t += 1024) s_found[t] = 0;
    __syncthreads();
    for (int f = tid; f < n_kp; f += 1024) { const int k = slot_in[(size_t)c * n_kp + f]; if (k >= 0) s_found[rep[koff + k]] = 1; }
    __syncthreads();
    run_pass();
    nadd = s_cnt[0] - s_cnt[1];
    st.n_add[0] = nadd;
  }
  if (STEP == 2) {
    for (int t = tid; t < TRK_MAXKP; t += 1024) s_found[t] = 0;
    __syncthreads();
    int passes = 0;
    if (in->narrow_in_loop) {
      for (int ip = 0; ip < n_kp; ip++) {
        if (tid == 0 && s_S[ip] >= 0) s_found[rep[koff + s_S[ip]]] = 1;
        __syncthreads();
        run_pass();
        passes++;
        const int raw = s_cnt[0], net = s_cnt[0] - s_cnt[1];
        __syncthreads();                                         // (run_pass resets the counters)
        if (raw == 0) { nadd = 0; break; }                       // every later pass is empty: the last one returns 0
        nadd = net;                                              // (counts iff this was pass N_ - 1)
      }
    } else {
      for (int f = tid; f < n_kp; f += 1024) if (s_S[f] >= 0) s_found[rep[koff + s_S[f]]] = 1;
      __syncthreads();
      run_pass();
      passes = 1;
      nadd = s_cnt[0] - s_cnt[1];
    }
    st.n_add[1] = nadd; st.narrow_passes = passes;
  }
  // ---- the gate behind the search (:1089, :1107), the slots back to memory, the next solve's row count
  const bool go = nadd + nGood >= 50;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < FPT; k++) { const int f = FPT * tid + k; if (f < n_kp) { S_g[f] = s_S[f]; cnt += s_S[f] >= 0 ? 1 : 0; } }
  const int total = rr_scan1024(cnt, s_w);
  if (tid == 1023) {
    if (go) {
      st.live = total; st.n_corr[STEP] = total;
      // the next PoseOptimization starts from Eigen::Quaterniond(Tcw_'s rotation) (src/CeresOptimizer.cc:286-291), and Tcw_ is the matrix of
      // the NORMALISED quaternion the solve before left (:336-340): Matrix_7_1_ToMatrix4d, then Matrix4dToMatrix_7_1
      double R[9], t[3], q[4];
      rr_pose_to_Rt(poses + 7 * c, R, t);
      const double m[3][3] = {{R[0], R[1], R[2]}, {R[3], R[4], R[5]}, {R[6], R[7], R[8]}};
      rot_to_quat(m, q);
      for (int k = 0; k < 4; k++) poses[7 * c + 3 + k] = q[k];
    }
    else st.stage = STEP == 1 ? ORBT_RR_FAIL_WIDE : ORBT_RR_FAIL_NARROW;
    state[c] = st;
  }
}

}  // namespace orbhip

extern "C" int orbt_relocalization_refine(orbx_ctx* ctx, const float* K4, const float* bounds, float log_scale_factor, const orbt_reloc_refine_candidate* cand,
                                          int n_cand, int n_kp, int check_ori, int narrow_in_loop, orbt_reloc_refine_result* res, int32_t* slot_kf_out,
                                          uint8_t* outlier_out, int32_t* first_match) {
  static const char* const entry = "orbt_relocalization_refine";
  CallClock call_clock;
  ORBHIP_REQUIRE(ctx && K4 && bounds && first_match && n_cand >= 0 && n_kp >= 0 && (n_cand == 0 || (cand && res)), ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(n_cand == 0 || n_kp == 0 || (slot_kf_out && outlier_out), ORBHIP_EINVAL, "NULL output");
  ORBHIP_REQUIRE(std::isfinite(log_scale_factor) && log_scale_factor > 0.f, ORBHIP_EINVAL, "bad log_scale_factor");
  ORBHIP_REQUIRE(n_cand <= ORBT_RR_MAX_CANDIDATES, ORBHIP_ECAP, "more than 64 candidates per call");
  ORBHIP_REQUIRE(n_kp <= TRK_MAXKP, ORBHIP_ECAP, "more than 4096 features per frame");
  *first_match = -1;
  if (n_cand == 0) return 0;
  // the keyframe sides, concatenated; rep[i] = the first feature of the candidate that holds the same point (the set's element)
  std::vector<RrCand> h_cand((size_t)n_cand);
  int ntot = 0, max_n = 1;
  for (int c = 0; c < n_cand; c++) {
    const orbt_reloc_refine_candidate& q = cand[c];
    ORBHIP_REQUIRE(q.n >= 0 && (q.n == 0 || (q.pt && q.Xw && q.desc && q.min_dist && q.max_dist && q.angle)), ORBHIP_EINVAL, "NULL candidate argument");
    ORBHIP_REQUIRE(q.n <= TRK_MAXKP, ORBHIP_ECAP, "more than 4096 features per keyframe");
    ORBHIP_REQUIRE(!q.Tcw || n_kp == 0 || q.slot_kf, ORBHIP_EINVAL, "NULL slot_kf of a candidate with a pose");
    RrCand& H = h_cand[c]; std::memset(&H, 0, sizeof(H));
    H.off = ntot; H.n = q.n; H.has_pose = q.Tcw ? 1 : 0;
    ntot += q.n; max_n = std::max(max_n, q.n);
  }
  std::vector<int32_t> h_rep((size_t)std::max(ntot, 1)), h_slot((size_t)n_cand * std::max(n_kp, 1), -1);
  {
    std::vector<std::pair<int32_t, int32_t>> ids;
    for (int c = 0; c < n_cand; c++) {
      const orbt_reloc_refine_candidate& q = cand[c];
      int32_t* rep = h_rep.data() + h_cand[c].off;
      ids.clear();
      for (int i = 0; i < q.n; i++) {
        if (q.pt[i] < -1) ORBHIP_ARG(arg_fail(entry, "candidates[%d].pt[%d] = %d is below -1", c, i, q.pt[i]));
        rep[i] = -1;
        if (q.pt[i] >= 0) ids.push_back({q.pt[i], i});
      }
      std::sort(ids.begin(), ids.end());
      for (size_t k = 0; k < ids.size(); k++) rep[ids[k].second] = (k > 0 && ids[k - 1].first == ids[k].first) ? rep[ids[k - 1].second] : ids[k].second;
      if (!q.Tcw) continue;
      char name[48]; std::snprintf(name, sizeof(name), "candidates[%d].slot_kf", c);
      ORBHIP_ARG(check_index(entry, name, q.slot_kf, n_kp, q.n, true));
      for (int f = 0; f < n_kp; f++)
        if (q.slot_kf[f] >= 0 && q.pt[q.slot_kf[f]] < 0) ORBHIP_ARG(arg_fail(entry, "%s[%d] = %d names a feature without a map point", name, f, q.slot_kf[f]));
      std::memcpy(h_slot.data() + (size_t)c * n_kp, q.slot_kf, 4 * (size_t)n_kp);
      for (int k = 0; k < 12; k++) ORBHIP_REQUIRE(std::isfinite(q.Tcw[k]), ORBHIP_EINVAL, "non-finite candidate pose");
    }
  }
  const TrkFrame& TF = g_trk_frame;
  ThreadWs& W = thread_ws();
  static thread_local uint32_t cand_hw = 0;                     // high-water mark of the candidate lists (both searches)
  int nlevels = 0, rc = 0;
  RrIn I; std::memset(&I, 0, sizeof(I));
  for (int k = 0; k < 4; k++) { I.K4[k] = K4[k]; I.bounds[k] = bounds[k]; }
  I.log_scale = log_scale_factor; I.check_ori = check_ori ? 1 : 0; I.narrow_in_loop = narrow_in_loop ? 1 : 0; I.n_cand = n_cand; I.n_kp = n_kp; I.ntot = ntot;
  std::vector<double> h_K4d((size_t)4 * n_cand);
  for (int c = 0; c < n_cand; c++) for (int k = 0; k < 4; k++) h_K4d[4 * (size_t)c + k] = (double)K4[k];
  for (int attempt = 0; attempt < 2; attempt++) {
    if ((rc = W.begin())) return rc;
    if ((rc = trk_dims(ctx, -1, nullptr, &nlevels)) || (rc = trk_require_resident(TF, W.device, ctx, nlevels, -1))) return rc;
    ORBHIP_REQUIRE(n_kp == TF.n_kp, ORBHIP_EINVAL, "n_kp differs from the resident frame's keypoint count");
    if ((rc = orbx_get_tables(ctx, I.scale, nullptr, nullptr, I.inv_sigma2, nullptr))) return rc;
    const int icap = std::max(TF.icap, 1);
    I.nlevels = nlevels; I.icap = icap;
    for (int c = 0; c < n_cand; c++) if (cand[c].Tcw && (rc = trk_pose7(cand[c].Tcw, h_cand[c].pose7))) return rc;
    ThreadWs::Pack in;
    const int pI = in.add(&I, sizeof(I)), pC = in.add(h_cand.data(), sizeof(RrCand) * (size_t)n_cand), pK = in.add(h_K4d.data(), 32 * (size_t)n_cand),
              pS = in.add(h_slot.data(), 4 * h_slot.size()), pR = in.add(h_rep.data(), 4 * h_rep.size());
    // (the per-feature arrays: one piece per array, the candidates' rows behind each other)
    std::vector<uint8_t> stage_buf;
    const size_t n1 = (size_t)std::max(ntot, 1);
    stage_buf.resize(n1 * (24 + 32 + 4 + 4 + 4));
    double* hX = (double*)stage_buf.data(); uint8_t* hD = (uint8_t*)(hX + 3 * n1);
    float* hMi = (float*)(hD + 32 * n1); float* hMa = hMi + n1; float* hA = hMa + n1;
    for (int c = 0; c < n_cand; c++) {
      const orbt_reloc_refine_candidate& q = cand[c]; const size_t o = (size_t)h_cand[c].off, n = (size_t)q.n;
      if (!n) continue;
      std::memcpy(hX + 3 * o, q.Xw, 24 * n); std::memcpy(hD + 32 * o, q.desc, 32 * n);
      std::memcpy(hMi + o, q.min_dist, 4 * n); std::memcpy(hMa + o, q.max_dist, 4 * n); std::memcpy(hA + o, q.angle, 4 * n);
    }
    const int pX = in.add(hX, 24 * n1), pD = in.add(hD, 32 * n1), pMi = in.add(hMi, 4 * n1), pMa = in.add(hMa, 4 * n1), pA = in.add(hA, 4 * n1);
    if ((rc = W.commit(in))) return rc;
    // ONE download block: [state | poses | totals of the two window searches | slots | flags]
    Carve C;
    const size_t oState = C.take(sizeof(RrState) * (size_t)n_cand), oPose = C.take(56 * (size_t)n_cand), oTot = C.take(8),
                 oSlot = C.take(4 * (size_t)icap * n_cand), oOutl = C.take((size_t)icap * n_cand);
    uint8_t* dblk = W.d<uint8_t>(C.total, &rc);
    TrkWindows Q;
    Q.alloc(W, ntot, RR_PAIRS_PER_QUERY, cand_hw, &rc);
    const size_t rows = (size_t)icap * n_cand;
    double* oX = W.d<double>(3 * rows, &rc); double* ouv = W.d<double>(2 * rows, &rc); float* ow = W.d<float>(rows, &rc);
    int32_t* ooff = W.d<int32_t>((size_t)n_cand + 1, &rc); uint8_t* row_outl = W.d<uint8_t>(rows, &rc); int32_t* d_ninl = W.d<int32_t>((size_t)n_cand, &rc);
    if (rc) return rc;
    const RrIn* dI = in.dev<RrIn>(pI); const RrCand* dC = in.dev<RrCand>(pC);
    RrState* dS = (RrState*)(dblk + oState); double* d_pose = (double*)(dblk + oPose); uint32_t* d_tot = (uint32_t*)(dblk + oTot);
    int32_t* d_slot = (int32_t*)(dblk + oSlot); uint8_t* d_outl = dblk + oOutl;
    const int32_t* d_rep = in.dev<int32_t>(pR); const double* dX = in.dev<double>(pX);
    const float* kps4 = TF.kps4.as<float>();
    // the poses the solves work on: [t, q] of the PnP poses (a candidate without one: identity, never read)
    {
      std::vector<double> hp((size_t)7 * n_cand, 0.0);
      for (int c = 0; c < n_cand; c++) { if (cand[c].Tcw) std::memcpy(&hp[7 * (size_t)c], h_cand[c].pose7, 56); else hp[7 * (size_t)c + 6] = 1.0; }
      double* up = W.up<double>(hp.data(), hp.size(), &rc);
      if (rc) return rc;
      ORBHIP_CHECK_HIP(hipMemcpyAsync(d_pose, up, 56 * (size_t)n_cand, hipMemcpyDeviceToDevice, W.s));
    }
    ORBHIP_CHECK_HIP(hipMemsetAsync(d_tot, 0, 8, W.s));
    auto solve = [&]() -> int {
      hipLaunchKernelGGL(k_rr_gather, dim3(n_cand), dim3(1024), 0, W.s, dI, dC, (const RrState*)dS, (const int32_t*)d_slot, dX, kps4, oX, ouv, ow, ooff);
      ORBHIP_CHECK_HIP(hipGetLastError());
      return ba_pose_optimization_batch_device(in.dev<double>(pK), d_pose, oX, ouv, ow, ooff, n_cand, row_outl, d_ninl, nullptr, (void*)W.s);
    };
    auto search = [&](int which, float th, int dmax) {
      hipLaunchKernelGGL(k_rr_project, dim3((max_n + 255) / 256, n_cand), dim3(256), 0, W.s, dI, dC, (const RrState*)dS, (const int32_t*)d_ninl, (const double*)d_pose, d_rep,
                         dX, in.dev<float>(pMi), in.dev<float>(pMa), which, th, Q.quv, Q.qr, Q.qlo, Q.qhi, Q.qv, Q.total);
      Q.launch(W.s, TF, in.dev<uint8_t>(pD), dmax);
    };
#define RR_STEP(N, DMAX)                                                                                                                                  \
  hipLaunchKernelGGL(k_rr_step<N>, dim3(n_cand), dim3(1024), 0, W.s, dI, dC, dS, d_pose, in.dev<int32_t>(pS), d_slot, d_outl, d_rep, in.dev<float>(pA), kps4,     \
                     (const int32_t*)ooff, (const uint8_t*)row_outl, (const int32_t*)d_ninl, (const uint8_t*)Q.qv, (const uint32_t*)Q.acc,                \
                     (const int32_t*)Q.accn, (const uint32_t*)Q.off, (const uint32_t*)Q.total, (const uint2*)Q.pairs, Q.cand_cap, DMAX)
    RR_STEP(0, 0);
    if ((rc = solve())) return rc;
    search(0, 10.0f, 100);
    RR_STEP(1, 100);
    ORBHIP_CHECK_HIP(hipMemcpyAsync(d_tot, Q.total, 4, hipMemcpyDeviceToDevice, W.s));
    if ((rc = solve())) return rc;
    search(1, 3.0f, 64);
    RR_STEP(2, 64);
    ORBHIP_CHECK_HIP(hipMemcpyAsync(d_tot + 1, Q.total, 4, hipMemcpyDeviceToDevice, W.s));
    if ((rc = solve())) return rc;
    RR_STEP(3, 0);
#undef RR_STEP
    ORBHIP_CHECK_HIP(hipGetLastError());
    const uint8_t* hb = W.down(dblk, C.total, &rc);
    if (rc || (rc = W.sync())) return rc;
    const uint32_t* tot = (const uint32_t*)(hb + oTot);
    if (Q.regrown(std::max(tot[0], tot[1]), cand_hw)) continue;
    const RrState* hs = (const RrState*)(hb + oState);
    for (int c = 0; c < n_cand; c++) {
      orbt_reloc_refine_result& r = res[c];
      r.stage = hs[c].stage; r.matched = hs[c].matched; r.narrow_passes = hs[c].narrow_passes; r.reserved = 0;
      for (int k = 0; k < 3; k++) { r.n_good[k] = hs[c].n_good[k]; r.n_correspondences[k] = hs[c].n_corr[k]; }
      r.n_additional[0] = hs[c].n_add[0]; r.n_additional[1] = hs[c].n_add[1];
      std::memcpy(r.pose7, hb + oPose + 56 * (size_t)c, 56);
      if (n_kp) {
        std::memcpy(slot_kf_out + (size_t)c * n_kp, hb + oSlot + 4 * (size_t)c * icap, 4 * (size_t)n_kp);
        std::memcpy(outlier_out + (size_t)c * n_kp, hb + oOutl + (size_t)c * icap, (size_t)n_kp);
      }
      if (r.matched && *first_match < 0) *first_match = c;
    }
    return 0;
  }
  return TrkWindows::no_fit();
}
