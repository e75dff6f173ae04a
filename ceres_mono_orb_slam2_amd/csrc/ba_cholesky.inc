// dense blocked Cholesky of the reduced camera system - part of the translation unit ba_solver.hip (textually included there; not compiled on its own).
// k_chol_la / k_chol_wg / k_chol_persist / k_chol_persist_blk, the 32x32 diagonal factor, forward / backward substitution.

// ---- dense blocked Cholesky (lower, in place), NB = 32 ---------------------------------------------------
#ifndef NB
#define NB 32
#endif
#if defined(ORBHIP_CHOL_PROF) && !defined(ORBHIP_TEST_HOOKS)
#define ORBHIP_TEST_HOOKS                /* the profiling build carries the test hooks too (tools/factor_ab.py) */
#endif
// Phase timing of the factorisation step kernels (tools/chol_phase_prof.py builds a scratch library with -DORBHIP_CHOL_PROF):
// wave 0 of workgroup 0 of problem 0 stamps s_memrealtime (100 MHz) at the phase boundaries; sums per step index.
#if defined(ORBHIP_SCHUR_PROF) && !defined(ORBHIP_CHOL_PROF)
__device__ unsigned long long g_p2_prof[8][128];
__device__ unsigned long long g_chol_prof[128][10];
#endif
#ifdef ORBHIP_CHOL_PROF
__device__ unsigned long long g_p2_prof[8][128];       // k_chol_persist_2l timeline (absolute s_memrealtime): see tools/chol_p2_timeline.py
#define P2_MARK(row, idx) do { if ((threadIdx.x & 63) == 0) atomicMax(&g_p2_prof[row][(idx) & 127], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } while (0)
__device__ unsigned long long g_chol_prof[128][10];
#define CHOL_STAMP(i) do { if (prof_on) { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); \
                              if (threadIdx.x == 0) g_chol_prof[prof_step][i] += t_ - prof_t; prof_t = t_; } } while (0)
#define CHOL_PROF_BEGIN(step) const bool prof_on = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64; const int prof_step = (step) & 127; \
                              unsigned long long prof_t = __builtin_amdgcn_s_memrealtime(); if (prof_on && threadIdx.x == 0) g_chol_prof[prof_step][9] += 1
#else
#define CHOL_STAMP(i) do { } while (0)
#define CHOL_PROF_BEGIN(step) do { } while (0)
#define P2_MARK(row, idx) do { } while (0)
#endif
// panel: every workgroup factors and inverts the 32x32 diagonal block redundantly in ONE wave
// (diag_factor_invert_wave below), workgroup 0 stores L11^-1; then every wave
// forms 16 rows of L21 = A21 * L11^-T on the FP64 matrix cores (2 column tiles x 8 k-steps of
// v_mfma_f64_16x16x4_f64).  Rows run to npad INCLUSIVE: row npad is the augmented rhs row.
typedef double double4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double bcast_lane(double v, int lane) {      // lane is a compile-time constant after unrolling
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, lane); hi = __builtin_amdgcn_readlane(hi, lane);
  return __hiloint2double(hi, lo);
}
// ---- 32x32 diagonal block: inverse of its Cholesky factor, by 1, 2 or 4 cooperating waves (round 6) ------------------------------
// What the chain needs from a diagonal block D is X = L^-1 (D = L L^T); L itself is never read.  Measured on gfx950
// (tools/ubench/f64_latency.hip, profiles/r06_f64_latency.txt): a lone wave issues ONE instruction per ~4.5 cycles whatever it is,
// a DEPENDENT v_fma_f64 costs no more than that, v_rcp_f64 / v_rsq_f64 ~20 cycles, a v_readlane round trip ~12, an LDS write ->
// broadcast read 106; v_mfma_f64_16x16x4 takes 65 cycles for 2048 flops and v_mfma_f64_4x4x4_4b 16.5 for 512 - the matrix cores'
// FP64 rate EQUALS the VALU's (64 lanes x 2 flops per 4.5 cycles), so they cannot shorten a 32 x 32 factor; its wall is the number
// of instructions one wave has to issue.  Rounds 2 - 5 factored with ~2100 instructions on one wave (4.56 us).  This form:
//   * square-root-free elimination: D = L~ diag(d) L~^T.  Lane r (< 32) of a wave keeps entries of row r, lane 32 + c' the same
//     entries of column c' of the identity (forward substitution with the unit factor L~ is the same instruction stream).  Column j
//     needs ONE uniform number, w_j = 1 / d_j: multiplier m = a(., j) w_j, then a(., k) -= m a(k, j) for k > j.  The column entries
//     a(k, j) are final BEFORE w_j is known (nothing scales them), so their trip through LDS (the broadcast operand of the update)
//     is off the critical path;
//   * the pivot recurrence is  d_(j+1) = sb - sa^2 w_j  with sa = a(j+1, j), sb = a(j+1, j+1) (both updated through column j-1 and
//     both in lane j+1's own registers), w_j = r0 (1 + u), r0 = v_rcp_f64(d_j) (2^-24), e = 1 - d_j r0, u = e + e^2 (one cubic step:
//     2^-72).  Written as q = sa^2 r0, p = sb - q, d_(j+1) = p - q u it is: readlane, rcp, e, u, fma - ~46 cycles per column, ten
//     instructions; no square root, no Newton iteration, no per-column scaling on it;
//   * at the end X(rr, c') = z(rr, c') / sqrt(d_rr): one vector rsqrt (cubic step) over the pivots, which lane rr kept;
//   * NW waves split the ENTRY COLUMNS (wave q owns columns [32 q / NW, 32 (q + 1) / NW) of every row): the owner of column j
//     publishes the lanes' multipliers (s_M) next to the column entries (s_C) and raises a counter in LDS; a wave first applies the
//     columns before its own block as they appear, then runs the chain over its block and hands it to the next wave.  Every entry
//     receives the same fmas in the same order and every pivot the same formula whatever NW is: the 1-, 2- and 4-wave forms give the
//     same bits (tests/test_gpu_diag_factor.py compares them on every class of block), so the kernels pick NW by the waves they have idle.
// A non-positive / non-finite pivot is reported (the block's inverse is then garbage; the caller discards the step).
// Measured on gfx950 against correctly rounded values (tests/test_gpu_diag_factor.py, 1 034 731 doubles over [2^-1021, 2^1021], every
// power of two and its neighbours): w of piv_recip IS the correctly rounded reciprocal on all of them (0 ulp), rsqrt_cubic is within 1 ulp
// (off by one on 13.8 %), both exact on powers of two; X against an mp reference: at most 2.04 x LAPACK's residual and 1.56 x its
// forward error per class of block (Wishart, condition 1e2 .. 1e13, graded, Jacobi-scaled, padded), asserted <= 4 x.
#define CHOL_SB() __builtin_amdgcn_sched_barrier(0)
#define CHOL_PIN(x) asm volatile("" : "+v"(x))
__device__ __forceinline__ void piv_recip(const double d, double& r0, double& u, double& w) {
  r0 = __builtin_amdgcn_rcp(d);
  const double e = fma(-d, r0, 1.0);
  u = fma(e, e, e);
  w = fma(r0, u, r0);
}
__device__ __forceinline__ double rsqrt_cubic(const double d) {      // 1 / sqrt(d): v_rsq_f64 (2^-23) and one cubic step
  const double y0 = __builtin_amdgcn_rsq(d);
  const double t = d * y0;
  const double e = fma(-t, y0, 1.0);
  const double p = fma(0.375, e, 0.5);
  const double ye = y0 * e;
  return fma(ye, p, y0);
}
typedef __attribute__((address_space(3))) int lds_int_t;
#if defined(ORBHIP_CHOL_PROF) || defined(BW_PROF)
__device__ unsigned long long g_df_stamp[4][4];
#endif
#ifdef ORBHIP_DF_STAMP                  // per wave: ticks (10 ns) from entry to [0] own block's start, [1] its end, [2] the function's end; [3] calls
#define DF_STAMP(i) do { if (lane0_) atomicAdd(&g_df_stamp[Q][i], (unsigned long long)__builtin_amdgcn_s_memrealtime() - t_in_); } while (0)
#else
#define DF_STAMP(i) do { } while (0)
#endif
template <int LANE>
__device__ __forceinline__ double writelane_f64(double v, const double s) {      // v with lane LANE replaced by the uniform s
  int lo = __double2loint(v), hi = __double2hiint(v);
  const int slo = __builtin_amdgcn_readfirstlane(__double2loint(s)), shi = __builtin_amdgcn_readfirstlane(__double2hiint(s));
  asm("v_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4" : "+v"(lo), "+v"(hi) : "s"(slo), "s"(shi), "n"(LANE));
  return __hiloint2double(hi, lo);
}
// LDS counter of published columns: plain LDS accesses, ordered by the LDS pipeline itself (a wave's DS instructions execute in
// issue order, so a reader that has SEEN the counter sees everything its writer stored before it) - no s_waitcnt on the writer's
// side.  The store is lane 0's alone, through the exec mask, without a branch; every lane of the wave is active at the call sites.
__device__ __forceinline__ void df_signal(int* s_col, const int v) {
  const unsigned addr = (unsigned)(unsigned long long)(lds_int_t*)s_col;
  asm volatile("s_mov_b64 exec, 1\n\tds_write_b32 %0, %1\n\ts_mov_b64 exec, -1" : : "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ int df_count(int* s_col) {
  const int v = __hip_atomic_load((lds_int_t*)s_col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
  return v;
}
// column c0 + JL of the owning wave's block (JL a template parameter: every register index, lane select and LDS offset is a literal).
// entering: (r0, u, w) belong to column j = c0 + JL, acc[JL] is final and sa2 its square, c1 = the column's entry a(j+1, j) (uniform, by
// v_readlane: column j's update of entry (j+1, j+1) makes the next sa - no time for LDS), cjc[] = its entries a(k, j) for the rows
// k >= j + 2 of the block (back from LDS, requested one body earlier).
// The statements are in ISSUE order (the inline asm of the signal and the fences pin the scheduler): the pivot recurrence first - t,
// readlane, rcp, e, u -, everything else in the shadows of its latencies.
template <int NW, int Q, int JL>
__device__ __forceinline__ void df_own_column(double (&acc)[NB / NW], double (&cjc)[NB / NW], double& r0, double& u, double& w, double& sa2, double& c1,
                                              double* s_C, double* s_M, double* s_R, int* s_col, const int col_base, const int lane) {
  constexpr int CB = NB / NW, c0 = CB * Q, j = c0 + JL;
  if constexpr (JL < CB) {
    CHOL_SB();                                                   // (a column's instructions stay together)
    if constexpr (JL + 1 < CB) {
      // the next pivot, from lane j+1's own entries: sa = acc[JL], sb = acc[JL + 1] (both updated through column j - 1)
      const double qv = sa2 * r0;
      const double pv = acc[JL + 1] - qv;
      const double t = fma(-qv, u, pv);
      const double d = bcast_lane(t, j + 1);                     // lane j + 1's t is the pivot
      const double m = acc[JL] * w;
      const double r0n = __builtin_amdgcn_rcp(d);
      if constexpr (NW > 1) s_M[j * 64 + lane] = m;
      acc[JL + 1] = fma(-m, c1, acc[JL + 1]);                    // column j + 1 is final: its entries go to LDS, the block's come back one body later
      s_C[(j + 1) * 64 + lane] = acc[JL + 1];
      sa2 = acc[JL + 1] * acc[JL + 1];
      double c1n = 0.0;
      if constexpr (JL + 2 < CB) { acc[JL + 2] = fma(-m, cjc[JL + 2], acc[JL + 2]); c1n = bcast_lane(acc[JL + 1], j + 2); }      // (entry j + 2: the sb after next - its operand had a column's time to come back from LDS)
      const double e = fma(-d, r0n, 1.0);
      if constexpr (NW > 1 && ((JL & 1) == 1)) df_signal(s_col, col_base + j + 1);      // (every other column: the consumers lag anyway; the block's last column signals below)
      const double un = fma(e, e, e);
      const double wn = fma(r0n, un, r0n);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      double cjn[CB];
#pragma unroll
      for (int kl = 0; kl < CB; kl++) cjn[kl] = 0.0;
      {
        constexpr int k0 = JL + 3;                               // first entry of column j + 1 the block needs from LDS
        constexpr int ke = k0 + (k0 & 1);
        if constexpr ((k0 & 1) != 0 && k0 < CB) cjn[k0] = s_C[(j + 1) * 64 + c0 + k0];
#pragma unroll
        for (int kl = ke; kl + 1 < CB; kl += 2) { const double2 v = *(const double2*)&s_C[(j + 1) * 64 + c0 + kl]; cjn[kl] = v.x; cjn[kl + 1] = v.y; }
      }
#pragma unroll
      for (int kl = JL + 3; kl < CB; kl++) acc[kl] = fma(-m, cjc[kl], acc[kl]);
      r0 = r0n; u = un; w = wn; c1 = c1n;
#pragma unroll
      for (int kl = 0; kl < CB; kl++) cjc[kl] = cjn[kl];
      df_own_column<NW, Q, JL + 1>(acc, cjc, r0, u, w, sa2, c1, s_C, s_M, s_R, s_col, col_base, lane);
    } else if constexpr (NW > 1) {
      const double m = acc[JL] * w;
      s_M[j * 64 + lane] = m;
      if constexpr (j + 1 < NB) { s_R[2 * j] = r0; s_R[2 * j + 1] = u; }      // (the next wave forms the pivot of column j + 1)
      df_signal(s_col, col_base + j + 1);
    }
  }
}
// in: s_L = the block (lower triangle, zeros above); out: s_X = L^-1 (full 32 x 32, exact zeros above the diagonal).
// s_C [NB][64]: column entries (the half of a row that lanes 32..63 write is never read; 16-byte aligned); s_M [NB][64]: multipliers
// (NW > 1); s_R [NB][2]: (r0, u) of a block's last column (NW > 1); s_col: an int in LDS, zero at kernel start; col_base = 32 x (factors
// this workgroup has done before) - the counter only grows.  Q: this wave's index, 0 .. NW - 1: a template parameter, so that every lane
// select, LDS offset and register index is a constant.  Returns non-zero for a bad pivot among this wave's columns.
template <int NW, int Q>
__device__ __forceinline__ int diag_factor_invert_q(double (*s_L)[NB + 1], double (*s_X)[NB + 1], double* s_C, double* s_M,
                                                    double* s_R, int* s_col, const int col_base) {
  constexpr int CB = NB / NW, c0 = CB * Q;
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));                                 // (opaque per call: the identity's entries and the LDS addresses are NOT hoisted out of the caller's column loop into dozens of registers)
  const int r = lane & 31;
  const bool inv = lane >= 32;
#ifdef ORBHIP_DF_STAMP
  const bool lane0_ = (threadIdx.x & 63) == 0; const unsigned long long t_in_ = __builtin_amdgcn_s_memrealtime();
  if (lane0_) atomicAdd(&g_df_stamp[Q][3], 1ull);
#endif
  double acc[CB], rowv[CB];
#pragma unroll
  for (int kl = 0; kl < CB; kl++) rowv[kl] = s_L[r][c0 + kl];      // (every lane reads row r; lanes 32..63 throw it away - no exec-masked loads)
#pragma unroll
  for (int kl = 0; kl < CB; kl++) acc[kl] = inv ? ((c0 + kl == r) ? 1.0 : 0.0) : rowv[kl];
  double r0 = 0.0, u = 0.0, w = 0.0;
  // ---- the columns before this wave's block, as their owners publish them (the next column's operands are requested before the
  //      current one's fmas whenever it is already there: a wave that lags catches up at issue speed, not at LDS latency)
  if constexpr (Q > 0) {
    // Two columns per trip.  The counter and BOTH columns' operands are requested in one go - counter first: the LDS serves a wave's
    // reads in order, so operands read behind a counter that already covered their column are the published ones; otherwise the trip is
    // repeated.  One LDS round trip per pair when the columns are there (the poll-then-load form needed two per column and fell a
    // microsecond behind its owner: 3.4 us per factor with four waves, most of it the three catch-ups at the block boundaries).
    // The owners signal every other column, so a pair appears together.  The last pair is peeled: its second column is the one before
    // this block, whose update follows the block's first pivot.
#define DF_LOAD(jj, m_, c_) do { m_ = s_M[(jj) * 64 + lane]; _Pragma("unroll") for (int kl = 0; kl < CB; kl += 2) { const double2 v_ = *(const double2*)&s_C[(jj) * 64 + c0 + kl]; c_[kl] = v_.x; c_[kl + 1] = v_.y; } } while (0)
#define DF_APPLY(m_, c_) do { _Pragma("unroll") for (int kl = 0; kl < CB; kl++) acc[kl] = fma(-(m_), c_[kl], acc[kl]); } while (0)
    double mA = 0.0, mB = 0.0, cA[CB], cB[CB];
#pragma unroll
    for (int kl = 0; kl < CB; kl++) { cA[kl] = 0.0; cB[kl] = 0.0; }
#pragma unroll 1
    for (int j = 0; j < c0 - 2; j += 2) {                        // (kept a loop: unrolled, the operands of every column were requested up front - 500 registers and scratch)
      for (int it = 0; it < (1 << 22); it++) {
        const int cnt = df_count(s_col);
        DF_LOAD(j, mA, cA);
        DF_LOAD(j + 1, mB, cB);
        if (cnt - col_base > j + 1) break;
      }
      DF_APPLY(mA, cA);
      DF_APPLY(mB, cB);
      asm volatile("" ::: "memory");
    }
    {
      constexpr int j = c0 - 2;
      double2 ru = {0.0, 0.0};
      for (int it = 0; it < (1 << 22); it++) {
        const int cnt = df_count(s_col);
        DF_LOAD(j, mA, cA);
        DF_LOAD(j + 1, mB, cB);
        ru = *(const double2*)&s_R[2 * (j + 1)];
        if (cnt - col_base > j + 1) break;
      }
      // the pivot of this block's first column: the owner's formula, sa from the published column, sb with column c0 - 2's update only
      acc[0] = fma(-mA, cA[0], acc[0]);
      const double qv = (cB[0] * cB[0]) * ru.x;
      const double pv = acc[0] - qv;
      const double t = fma(-qv, ru.y, pv);
      const double d = bcast_lane(t, c0);
      piv_recip(d, r0, u, w);
#pragma unroll
      for (int kl = 1; kl < CB; kl++) acc[kl] = fma(-mA, cA[kl], acc[kl]);
      DF_APPLY(mB, cB);
    }
#undef DF_LOAD
#undef DF_APPLY
  } else {
    const double d = bcast_lane(acc[0], 0);
    piv_recip(d, r0, u, w);
  }
  DF_STAMP(0);
  // ---- this wave's block: column c0 + JL; cjc[] = its entries a(k, j), k >= j + 3 in the block (requested when the column became final)
  double cjc[CB];
#pragma unroll
  for (int kl = 0; kl < CB; kl++) cjc[kl] = 0.0;
  s_C[c0 * 64 + lane] = acc[0];
  double c1 = bcast_lane(acc[0], c0 + 1);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
  for (int kl = 2; kl < CB; kl += 2) { const double2 v = *(const double2*)&s_C[c0 * 64 + c0 + kl]; cjc[kl] = v.x; cjc[kl + 1] = v.y; }
  double sa2 = acc[0] * acc[0];
  df_own_column<NW, Q, 0>(acc, cjc, r0, u, w, sa2, c1, s_C, s_M, s_R, s_col, col_base, lane);
  DF_STAMP(1);
  // ---- X(rr, c') = z(rr, c') / sqrt(d_rr) for the rows of this block; bad pivots
  // (the scale is the diagonal entry lane k itself ends up with, a(k, k) after column k - 1's update: the recurrence's d_k rounded
  // along the other path - either is a pivot of the computed elimination to within rounding, and this one costs the columns nothing)
  // - and it is already in LDS: lane k published it with column k's entries, s_C[k][k] (the slot no update reads).
  const bool mine = !inv && r >= c0 && r < c0 + CB;
  const double dmine = mine ? s_C[r * 64 + r] : 1.0;
  const int bad = __ballot(mine && __builtin_isfpclass(dmine, 0x180) == 0) != 0ull ? 1 : 0;      // anything but a positive (sub)normal number
  const double y = rsqrt_cubic(dmine);
  double xs[CB];
#pragma unroll
  for (int kl = 0; kl < CB; kl++) xs[kl] = acc[kl] * bcast_lane(y, c0 + kl);
  if (inv) {
#pragma unroll
    for (int kl = 0; kl < CB; kl++) s_X[c0 + kl][r] = xs[kl];    // column r of L^-1 (the zeros above the diagonal come out by themselves)
  }
  DF_STAMP(2);
  return bad;
}
template <int NW>
__device__ __forceinline__ int diag_factor_invert_nw(double (*s_L)[NB + 1], double (*s_X)[NB + 1], double* s_C, double* s_M, double* s_R, int* s_col,
                                                     const int col_base, const int q_in) {
  const int q = __builtin_amdgcn_readfirstlane(q_in);            // (a wave index: uniform - scalar branches, not exec-masked regions)
  if constexpr (NW == 1) return diag_factor_invert_q<1, 0>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
  else if constexpr (NW == 2) {
    if (q == 0) return diag_factor_invert_q<2, 0>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
    return diag_factor_invert_q<2, 1>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
  } else {
    if (q == 0) return diag_factor_invert_q<4, 0>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
    if (q == 1) return diag_factor_invert_q<4, 1>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
    if (q == 2) return diag_factor_invert_q<4, 2>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
    return diag_factor_invert_q<4, 3>(s_L, s_X, s_C, s_M, s_R, s_col, col_base);
  }
}
#ifdef ORBHIP_CHOL_PROF
// debug: the factor with NW = 1, 2, 4 waves on the same block, n repetitions each, for a bitwise comparison and a timing (tools/factor_ab.py)
template <int NW>
__global__ __launch_bounds__(256) void k_factor_nw(const double* __restrict__ A, double* __restrict__ X, int n, unsigned long long* ticks) {
  __shared__ double s_L[NB][NB + 1], s_X[NB][NB + 1];
  __shared__ __attribute__((aligned(16))) double s_C[NB * 64], s_M[NB * 64], s_R[2 * NB];
  __shared__ int s_col, s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) { s_col = 0; s_bad = 0; }
  for (int i = tid; i < NB * NB; i += 256) s_L[i / NB][i % NB] = (i % NB <= i / NB) ? A[i] : 0.0;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  for (int k = 0; k < n; k++) {
    if (tid < 64 * NW) { if (diag_factor_invert_nw<NW>(s_L, s_X, s_C, s_M, s_R, &s_col, NB * k, tid >> 6)) s_bad = 1; }
    __syncthreads();
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
  for (int i = tid; i < NB * NB; i += 256) X[i] = s_X[i / NB][i % NB];
  if (tid == 0) { ticks[0] = t1 - t0; ticks[1] = (unsigned long long)s_bad; }
}
#endif
#ifdef ORBHIP_TEST_HOOKS
// test hook (tests/test_gpu_diag_factor.py): nblk DIFFERENT blocks factored back to back by one workgroup, the way k_chol_wg walks the
// columns of a system - one barrier between staging a block and its factor, one between the factor and the readers of X, the counter
// base NB * b, the scratch of the previous block (s_C, s_M, s_R) left as it is.  A bad pivot is recorded per block and the walk goes on.
template <int NW>
__global__ __launch_bounds__(256) void k_factor_batch_nw(const double* __restrict__ A, double* __restrict__ X, int* __restrict__ bad, int nblk) {
  __shared__ double s_L[NB][NB + 1], s_X[NB][NB + 1];
  __shared__ __attribute__((aligned(16))) double s_C[NB * 64], s_M[NB * 64], s_R[2 * NB];
  __shared__ int s_col;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  if (tid == 0) s_col = 0;
  __syncthreads();
  for (int b = 0; b < nblk; b++) {
    const double* Ab = A + (size_t)b * NB * NB;
    for (int i = tid; i < NB * NB; i += 256) s_L[i / NB][i % NB] = (i % NB <= i / NB) ? Ab[i] : 0.0;
    __syncthreads();
    if (w < NW) {
      const int fail = diag_factor_invert_nw<NW>(s_L, s_X, s_C, s_M, s_R, &s_col, NB * b, w);
      if (fail && lane == 0) bad[b] = 1;                         // (zeroed by the host)
    }
    __syncthreads();
    double* Xb = X + (size_t)b * NB * NB;
    for (int i = tid; i < NB * NB; i += 256) Xb[i] = s_X[i / NB][i % NB];
  }
}
// test hook: the two scalar maps of the factor, element-wise (w of piv_recip, rsqrt_cubic)
__global__ __launch_bounds__(256) void k_factor_scalar_maps(const double* __restrict__ x, double* __restrict__ w_out, double* __restrict__ y_out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double r0, u, w;
  piv_recip(x[i], r0, u, w);
  w_out[i] = w;
  y_out[i] = rsqrt_cubic(x[i]);
}
#endif
// G = groups of 16 L21 rows per wave.  Every workgroup repeats the diagonal factor, so a lockstep batch (throughput-bound)
// runs G = 4 (256 rows per workgroup: 3.3x fewer repeated factors at n = 600, +8 % solves/s), while a single problem
// (latency-bound) runs G = 1: with G = 4 its L21 loads - 16 rows x 32 bytes per instruction, the MFMA operand layout -
// concentrate on 3 CUs instead of 10 and the panel takes 18 us instead of 9.8.  Same arithmetic per row either way.
template <int G>
__global__ __launch_bounds__(256) void k_chol_panel(const BaDev* __restrict__ Dv, int k) {
  const BaDev D = Dv[blockIdx.y];
  if (D.chol_la) return;                                      // factored by k_chol_la
  BaState* st = D.st;
  const StFlags F = ld_flags(st);
  __shared__ double s_L[NB][NB + 1];
  __shared__ double s_X[NB][NB + 1];
  __shared__ __attribute__((aligned(16))) double s_T[NB][64];   // column broadcast buffer of the factor
  __shared__ int s_fail;
  const int np = D.npad, tid = threadIdx.x;
  if (k >= np || k + NB + (int)blockIdx.x * (64 * G) > np) return;     // beyond this problem's matrix (batched launch)
  double* S = D.S;
  // this wave's G x 16 rows of A21 do not depend on the diagonal factor: their loads are issued first and land while wave 0 factors
  const int w = tid >> 6, lane = tid & 63;
  const int row0 = k + NB + (blockIdx.x * 4 + w) * (16 * G);
  const int li = lane & 15, lk = lane >> 4;
  double a[G][8];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int arow = row0 + 16 * g + li;
#pragma unroll
    for (int ks = 0; ks < 8; ks++) a[g][ks] = (arow <= np) ? S[(size_t)arow * np + k + 4 * ks + lk] : 0.0;
  }
  double d4[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const int i = tid + 256 * u, r = i / NB, c = i % NB; d4[u] = (c <= r) ? S[(size_t)(k + r) * np + k + c] : 0.0; }
  // (the state flags are read AFTER the matrix loads are in flight: one dependent global round trip less per launch;
  // S is a valid allocation for finished problems too)
  if (F.done || !F.valid || F.chol_fail) return;
#pragma unroll
  for (int u = 0; u < 4; u++) { const int i = tid + 256 * u; s_L[i / NB][i % NB] = d4[u]; }
  if (tid == 0) s_fail = 0;
  __syncthreads();
  if (tid < 64) {
    const int fail = diag_factor_invert_nw<1>(s_L, s_X, &s_T[0][0], nullptr, nullptr, nullptr, 0, 0);
    if (fail && tid == 0) s_fail = 1;
  }
  __syncthreads();
  if (s_fail) { if (tid == 0 && blockIdx.x == 0) st->chol_fail = 1; return; }
  if (blockIdx.x == 0) {
    double* Di = D.Dinv + (size_t)(k / NB) * NB * NB;
    for (int i = tid; i < NB * NB; i += 256) {
      int r = i / NB, c = i % NB;
      // (L11 itself is NOT written back: nothing downstream reads it - the substitutions use L11^-1 - and the other
      // workgroups of this launch, which factor the same block redundantly, may still be reading the unfactored one)
      Di[i] = s_X[r][c];
    }
  }
  // ---- L21 rows: X = A * Linv^T on the matrix cores --------------------------------------------------
  double b0[8], b1[8];
#pragma unroll
  for (int ks = 0; ks < 8; ks++) { b0[ks] = s_X[li][4 * ks + lk]; b1[ks] = s_X[16 + li][4 * ks + lk]; }     // B[k][j] = Linv[j][k]
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int rg0 = row0 + 16 * g;
    if (rg0 > np) break;
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g][ks], b0[ks], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g][ks], b1[ks], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int rg = 0; rg < 4; rg++) {
      const int orow = rg0 + (lane >> 4) + 4 * rg;
      if (orow <= np) {
        S[(size_t)orow * np + k + (lane & 15)] = acc0[rg];
        S[(size_t)orow * np + k + 16 + (lane & 15)] = acc1[rg];
      }
    }
  }
}

// trailing update C -= L[:, kcol:kcol+K] * L[:, kcol:kcol+K]^T on the FP64 matrix cores for the rows >= r_lo and the
// columns [c_lo, c_hi) of the lower triangle; one 64x64 tile per workgroup, each of the 4 waves owns a 32x32 quadrant
// as 2x2 v_mfma_f64_16x16x4_f64 tiles, K (32..128) is walked in 32-wide LDS stages.  Two-level blocking: the four
// 32-wide panels of a 128-wide outer block only update the rest of that block ("thin" launches, K=32); everything to
// the right of the outer block is updated ONCE with K=128 (4x the flops per byte of C moved).  Workgroups with
// blockIdx.x >= ntiles update the augmented rhs row (row npad) over the same column range.
__device__ __forceinline__ void chol_syrk_body(const BaDev& D, const BaState* st, const int bx, int kcol, int K, int r_lo, int c_lo, int c_hi_cap, int tiles_c, int ntiles,
                                               double (*s_A)[NB + 1], double (*s_B)[NB + 1], int c_rhs_min = 0) {
  const StFlags F = ld_flags(st);
  const int np = D.npad, tid = threadIdx.x;
  // batched launch: the grid and (kcol, K, r_lo, c_lo, c_hi_cap) are laid out for the LARGEST reduced system of the batch;
  // this problem clips the column range to its own size and drops the steps / tiles that fall outside
  const int c_hi = min(c_hi_cap, np);
  if (kcol + K > np || c_hi <= c_lo) return;
  double* S = D.S;
  if (bx >= ntiles) {           // augmented rhs row
    if (F.done || !F.valid || F.chol_fail) return;
    double* zrow = S + (size_t)np * np;
    double* s_z = &s_A[0][0];
    for (int i = tid; i < K; i += 256) s_z[i] = zrow[kcol + i];
    __syncthreads();
    const int c = c_lo + (bx - ntiles) * 256 + tid;
    if (c < c_hi && c >= c_rhs_min) {
      const double* L = S + (size_t)c * np + kcol;
      double sum = 0.0;
      for (int m = 0; m < K; m++) sum += L[m] * s_z[m];
      zrow[c] -= sum;
    }
    return;
  }
  const int ti = bx / tiles_c, tj = bx - ti * tiles_c;
  const int r0 = r_lo + ti * 64, c0 = c_lo + tj * 64;
  if (r0 + 63 < c0 || r0 >= np || c0 >= c_hi) return;         // tile entirely above the diagonal / outside this problem
  const int w = tid >> 6, lane = tid & 63;
  const int qr = (w >> 1) * 32, qc = (w & 1) * 32;            // quadrant origin inside the 64x64 tile
  const bool qskip = (r0 + qr + 31 < c0 + qc);                // quadrant entirely above the diagonal
  double4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  const int li = lane & 15, lk = lane >> 4;                   // A[i=lane&15][k=lane>>4], B[k=lane>>4][j=lane&15]
  // the first K stage and this lane's C entries are requested before the state flags are looked at (one dependent
  // global round trip less per launch), and C no longer waits for the matrix-core loop to finish
  double va[8], vb[8], cpre[2][2][4];
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int i = tid + 256 * u, r = i / NB, c = i % NB;
    va[u] = (r0 + r < np) ? S[(size_t)(r0 + r) * np + kcol + c] : 0.0;
    vb[u] = (c0 + r < c_hi) ? S[(size_t)(c0 + r) * np + kcol + c] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int row = r0 + qr + 16 * i + (lane >> 4) + 4 * rg;
        const int col = c0 + qc + 16 * j + (lane & 15);
        cpre[i][j][rg] = (!qskip && row < np && col < c_hi && col <= row) ? S[(size_t)row * np + col] : 0.0;
      }
  if (F.done || !F.valid || F.chol_fail) return;
  for (int k0 = 0; k0 < K; k0 += NB) {
    __syncthreads();
    if (k0 > 0) {
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = tid + 256 * u, r = i / NB, c = i % NB;
        va[u] = (r0 + r < np) ? S[(size_t)(r0 + r) * np + kcol + k0 + c] : 0.0;
        vb[u] = (c0 + r < c_hi) ? S[(size_t)(c0 + r) * np + kcol + k0 + c] : 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) { const int i = tid + 256 * u; s_A[i / NB][i % NB] = va[u]; s_B[i / NB][i % NB] = vb[u]; }
    __syncthreads();
    if (!qskip) {
#pragma unroll
      for (int kk = 0; kk < NB; kk += 4) {
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; i++) a[i] = s_A[qr + 16 * i + li][kk + lk];
#pragma unroll
        for (int j = 0; j < 2; j++) b[j] = s_B[qc + 16 * j + li][kk + lk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  }
  if (qskip) return;
  // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int row = r0 + qr + 16 * i + (lane >> 4) + 4 * rg;
        const int col = c0 + qc + 16 * j + (lane & 15);
        if (row < np && col < c_hi && col <= row) S[(size_t)row * np + col] = cpre[i][j][rg] - acc[i][j][rg];
      }
}

__global__ __launch_bounds__(256) void k_chol_syrk(const BaDev* __restrict__ Dv, int kcol, int K, int r_lo, int c_lo, int c_hi_cap, int tiles_c, int ntiles) {
  const BaDev D = Dv[blockIdx.y];
  if (D.chol_la) return;                                      // factored by k_chol_la
  __shared__ double s_A[64][NB + 1], s_B[64][NB + 1];
  chol_syrk_body(D, D.st, (int)blockIdx.x, kcol, K, r_lo, c_lo, c_hi_cap, tiles_c, ntiles, s_A, s_B);
}

// ---- look-ahead Cholesky step for reduced systems up to 1024 unknowns (LocalBA: 600) -----------------------------------
// The two-level scheme above is a chain of panel -> update -> panel ... launches; at n = 600 every launch is latency-bound
// (9.8 + 6.1 us per step).  Here ONE launch per 32-column step carries both roles:
//   role A (first nA workgroups): panel k.  The rank-32 update of the PREVIOUS step is applied to this column block inside
//     the kernel: the diagonal block as D -= P P^T before it is factored (P = the previous panel's rows of the diagonal
//     block), and the rows below algebraically, L21 = A21 X^T - Lprev (X P)^T with X = L11^-1 - both operand sets are
//     loaded straight into the MFMA layout before the factor starts, M = X P costs 8 MFMAs per wave after the inverse;
//   role B (remaining workgroups): the previous step's update of everything to the RIGHT of this column block (and of the
//     augmented rhs row) - the old k_chol_syrk body, now off the critical path because it runs beside the factor.
// Same launch count as panels alone; deterministic (fixed MFMA order).
// Larger systems (hybrid = 1: the problems with chol_la == 0) run the same kernel INSIDE each 128-column outer block of the
// two-level scheme: k0 = first column of the outer block (its first step has no pending update: everything older was applied
// by the K = 128 updates), c_cap = its end (role B stops there; the rest of the matrix gets the four panels at once).
//   role C (workgroups behind role B): a share of the PREVIOUS outer block's K = 128 update of everything to the right of
//     this outer block.  That update is needed only after this block's steps, so it is taken off the serial chain and dealt
//     out over this block's launches (tile t goes to step t mod nq), beside the latency-bound panel work.  (A second stream
//     joined by events inside the captured graph was tried first: ~40 us per fork / join, slower than no overlap at all.)
struct CholWide { int kcol, K, lo, tiles_c, total, nrhs, q, nq; };     // total = tiles of the whole update; nq = 0: no role C
template <int G>
__global__ __launch_bounds__(256) void k_chol_la(const BaDev* __restrict__ Dv, int k, int k0, int c_cap, int nA, int tiles_c, int ntiles, int nB, int hybrid, CholWide wd) {
  const BaDev D = Dv[blockIdx.y];
  if ((D.chol_la != 0) == (hybrid != 0)) return;
  BaState* st = D.st;
  const StFlags F = ld_flags(st);
  __shared__ __attribute__((aligned(16))) double s_raw[4 * NB * (NB + 1) + NB * 64];
  const int np = D.npad, tid = threadIdx.x;
  if ((int)blockIdx.x >= nA) {
    double (*s_A)[NB + 1] = (double (*)[NB + 1])s_raw;
    double (*s_B)[NB + 1] = (double (*)[NB + 1])(s_raw + 64 * (NB + 1));
    const int bb = (int)blockIdx.x - nA;
    if (bb < nB) chol_syrk_body(D, st, bb, k - NB, NB, k + NB, k + NB, c_cap, tiles_c, ntiles, s_A, s_B);
    else {
      const int wi = bb - nB, cnt = (wd.total - wd.q + wd.nq - 1) / wd.nq;          // this step's tiles: q, q + nq, q + 2 nq, ...
      const int bx = wi < cnt ? wd.q + wi * wd.nq : wd.total + (wi - cnt);           // behind them (step 0 only): the rhs-row workgroups
      chol_syrk_body(D, st, bx, wd.kcol, wd.K, wd.lo, wd.lo, INT_MAX, wd.tiles_c, wd.total, s_A, s_B);
    }
    return;
  }
  double (*s_L)[NB + 1] = (double (*)[NB + 1])s_raw;
  double (*s_X)[NB + 1] = (double (*)[NB + 1])(s_raw + NB * (NB + 1));
  double (*s_P)[NB + 1] = (double (*)[NB + 1])(s_raw + 2 * NB * (NB + 1));
  double (*s_T)[64] = (double (*)[64])(s_raw + 4 * NB * (NB + 1));          // 16-byte aligned: 4 * 32 * 33 * 8 bytes
  __shared__ int s_fail;
  if (k >= np || k + NB + (int)blockIdx.x * (64 * G) > np) return;     // beyond this problem's matrix (batched launch)
  CHOL_PROF_BEGIN(k / NB);
  double* S = D.S;
  const bool upd = k > k0;
  const int kp = k - NB;
  const int w = tid >> 6, lane = tid & 63;
  const int row0 = k + NB + (blockIdx.x * 4 + w) * (16 * G);
  const int li = lane & 15, lk = lane >> 4;
  // request order = need order: the two 32x32 blocks the factor waits for first, the L21 operands behind them
  double d4[4], p4[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = tid + 256 * u, r = i / NB, c = i % NB;
    d4[u] = (c <= r) ? S[(size_t)(k + r) * np + k + c] : 0.0;
    p4[u] = upd ? S[(size_t)(k + r) * np + kp + c] : 0.0;
  }
  // G = 1 (one problem at a time: latency): the L21 operands of this wave's rows are requested HERE, before the factor, and
  // wait in registers.  G = 4 (lockstep batches: throughput): they are loaded where they are used instead - 128 registers
  // less, so that the kernel fits two waves per SIMD (338 -> <= 256 registers; the trailing-update workgroups of the same
  // launch, which are the majority, were held to one workgroup per CU by the panel role's register count).
  constexpr bool EARLY = (G == 1);
  double a[EARLY ? G : 1][8], ap[EARLY ? G : 1][8];
  if constexpr (EARLY) {
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int arow = row0 + 16 * g + li;
#pragma unroll
      for (int ks = 0; ks < 8; ks++) {
        a[g][ks] = (arow <= np) ? S[(size_t)arow * np + k + 4 * ks + lk] : 0.0;
        ap[g][ks] = (upd && arow <= np) ? -S[(size_t)arow * np + kp + 4 * ks + lk] : 0.0;      // negated: A21 + P (-Lprev)^T
      }
    }
  }
  if (F.done || !F.valid || F.chol_fail) return;
#pragma unroll
  for (int u = 0; u < 4; u++) { const int i = tid + 256 * u; s_L[i / NB][i % NB] = d4[u]; s_P[i / NB][i % NB] = p4[u]; }
  if (tid == 0) s_fail = 0;
  __syncthreads();
  CHOL_STAMP(0);                                              // loads landed
  const int ti = w >> 1, tj = w & 1;                         // this wave's 16x16 tile of the 32x32 products
  // The previous step's rank-32 update of THIS column block's rows below the diagonal, A21 <- A21 - Lprev P^T, on the matrix
  // cores before the factor starts (round 3: it used to be folded algebraically into the product behind the factor,
  // L21 = A21 X^T - Lprev (X P)^T, which put M = X P and a barrier on the serial chain).  a[ks] is at once the MFMA A operand
  // of k-step ks and - the same register - row (lane >> 4) + 4 (ks & 3) of the 16 x 16 C tile ks >> 2 of A21^T, so the update
  // accumulates INTO it: tile t of A21'^T = A21^T + P (-Lprev)^T with P's rows 16 t .. as the A operand and ap as the B operand.
  auto apply_prev = [&](double (&av)[8], const double (&apv)[8]) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
      double4_t acc = {av[4 * t], av[4 * t + 1], av[4 * t + 2], av[4 * t + 3]};
#pragma unroll
      for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * t + li][4 * ks + lk], apv[ks], acc, 0, 0, 0);
      av[4 * t] = acc[0]; av[4 * t + 1] = acc[1]; av[4 * t + 2] = acc[2]; av[4 * t + 3] = acc[3];
    }
  };
  if (upd) {
    if (tj <= ti) {                                           // D -= P P^T on the lower tiles
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * ti + li][4 * ks + lk], s_P[16 * tj + li][4 * ks + lk], acc, 0, 0, 0);
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int r = 16 * ti + (lane >> 4) + 4 * rg, c = 16 * tj + (lane & 15);
        if (c <= r) s_L[r][c] -= acc[rg];
      }
    }
    __syncthreads();
  }
  CHOL_STAMP(1);                                              // D -= P P^T
  if (tid < 64) {
    const int fail = diag_factor_invert_nw<1>(s_L, s_X, &s_T[0][0], nullptr, nullptr, nullptr, 0, 0);
    if (fail && tid == 0) s_fail = 1;
    CHOL_STAMP(2);                                            // factor + inverse
  } else if (upd) {                                           // waves 1..3 bring their rows up to date beside the factor ...
    if constexpr (EARLY) {
#pragma unroll
      for (int g = 0; g < G; g++) apply_prev(a[g], ap[g]);
    }
  }
  __syncthreads();
  CHOL_STAMP(3);
  if (s_fail) { if (tid == 0 && blockIdx.x == 0) st->chol_fail = 1; return; }
  if (tid < 64 && upd) {                                      // ... wave 0 behind it
    if constexpr (EARLY) {
#pragma unroll
      for (int g = 0; g < G; g++) apply_prev(a[g], ap[g]);
    }
  }
  // ---- L21 rows on the matrix cores: A21' X^T ----------------------------------------------------------------------------
  double b0[8], b1[8];
#pragma unroll
  for (int ks = 0; ks < 8; ks++) { b0[ks] = s_X[li][4 * ks + lk]; b1[ks] = s_X[16 + li][4 * ks + lk]; }     // B[k][j] = X[j][k]
  CHOL_STAMP(4);                                              // operand reads
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int rg0 = row0 + 16 * g;
    if (rg0 > np) break;
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const int gi = EARLY ? g : 0;
    if constexpr (!EARLY) {
      const int arow = rg0 + li;
#pragma unroll
      for (int ks = 0; ks < 8; ks++) {
        a[0][ks] = (arow <= np) ? S[(size_t)arow * np + k + 4 * ks + lk] : 0.0;
        ap[0][ks] = (upd && arow <= np) ? -S[(size_t)arow * np + kp + 4 * ks + lk] : 0.0;
      }
    }
    if constexpr (!EARLY) { if (upd) apply_prev(a[0], ap[0]); }
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[gi][ks], b0[ks], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[gi][ks], b1[ks], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int rg = 0; rg < 4; rg++) {
      const int orow = rg0 + (lane >> 4) + 4 * rg;
      if (orow <= np) {
        S[(size_t)orow * np + k + (lane & 15)] = acc0[rg];
        S[(size_t)orow * np + k + 16 + (lane & 15)] = acc1[rg];
      }
    }
  }
  CHOL_STAMP(5);                                              // L21 on the matrix cores + stores
  if (blockIdx.x == 0) {                                      // L11 and L11^-1 leave last: nothing in this launch waits for them
    double* Di = D.Dinv + (size_t)(k / NB) * NB * NB;
    for (int i = tid; i < NB * NB; i += 256) {
      int r = i / NB, c = i % NB;
      // (L11 itself is NOT written back: nothing downstream reads it - the substitutions use L11^-1 - and the other
      // workgroups of this launch, which factor the same block redundantly, may still be reading the unfactored one)
      Di[i] = s_X[r][c];
    }
  }
  CHOL_STAMP(6);                                              // L11^-1 store
}

// ---- problem-parallel Cholesky for LOCKSTEP BATCHES: one workgroup factors one reduced system (<= 1024 unknowns) ------------
// Round 4 (VERDICT r3 next #1a).  A lockstep batch used to walk one k_chol_la<4> launch per 32-column step: 19 launches per LM
// iteration at C4 size, every one a panel + a rank-32 update that reads and writes the whole trailing matrix (18 MB per
// factorisation), every panel workgroup repeating the diagonal factor - 24 % of a batched solve.  A batch has many systems, so
// the parallelism can come from the PROBLEMS instead: one 512-thread workgroup per system, no flags, no co-residency
// requirement, no launch chain.  The schedule is LEFT-looking by block column: the tiles (i, c) of column c are brought up to
// date in registers from the finished columns j < c (read once per column: 9.4 MB per factorisation, written once: 1.5 MB),
// eight block rows at a time - one 32 x 32 tile per wave; per step j the workgroup stages L(c, j) and the eight L(i, j) in LDS
// (the next step's loads are in flight during the matrix-core loop).
// The ARITHMETIC is the step kernels', operation for operation, so results are bit-identical to k_chol_la / k_chol_persist
// and a batched solve stays bit-identical to single calls (tests/test_gpu_ba.py):
//   tile (i, c), i > c:  T = A(i, c); for j = 0 .. c-2: T = T - (eight MFMA k-steps of L(i, j) L(c, j)^T from zero)   [chol_syrk_body]
//                        j = c-1: T'^T accumulated on the matrix cores from T^T with P = L(c, c-1), -L(i, c-1)       [apply_prev]
//                        L(i, c) = T' X_c^T (eight k-steps from zero), X_c = L(c, c)^-1
//   diagonal tile:       the syrk form for every j <= c-1, lower triangle; factor + inverse by two waves (diag_factor_invert_2w:
//                        the one-wave function's bits)
//   rhs row (row npad):  z_c -= sum_m L(c, 32 j + m) z(32 j + m) for j <= c-2 (sequential mul / add per column, VALU), then the
//                        row's last update and the multiplication by X_c^T on the matrix cores as a 16-row tile whose first
//                        row is z and whose other rows are zero (k_chol_la's role A sees the row exactly like that).
#define CW_BAND_MAX 30                 /* a system of more than 32 block rows is factored by the look-ahead family only when no row's envelope is wider than this (the list of a column's active rows: NB + 2 entries) */
#define CW_TPB 256
#define CW_NW (CW_TPB / 64)
#ifndef CW_RPW
#define CW_RPW 2                       /* block rows per wave and group: eight rows of a column are in flight per workgroup */
#endif
#define CW_NSCA (CW_RPW == 1 ? CW_NW - 1 : CW_NW * CW_RPW)      /* scratch tiles: with one row per wave, wave 0 borrows D_c's tile (it is the diagonal wave in the group that factors) */
#define CW_TILE (NB * (NB + 1))
/* LDS: L(c, j) twice (double buffer), a scratch tile per (wave, row slot), X_c, D_c, the factor's column buffer, the rhs row's
   z(j) twice: 118 KB - one workgroup per CU, which the register count (one wave per SIMD, three operand sets in flight) implies anyway */
#define CW_LDS_DOUBLES ((4 + CW_NSCA) * CW_TILE + NB * 64 + 2 * NB + NB * 64 + 2 * NB)      /* ... + the factor's multipliers and (r0, u) pairs */
#if CW_RPW == 1
#define CW_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#else
#define CW_ATTR
#endif
__global__ __launch_bounds__(CW_TPB) CW_ATTR void k_chol_wg(const BaDev* __restrict__ Dv) {
  const BaDev D = Dv[blockIdx.x];
  if (!D.chol_la) return;
  BaState* st = D.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.valid || F.chol_fail) return;
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  constexpr int NSC = CW_NW * CW_RPW, NSCA = CW_NSCA;
  double (*s_X)[NB + 1] = (double (*)[NB + 1])(s_dyn + (2 + NSCA) * CW_TILE);
  double (*s_L)[NB + 1] = (double (*)[NB + 1])(s_dyn + (3 + NSCA) * CW_TILE);
  double (*s_T)[64] = (double (*)[64])(s_dyn + (4 + NSCA) * CW_TILE);           // 16-byte aligned: a multiple of 32 * 33 * 8 bytes
  double* s_z = s_dyn + (4 + NSCA) * CW_TILE + NB * 64;                         // [2][NB]
  double* s_M = s_z + 2 * NB;                                                   // [NB][64]: the factor's multipliers (16-byte aligned)
  double* s_R = s_M + NB * 64;                                                  // [NB][2]
  __shared__ int s_fail, s_col, s_nrows;
  __shared__ int s_rows[NB + 2];                               // the ACTIVE rows of the current column (skyline), ascending
  const int* __restrict__ tf = D.tile_first;
  const int np = D.npad, nb = np / NB, tid = threadIdx.x;
  const int w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  double* S = D.S;
  double* zrow = S + (size_t)np * np;
  if (tid == 0) { s_fail = 0; s_col = 0; }
  const int lrow = tid >> 4, lcol = 2 * (tid & 15);             // this thread's entries of the staged L(c, j): rows lrow and lrow + 16
  __syncthreads();
  for (int c = 0; c < nb; c++) {
    const size_t cb = (size_t)c * NB;
    // SKYLINE (round 5; host: tile_first).  Tile (i, c) is structurally zero - and stays zero in L - unless tile_first[i] <= c, and
    // L(c, j) = 0 for j < tile_first[c]: the column's rows are the ACTIVE ones only (wave 0 compacts them), its update steps start at
    // j0 = tile_first[c], and a row skips the steps before its own first column.  What is skipped is a subtraction of an exact zero
    // (eight MFMA k-steps from zero with a zero operand) or a product with a zero tile: the bits of every entry are those of the dense
    // walk (the step kernels still make it; tests/test_gpu_ba.py compares).  A banded reduced system - a map whose points are seen by a
    // few consecutive keyframes: C4 of the bench has 55 active tiles of 190 and 55 tile updates of 1140 - costs its band; a dense one
    // costs what it did.
    if (w == 0) {
      // (64 rows per ballot; a system comes here only when no column has more active rows than the list holds - csrc/ba_host.inc; the
      // rhs row is always active and goes last)
      int n = 0;
      for (int base = c; base < nb; base += 64) {
        const int i = base + lane;
        const bool actv = i < nb && (i == c || tf[min(i, nb)] <= c);
        const unsigned long long m = __ballot(actv);
        if (actv) s_rows[n + __popcll(m & ((1ull << lane) - 1ull))] = i;
        n += __popcll(m);
      }
      if (lane == 0) { s_rows[n] = nb; s_nrows = n + 1; }
    }
    __syncthreads();
    const int nrows = s_nrows;
    const int j0 = min(tf[c], c);
    const bool upd = j0 < c;
    // rows of this column: c (the diagonal tile), the active ones of c + 1 .. nb - 1, and nb = the rhs row; CW_NW * CW_RPW at a time,
    // wave w takes the entries g0 + w and g0 + w + CW_NW of the list
    for (int g0 = 0; g0 < nrows; g0 += NSC) {
      CHOL_PROF_BEGIN(c);
      int my[CW_RPW], fi[CW_RPW]; bool valid[CW_RPW], is_diag[CW_RPW], is_rhs[CW_RPW], is_row[CW_RPW];
      double T[CW_RPW][2][2][4];
      double zc = 0.0;
#pragma unroll
      for (int t = 0; t < CW_RPW; t++) {
        my[t] = (g0 + w + CW_NW * t < nrows) ? s_rows[g0 + w + CW_NW * t] : nb + 1;
        valid[t] = my[t] <= nb; is_diag[t] = my[t] == c; is_rhs[t] = my[t] == nb; is_row[t] = valid[t] && !is_diag[t] && !is_rhs[t];
        fi[t] = is_row[t] ? tf[my[t]] : 0;                       // (the row's L(i, j) is zero for j < fi: those steps are skipped, except the last one, whose tile the last update reads)
        const size_t rb = (size_t)my[t] * NB;
#pragma unroll
        for (int I = 0; I < 2; I++)
#pragma unroll
          for (int J = 0; J < 2; J++)
#pragma unroll
            for (int rg = 0; rg < 4; rg++)
              T[t][I][J][rg] = (valid[t] && !is_rhs[t]) ? S[(rb + 16 * I + lk + 4 * rg) * np + cb + 16 * J + li] : 0.0;
        if (is_rhs[t] && lane < NB) zc = zrow[cb + lane];
      }
      // ---- the updates j = j0 .. c-1.  L(c, j), which every row of the column needs, is staged in LDS by the whole workgroup
      // (double buffer, ONE barrier per step); a wave's own L(i, j) come straight from global memory in the MFMA operand layout
      // (a first version staged them in LDS as well: two barriers and an LDS round trip per step).  Two register sets in
      // rotation: step j computes from set (j - j0) & 1 (64 MFMAs per wave, ~1.8 us) while the loads of step j + 1 are in flight.
      // (round 5) L(i, j) is fetched COALESCED - a lane takes 16 bytes, a load instruction four whole 256-byte tile rows - and turned
      // into the MFMA operand layout through the slot's own scratch tile (free during the update loop; wave-private: no barrier).  The
      // operand-layout loads they replace (8 bytes per lane, 16 rows x 32 bytes per instruction) touched every cache line of a tile
      // eight times: 512 line requests per tile instead of 64, as many cycles of the CU's address pipeline per step as the step's 256
      // MFMAs take on the matrix pipes.  Same values, same products: nothing changes in the arithmetic.
      struct Stage { double A[CW_RPW][16]; double2 pb[2]; double z; };    // A: [2 q], [2 q + 1] = L(i, j)[4 q + lk][2 li], [2 li + 1] (as loaded); this thread's share of L(c, j); z(j)
      Stage G0, G1;
#pragma unroll
      for (int t = 0; t < CW_RPW; t++)
#pragma unroll
        for (int k = 0; k < 16; k++) { G0.A[t][k] = 0.0; G1.A[t][k] = 0.0; }
      G0.z = G1.z = 0.0;
      auto issue = [&](int j, Stage& G) {
        const size_t jb = (size_t)j * NB;
#pragma unroll
        for (int h = 0; h < 2; h++) G.pb[h] = *(const double2*)&S[(cb + lrow + 16 * h) * np + jb + lcol];
#pragma unroll
        for (int t = 0; t < CW_RPW; t++) {
          if (is_row[t] && (j >= fi[t] || j == c - 1)) {
            const size_t rb = (size_t)my[t] * NB;
#pragma unroll
            for (int q = 0; q < 8; q++) { const double2 v = *(const double2*)&S[(rb + 4 * q + lk) * np + jb + 2 * li]; G.A[t][2 * q] = v.x; G.A[t][2 * q + 1] = v.y; }
          }
          if (is_rhs[t] && lane < NB) G.z = zrow[jb + lane];
        }
      };
      auto step = [&](int j, const Stage& Gc, Stage& Gn) {
        const int par = (j - j0) & 1;
        const bool last = j == c - 1;
        double (*s_B)[NB + 1] = (double (*)[NB + 1])(s_dyn + par * CW_TILE);
#pragma unroll
        for (int h = 0; h < 2; h++) { s_B[lrow + 16 * h][lcol] = Gc.pb[h].x; s_B[lrow + 16 * h][lcol + 1] = Gc.pb[h].y; }
        if ((is_rhs[0] || is_rhs[CW_RPW - 1]) && lane < NB) s_z[par * NB + lane] = Gc.z;
        __syncthreads();                                         // (buffer `par` was last read in step j - 2: every wave has passed step j - 1's barrier since)
        if (j + 1 < c) issue(j + 1, Gn);
        double b0[8], b1[8];
#pragma unroll
        for (int ks = 0; ks < 8; ks++) { b0[ks] = s_B[li][4 * ks + lk]; b1[ks] = s_B[16 + li][4 * ks + lk]; }
        // the rows' L(i, j): as loaded -> the slot's scratch tile -> operand layout (every slot's write first, then slot after slot)
#pragma unroll
        for (int t = 0; t < CW_RPW; t++) {
          if (is_row[t] && (j >= fi[t] || last)) {
            double (*s_Sw)[NB + 1] = (double (*)[NB + 1])(s_dyn + (CW_RPW == 1 ? (w == 0 ? 3 + NSCA : 1 + w) : 2 + CW_RPW * w + t) * CW_TILE);
#pragma unroll
            for (int q = 0; q < 8; q++) { s_Sw[4 * q + lk][2 * li] = Gc.A[t][2 * q]; s_Sw[4 * q + lk][2 * li + 1] = Gc.A[t][2 * q + 1]; }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < CW_RPW; t++) {
          double opA[16];
#pragma unroll
          for (int k = 0; k < 16; k++) opA[k] = 0.0;
          if (is_row[t] && j >= fi[t] && !last) {
            const double (*s_Sw)[NB + 1] = (const double (*)[NB + 1])(s_dyn + (CW_RPW == 1 ? (w == 0 ? 3 + NSCA : 1 + w) : 2 + CW_RPW * w + t) * CW_TILE);
#pragma unroll
            for (int I = 0; I < 2; I++)
#pragma unroll
              for (int ks = 0; ks < 8; ks++) opA[8 * I + ks] = s_Sw[16 * I + li][4 * ks + lk];
            // (after the last step the tile still holds L(i, c-1): the last update below reads its operand from there)
          }
          if (is_rhs[t]) {
            if (!last && lane < NB) {                            // k_chol_la's rhs role: sequential mul / add, then one subtraction
              const double* z = s_z + par * NB;
              double sum = 0.0;
#pragma unroll
              for (int m = 0; m < NB; m++) sum += s_B[lane][m] * z[m];
              zc -= sum;
            }
          } else if (is_diag[t] || (is_row[t] && !last && j >= fi[t])) {       // chol_syrk_body: eight k-steps from zero, then C - acc
            double4_t acc[2][2];
#pragma unroll
            for (int I = 0; I < 2; I++)
#pragma unroll
              for (int J = 0; J < 2; J++) acc[I][J] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {
              const double a0 = is_diag[t] ? b0[ks] : opA[ks], a1 = is_diag[t] ? b1[ks] : opA[8 + ks];
              acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0[ks], acc[0][0], 0, 0, 0);
              acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1[ks], acc[0][1], 0, 0, 0);
              acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0[ks], acc[1][0], 0, 0, 0);
              acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1[ks], acc[1][1], 0, 0, 0);
            }
#pragma unroll
            for (int I = 0; I < 2; I++)
#pragma unroll
              for (int J = 0; J < 2; J++)
#pragma unroll
                for (int rg = 0; rg < 4; rg++) T[t][I][J][rg] = T[t][I][J][rg] - acc[I][J][rg];
          }
        }
      };
      if (upd) issue(j0, G0);
      CHOL_STAMP(0);                                             // T requested, first loads issued
      for (int j = j0; j < c; j += 2) {
        step(j, G0, G1);
        if (j + 1 < c) step(j + 1, G1, G0);
      }
      CHOL_STAMP(1);                                             // the update steps
      // (after the loop: P = L(c, c-1) is in LDS buffer (c - 1 - j0) & 1, this wave's L(i, c-1) in its scratch tile, z(c-1) in s_z)
      const double (*s_P)[NB + 1] = (const double (*)[NB + 1])(s_dyn + ((c - 1 - j0) & 1) * CW_TILE);
      // ---- T goes from the C layout of its updates to the A-operand layout through the slot's scratch tile (the step kernels make
      // the same trip through global memory); the tile's last update rides on the way (k_chol_la's apply_prev: the registers are
      // rows of the C tiles of A^T).  a[t][I][ks]: rows 16 I .. of T', operand layout.
      double a[CW_RPW][2][8];
#pragma unroll
      for (int t = 0; t < CW_RPW; t++) {
        double (*s_Sw)[NB + 1] = (double (*)[NB + 1])(s_dyn + (CW_RPW == 1 ? (w == 0 ? 3 + NSCA : 1 + w) : 2 + CW_RPW * w + t) * CW_TILE);
#pragma unroll
        for (int I = 0; I < 2; I++)
#pragma unroll
          for (int ks = 0; ks < 8; ks++) a[t][I][ks] = 0.0;
        if (valid[t] && !is_diag[t]) {
          double ap[2][8];
#pragma unroll
          for (int I = 0; I < 2; I++)
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {
              double v = 0.0;
              if (upd) {
                if (!is_rhs[t]) v = -s_Sw[16 * I + li][4 * ks + lk];      // L(i, c-1), left in the slot's tile by the last update step
                else if (I == 0 && li == 0) v = -s_z[((c - 1 - j0) & 1) * NB + 4 * ks + lk];
              }
              ap[I][ks] = v;
            }
          if (is_rhs[t]) { if (lane < NB) s_Sw[0][lane] = zc; }
          else {
#pragma unroll
            for (int I = 0; I < 2; I++)
#pragma unroll
              for (int J = 0; J < 2; J++)
#pragma unroll
                for (int rg = 0; rg < 4; rg++) s_Sw[16 * I + lk + 4 * rg][16 * J + li] = T[t][I][J][rg];
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int I = 0; I < 2; I++)
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {
              double v = 0.0;
              if (!is_rhs[t]) v = s_Sw[16 * I + li][4 * ks + lk]; else if (I == 0 && li == 0) v = s_Sw[0][4 * ks + lk];
              a[t][I][ks] = v;
            }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
          if (upd) {
#pragma unroll
            for (int I = 0; I < 2; I++) {
              if (is_rhs[t] && I == 1) break;
#pragma unroll
              for (int q = 0; q < 2; q++) {
                double4_t acc = {a[t][I][4 * q], a[t][I][4 * q + 1], a[t][I][4 * q + 2], a[t][I][4 * q + 3]};
#pragma unroll
                for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * q + li][4 * ks + lk], ap[I][ks], acc, 0, 0, 0);
                a[t][I][4 * q] = acc[0]; a[t][I][4 * q + 1] = acc[1]; a[t][I][4 * q + 2] = acc[2]; a[t][I][4 * q + 3] = acc[3];
              }
            }
          }
        }
      }
      CHOL_STAMP(2);                                             // layout change + last update
      // ---- the diagonal tile of this column: factor + inverse (first group only).  Nothing of the rows is kept in registers
      // across the factor: T' waits in the scratch tiles, in the layout it is read back in.
      if (g0 == 0) {
        if (w == 0) {
#pragma unroll
          for (int I = 0; I < 2; I++)
#pragma unroll
            for (int J = 0; J < 2; J++)
#pragma unroll
              for (int rg = 0; rg < 4; rg++) {
                const int r = 16 * I + lk + 4 * rg, cc = 16 * J + li;
                s_L[r][cc] = (cc <= r) ? T[0][I][J][rg] : 0.0;
              }
        }
#pragma unroll
        for (int t = 0; t < CW_RPW; t++) {
          double (*s_Sw)[NB + 1] = (double (*)[NB + 1])(s_dyn + (CW_RPW == 1 ? (w == 0 ? 3 + NSCA : 1 + w) : 2 + CW_RPW * w + t) * CW_TILE);
          if (valid[t] && !is_diag[t]) {
#pragma unroll
            for (int I = 0; I < 2; I++)
#pragma unroll
              for (int ks = 0; ks < 8; ks++) s_Sw[16 * I + li][4 * ks + lk] = a[t][I][ks];
          }
        }
        __syncthreads();
#ifndef CW_EXP_NOFACTOR
        {                                                        // all four waves: two entry-column blocks of eight each ... (diag_factor_invert_nw)
          const int fail = diag_factor_invert_nw<CW_NW>(s_L, s_X, &s_T[0][0], s_M, s_R, &s_col, NB * c, w);
          if (fail && lane == 0) s_fail = 1;
        }
#else
        for (int i = tid; i < NB * NB; i += CW_TPB) s_X[i / NB][i % NB] = (i / NB == i % NB) ? 1.0 : 0.0;
#endif
        __syncthreads();
        if (s_fail) { if (tid == 0) st->chol_fail = 1; return; }
        double* Di = D.Dinv + (size_t)c * NB * NB;
        for (int i = tid; i < NB * NB; i += CW_TPB) Di[i] = s_X[i / NB][i % NB];
#pragma unroll
        for (int t = 0; t < CW_RPW; t++) {
          double (*s_Sw)[NB + 1] = (double (*)[NB + 1])(s_dyn + (CW_RPW == 1 ? (w == 0 ? 3 + NSCA : 1 + w) : 2 + CW_RPW * w + t) * CW_TILE);
          const bool back = valid[t] && !is_diag[t];              // (assigned on every path: nothing is live across the factor)
#pragma unroll
          for (int I = 0; I < 2; I++)
#pragma unroll
            for (int ks = 0; ks < 8; ks++) a[t][I][ks] = back ? s_Sw[16 * I + li][4 * ks + lk] : 0.0;
        }
      }
      CHOL_STAMP(3);                                             // factor + inverse (first group)
      // ---- L(i, c) = T' X_c^T
#pragma unroll
      for (int t = 0; t < CW_RPW; t++) {
        if (!(valid[t] && !is_diag[t])) continue;
        const size_t rb = (size_t)my[t] * NB;
#pragma unroll
        for (int I = 0; I < 2; I++) {
          if (is_rhs[t] && I == 1) break;                        // (one row)
          double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < 8; ks++) {
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][I][ks], s_X[li][4 * ks + lk], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][I][ks], s_X[16 + li][4 * ks + lk], acc1, 0, 0, 0);
          }
          if (is_rhs[t]) {
            if (lk == 0) { zrow[cb + li] = acc0[0]; zrow[cb + 16 + li] = acc1[0]; }
          } else {
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
              const size_t orow = rb + 16 * I + lk + 4 * rg;
              S[orow * np + cb + li] = acc0[rg];
              S[orow * np + cb + 16 + li] = acc1[rg];
            }
          }
        }
      }
      __syncthreads();                                           // (the LDS buffers and s_z are free for the next group; this group's L tiles are visible)
      CHOL_STAMP(4);                                             // L = T' X^T, stores, barrier
    }
  }
}

// ---- persistent look-ahead Cholesky: ONE launch for the whole factorisation of a reduced system <= 1024 -------------------
// k_chol_la is one launch per 32-column step, and a step's kernel spends 2.5 of its 10.8 us waiting for its first loads and
// ~1 us outside the kernel (profiles/r02_chol_phase_prof_fused.json): the chain of 19 (C4) steps is launch- and
// load-latency on top of the 5.1 us diagonal factor.  Here the steps are iterations of a loop inside ONE kernel and the
// dependencies between workgroups are flags in global memory (tools/ubench/flag_hop.hip: a flag + 8 KB hand-off between two
// workgroups costs 1.1 - 1.4 us with agent-scope (sc1) data accesses, 2.7 - 3.6 us with __threadfence on both sides, so every
// access to data another workgroup wrote or will read is an agent-scope relaxed atomic and no fence is used):
//   workgroup 0, the CHAIN: all diagonal blocks and the sub-diagonal tile of every step.  Per step k: wave 0 factors and
//     inverts D_k; meanwhile waves 1..3 wait for row k+1 to be final and stage its three tiles; then M_k = X_k P_k,
//     L(k+1,k) = A(k+1,k) X_k^T - L(k+1,k-1) M_k^T, D_(k+1) = A(k+1,k+1) - L(k+1,k) L(k+1,k)^T in LDS - the chain never waits
//     for a kernel boundary or for its own stores - and X_k, M_k, L(k+1,k) are published (flag XREADY = k + 1);
//   ROW i (2 <= i < nb), its PRODUCER: for j = 0 .. i - 2: waits for X_j / M_j, L(i,j) = A(i,j) X_j^T - L(i,j-1) M_j^T, flag
//     LREADY[i] = j + 1; in its last step also the row's diagonal tile, flag FINAL[i];
//   ROW i, its ceil((i-1)/8) CONSUMERS: update j of their tiles (i, c), c = j + 2 .. i, with L(i,j) and L(c,j) of the rows above:
//     all flags of the step, then all loads of the step, then the MFMAs; flag PROG[i][share] = j + 1;
//   the last workgroup, the augmented rhs ROW: the same with one row, to the last block (forward substitution).
// The ARITHMETIC is k_chol_la's, operation for operation (tile (i,c) receives the updates 0 .. c-2 one by one as cpre - acc of
// eight MFMA k-steps, the last one algebraically through M; the rhs row's updates are the same sequential mul / add), so the
// results are bit-identical to the launch-per-step kernels (tests/test_gpu_ba.py::test_persistent_cholesky_is_bit_identical)
// and batched solves (k_chol_la<4>, throughput-bound) stay bit-identical to single calls.
// Residency: rows and consumers wait for workgroups with a smaller blockIdx.x, but the CHAIN (blockIdx.x 0) waits for
// FINAL[k + 1] of rows with LARGER indices - progress needs the chain and the rows it waits for to be co-resident.  The host
// therefore accounts the persistent launches of this process in workgroup slots (PersistLease) and falls back to the step
// kernels when a solve does not get its slots; kernels of OTHER streams / processes can still delay a row's dispatch, which is
// what the time bound of cp_wait is for: a wait that runs out ends the solve with termination 7 / ORBHIP_ETIMEOUT (never as a
// rejected LM step), a failed pivot raises FAIL = 1; either ends every other wait at once.
#define CP_XREADY 0
#define CP_FAIL 1
#define CP_LREADY 2
#define CP_FINAL 40
#define CP_PROG 80                 // [CP_PROG + 4 * row + share]: steps this share of the row has completed
#define CP_NFLAGS 256
#define CP_CH 8                    // tiles a row workgroup updates per step (their operands wait in registers together)
#define CP_SHARES 16               // consumer workgroups a row can have (k_chol_persist's PROG flags per row): envelopes up to 128 tiles
#define CP_SPIN_CAP (1 << 21)      /* polls of the waves of ONE workgroup waiting for each other (LDS counters): never long */
#define CP_LDS_DOUBLES ((1 + CP_CH) * NB * (NB + 1))      /* a consumer: L(i,j) + CP_CH operand tiles; the chain: 6 tiles + the factor's column buffer */
// (round 6: through address-space-1 pointers.  On the generic pointers of the BaDev struct these were FLAT instructions, which count as
// LDS traffic too: every `s_waitcnt lgkmcnt(0)` of a workgroup that lives on LDS round trips also waited for its global hand-offs.)
typedef double __attribute__((address_space(1))) * gdp_t;
typedef int __attribute__((address_space(1))) * gip_t;
__device__ __forceinline__ double ld_sc1(const double* p) { return __hip_atomic_load((gdp_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(double* p, double v) { __hip_atomic_store((gdp_t)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// Every wait is bounded - by TIME (s_memrealtime, 100 MHz), not by a spin count: the workgroup waited for may simply not be
// resident yet when another stream's kernels hold the CUs.  Five seconds is far beyond any such delay and still ends a genuine
// hang.  A wait that runs out of time is NOT a failed pivot: CP_FAIL takes the value 2 (a failed pivot: 1; either ends every
// other wait at once), BaState::chol_fail becomes 2, k_ba_iter_end ends the solve with termination 7 and the entry point
// returns ORBHIP_ETIMEOUT with the last accepted iterate - the LM radius is not touched (ADVICE r3, VERDICT r3 weak #6).
// g_cp_wait_ticks: the limit in 10-ns ticks; ba_set_wait_limit_ms() sets it (a deployment's deadline; tests shrink it to force the timeout path).
__device__ unsigned long long g_cp_wait_ticks = 500000000ull;
__device__ __forceinline__ void cp_timeout(int* flags) { __hip_atomic_fetch_max(flags + CP_FAIL, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool cp_wait(int* flags, int which, int v) {
  if (__hip_atomic_load((gip_t)(flags + which), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) { HANDOFF_ACQUIRE(); return true; }
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long limit = g_cp_wait_ticks;
  for (unsigned it = 0;; it++) {
    if (__hip_atomic_load((gip_t)(flags + which), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= v) { HANDOFF_ACQUIRE(); return true; }
    if ((it & 7) == 7 && __hip_atomic_load((gip_t)(flags + CP_FAIL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
    if ((it & 63) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > limit) { cp_timeout(flags); return false; }
    __builtin_amdgcn_s_sleep(1);
  }
}
__device__ __forceinline__ void cp_set(int* flags, int which, int v) { __hip_atomic_store((gip_t)(flags + which), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a workgroup gives up (its own failed pivot, or a wait that returned false): the reason is 1 unless somebody's wait timed out
__device__ __forceinline__ void cp_die(BaState* st, int* flags) {
  const int seen = __hip_atomic_fetch_max(flags + CP_FAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(&st->chol_fail, seen > 1 ? seen : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// consumers of block row i of the persistent look-ahead factorisation: the tiles (i, c), c = f + 2 .. i, behind the row's first column f
// (tile_first), CP_CH per workgroup and step.  Host (workgroup count) and device (workgroup -> role) use this one function.
__host__ __device__ __forceinline__ int cp_row_consumers(int i, int f) {
  const int cnt = i - (f < i ? f : i) - 1;
  return cnt > 0 ? (cnt + CP_CH - 1) / CP_CH : 0;
}

__global__ __launch_bounds__(256) void k_chol_persist(const BaDev* __restrict__ Dv) {
  const BaDev D = Dv[blockIdx.y];
  if (!D.chol_la) return;
  BaState* st = D.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.valid || F.chol_fail) return;
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int np = D.npad, nb = np / NB, tid = threadIdx.x, bx = (int)blockIdx.x;
  const int w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int ti = w >> 1, tj = w & 1;
  double* S = D.S;
  double* Dinv = D.Dinv;
  int* flags = D.cflags;
  // flag layout by the system's own block-row count (round 5: systems of more than 32 block rows come here when their skyline is narrow)
  const int F_LREADY = 2, F_FINAL = 2 + (nb + 2), F_PROG = 2 + 2 * (nb + 2);
  const int* __restrict__ tf = D.tile_first;
  if (bx == 0) {
    // ------------------------------------------------------------------------------------------------ the chain
    double (*s_L)[NB + 1] = (double (*)[NB + 1])s_dyn;                                  // D_k
    double (*s_X)[NB + 1] = (double (*)[NB + 1])(s_dyn + NB * (NB + 1));                // X_k = L_kk^-1
    double (*s_P)[NB + 1] = (double (*)[NB + 1])(s_dyn + 2 * NB * (NB + 1));            // P_k = L(k, k-1); after the L phase L(k+1, k)
    double (*s_A1)[NB + 1] = (double (*)[NB + 1])(s_dyn + 3 * NB * (NB + 1));           // A(k+1, k), updates 0 .. k-2 applied
    double (*s_Lp)[NB + 1] = (double (*)[NB + 1])(s_dyn + 4 * NB * (NB + 1));           // L(k+1, k-1)
    double* s_share = s_dyn + 5 * NB * (NB + 1);                                        // wave 1 -> wave 0: the updated rows 0..15 of A(k+1, k) [lane][8]
    double (*s_T)[64] = (double (*)[64])(s_dyn + 6 * NB * (NB + 1));                    // 16-byte aligned: 6 * 32 * 33 * 8 bytes
    __shared__ int s_fail, s_arrive, s_arrive2, s_grp;
#pragma unroll
    for (int u = 0; u < 4; u++) { const int i = tid + 256 * u, r = i / NB, c = i % NB; s_L[r][c] = (c <= r) ? S[(size_t)r * np + c] : 0.0; }
    if (tid == 0) { s_fail = 0; s_arrive = 0; s_arrive2 = 0; s_grp = 0; }
    // waves 1..3 own the lower 16x16 tiles of the NEXT diagonal block: (0,0), (1,0), (1,1)
    const int di = (w == 1) ? 0 : 1, dj = (w == 3) ? 1 : 0;
    const int ai = (w <= 1) ? 0 : 1;                            // the 16 rows of A(k+1, k) this wave multiplies: waves 0, 1 the upper, 2, 3 the lower
    int n_grp = 0;
    __syncthreads();
    for (int k = 0; k < nb; k++) {
      const bool upd = k > 0, next = k + 1 < nb;
      CHOL_PROF_BEGIN(k);
      double c2[4] = {0.0, 0.0, 0.0, 0.0};
      double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (tid < 64) {
        const int fail = diag_factor_invert_nw<1>(s_L, s_X, &s_T[0][0], nullptr, nullptr, nullptr, 0, 0);
        if (fail && tid == 0) s_fail = 1;
        CHOL_STAMP(0);                                          // factor + inverse
      } else if (next) {
        // stage row k + 1: its tile in column block k (updates 0 .. k-2 applied), L(k+1, k-1), and this wave's entries of its
        // diagonal tile (updates 0 .. k-1 applied); then the tile's last update, A <- A - L(k+1, k-1) P_k^T, beside the factor
        bool ok = true;
        if (upd) ok = cp_wait(flags, F_FINAL + k + 1, 1);
        if (!ok) s_fail = 2;
        const size_t rb = (size_t)(k + 1) * NB;
        {
          // (all twelve loads of a lane are requested before the first LDS store: the load -> store loop it used to be cost the
          // staging waves six dependent global round trips per step, most of the chain's "stall")
          double ta[6], tl[6];
#pragma unroll
          for (int u = 0; u < 6; u++) {
            const int i = tid - 64 + 192 * u, r = i / NB, c = i % NB;
            ta[u] = i < NB * NB ? ld_sc1(&S[(rb + r) * np + (size_t)k * NB + c]) : 0.0;
            tl[u] = (upd && i < NB * NB) ? ld_sc1(&S[(rb + r) * np + (size_t)(k - 1) * NB + c]) : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 6; u++) {
            const int i = tid - 64 + 192 * u, r = i / NB, c = i % NB;
            if (i < NB * NB) { s_A1[r][c] = ta[u]; s_Lp[r][c] = tl[u]; }
          }
        }
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int r = 16 * di + (lane >> 4) + 4 * rg, c = 16 * dj + (lane & 15);
          c2[rg] = (c <= r) ? ld_sc1(&S[(rb + r) * np + rb + c]) : 0.0;
        }
        // the three staging waves meet (wave 0 is in the factor: no __syncthreads here)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        n_grp += 3;
        if (lane == 0) __hip_atomic_fetch_add(&s_grp, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (int it = 0; it < CP_SPIN_CAP && __hip_atomic_load(&s_grp, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < n_grp; it++) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
        for (int ks = 0; ks < 8; ks++) a[ks] = s_A1[16 * ai + li][4 * ks + lk];
        if (upd) {
#pragma unroll
          for (int t = 0; t < 2; t++) {                         // (k_chol_la's apply_prev: the registers are rows of the C tiles of A^T)
            double4_t acc = {a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]};
#pragma unroll
            for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * t + li][4 * ks + lk], -s_Lp[16 * ai + li][4 * ks + lk], acc, 0, 0, 0);
            a[4 * t] = acc[0]; a[4 * t + 1] = acc[1]; a[4 * t + 2] = acc[2]; a[4 * t + 3] = acc[3];
          }
        }
        if (w == 1) {
#pragma unroll
          for (int ks = 0; ks < 8; ks++) s_share[lane * 8 + ks] = a[ks];
        }
      }
      __syncthreads();
      CHOL_STAMP(1);                                            // barrier: what the staging waves are late by
      if (s_fail) { if (tid == 0) cp_die(st, flags); return; }
      {
        double* Di = Dinv + (size_t)k * NB * NB;
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = tid + 256 * u; st_sc1(&Di[i], s_X[i / NB][i % NB]); }
      }
      CHOL_STAMP(2);                                            // X stores issued
      if (next) {
        if (w == 0) {
#pragma unroll
          for (int ks = 0; ks < 8; ks++) a[ks] = s_share[lane * 8 + ks];
        }
        // L(k+1, k) = A' X^T on the matrix cores: the new P
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], s_X[16 * tj + li][4 * ks + lk], acc, 0, 0, 0);
        const size_t rb = (size_t)(k + 1) * NB;
#pragma unroll
        for (int rg = 0; rg < 4; rg++) s_P[16 * ti + (lane >> 4) + 4 * rg][16 * tj + (lane & 15)] = acc[rg];
        // X_k has left (its stores were issued before the MFMAs above): the last wave to see that publishes it - the row
        // producers start on step k a microsecond before the chain is through with it
        HANDOFF_DRAIN();
        if (lane == 0 && __hip_atomic_fetch_add(&s_arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 4 * k + 3) cp_set(flags, CP_XREADY, k + 1);
#pragma unroll
        for (int rg = 0; rg < 4; rg++) st_sc1(&S[(rb + 16 * ti + (lane >> 4) + 4 * rg) * np + (size_t)k * NB + 16 * tj + (lane & 15)], acc[rg]);
        // (round 6: a barrier for the LDS only - __syncthreads() also waits for the stores just issued, ~0.4 us on every step's chain;
        // they drain beside the update below and are waited for where they are published, before LREADY)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        CHOL_STAMP(3);                                          // L(k+1, k)
        if (w >= 1) {                                           // D_(k+1) = A(k+1,k+1) - P P^T on the lower tiles
          double4_t a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < 8; ks++) a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * di + li][4 * ks + lk], s_P[16 * dj + li][4 * ks + lk], a2, 0, 0, 0);
#pragma unroll
          for (int rg = 0; rg < 4; rg++) {
            const int r = 16 * di + (lane >> 4) + 4 * rg, c = 16 * dj + (lane & 15);
            if (c <= r) s_L[r][c] = c2[rg] - a2[rg];
          }
        }
        // L(k+1, k) has left: it is the P the row producers need for their step k + 1
        HANDOFF_DRAIN();
        if (lane == 0 && __hip_atomic_fetch_add(&s_arrive2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 4 * k + 3) cp_set(flags, F_LREADY + k + 1, k + 1);
      }
      CHOL_STAMP(4);                                            // D update
      if (!next) {                                              // the last step: X is published here
        HANDOFF_DRAIN();
        __syncthreads();
        if (tid == 0) cp_set(flags, CP_XREADY, k + 1);
      }
      __syncthreads();
      CHOL_STAMP(5);                                            // barrier
    }
    return;
  }
  // -------------------------------------------------------------------------------------------------- a row
  // workgroups behind the chain, row by row (i = 2 .. nb - 1, then the rhs row nb): one PRODUCER - L(i, j) for every step - and
  // W_i = ceil((i - 1) / CP_CH) CONSUMERS - share g applies update j to the tiles (i, c), c % W_i == g, at most CP_CH per step.
  // Two short pipelines instead of one long step: a row keeps up with the chain when each stage fits a chain step.
  // RING (round 5; D.persist_ring = R > 0: every row has at most one consumer workgroup, i.e. its envelope is <= CP_CH + 1 tiles wide).
  // A row's workgroups have work only while the chain is between the row's first column and the row itself, so in a narrow-band system
  // row i + R (R = widest envelope + 1) starts after row i has handed its diagonal tile over: producer slot r walks the rows 2 + r,
  // 2 + r + R, ... one after the other, consumer slot r likewise - 2 R + 3 workgroups whatever the size of the system (a 94-block-row
  // GlobalBA with a band of 3: 11, not 187).  What has to be CO-RESIDENT for the chain to progress shrinks with it: under another
  // stream's high-priority kernels (the Tracking thread) the 187 one-workgroup-per-CU launches starved into the wait limit.
  // The ring walks the PREFIX of rows whose envelopes are narrow (rows 2 .. D.persist_ring_rows - 1); the rows behind it - a map with a
  // loop closure: the last keyframes also see landmarks of the first ones, their envelopes start at column 0 - keep a producer and
  // their consumers each, as every row does without a ring.
  const int ring = D.persist_ring, ring_rows = ring > 0 ? D.persist_ring_rows : 2;
  int irow = -1, share = -1, W = 1;                             // share -1: the producer
  bool is_rhs = false, in_ring = false;
  if (ring > 0 && bx <= 2 * ring) {
    if (bx <= ring) { irow = 2 + (bx - 1); share = -1; }
    else { irow = 2 + (bx - ring - 1); share = 0; }
    in_ring = true;
    if (irow >= ring_rows) return;
  } else {
    int b = ring > 0 ? 2 * ring + 1 : 1;
    for (int i = ring_rows; i < nb && irow < 0; i++) {
      const int wi = cp_row_consumers(i, tf[i]);               // (SKYLINE: a row's own L(i, j) is zero before column tile_first[i] - only the tiles behind it are ever updated)
      if (bx < b + 1 + wi) { irow = i; share = bx - b - 1; W = max(wi, 1); }
      b += 1 + wi;
    }
    if (irow < 0) { if (bx == b || bx == b + 1) { irow = nb; is_rhs = true; share = bx - b - 1; } else return; }
  }
  __shared__ int s_dead;
  if (tid == 0) s_dead = 0;
  for (bool first_row = true;; first_row = false) {             // the rows of this workgroup (one unless ring)
  if (!first_row) { if (!in_ring) return; irow += ring; if (irow >= ring_rows) return; }
  const size_t r0 = is_rhs ? (size_t)np : (size_t)irow * NB;
  double (*s_Lc)[NB + 1] = (double (*)[NB + 1])s_dyn;           // L(i, j) of the current step
  double (*s_Lq)[NB + 1] = (double (*)[NB + 1])(s_dyn + NB * (NB + 1));      // L(i, j-1)
  __syncthreads();
  if (share < 0) {
    // ---- producer: L(i, j) = A(i, j) X_j^T - L(i, j-1) M_j^T; in its last step (j = i - 2) also the row's diagonal tile
    const int jend = is_rhs ? nb : irow - 1;
    // SKYLINE: L(i, j) = 0 for j < tile_first[i] - those steps do not exist (the zeros are in memory since the zero fill): the row
    // announces them at once, starts at jstart, and a row without any step only hands its diagonal tile to the chain
    const int jstart = is_rhs ? 0 : min(tf[irow], jend);
    if (tid == 0 && jstart > 0) cp_set(flags, F_LREADY + irow, jstart);
    if (jstart >= jend) { if (tid == 0) cp_set(flags, F_FINAL + irow, 1); continue; }
    const int arow = 16 * ti + li;                              // this lane's row of the A operand
    double (*s_A)[NB + 1] = (double (*)[NB + 1])(s_dyn + 2 * NB * (NB + 1));
    double (*s_Xj)[NB + 1] = (double (*)[NB + 1])(s_dyn + 3 * NB * (NB + 1));
    double (*s_Mj)[NB + 1] = (double (*)[NB + 1])(s_dyn + 4 * NB * (NB + 1));
    for (int j = jstart; j < jend; j++) {
      const bool upd = j > jstart, last = !is_rhs && j == jend - 1;       // (j == jstart: L(i, j-1) is zero, the tile has no pending update)
      // before X_j exists: the tile (i, j) with its last update, A' = A - L(i, j-1) P_j^T (P_j = L(j, j-1), the chain's tile of
      // the previous step); all its inputs are one chain step old
      bool ok = true;
      // (the consumers' steps start at jstart as well: a wait for a step before it would never end)
      if (j - 2 >= jstart) ok = cp_wait(flags, F_PROG + CP_SHARES * irow + (j % W), j - 1);          // tile (i, j) has its update j - 2
      if (ok && last && j - 1 >= jstart) ok = cp_wait(flags, F_PROG + CP_SHARES * irow + (irow % W), j);   // the diagonal tile has update j - 1
      if (ok && last && j - 1 >= jstart) ok = cp_wait(flags, F_PROG + CP_SHARES * irow + ((irow - 1) % W), j);   // ... and tile (i, i-1), which FINAL hands to the chain (another share's when W > 1: it finished a chain step ago, but only a flag says so)
      if (ok && upd) ok = cp_wait(flags, F_LREADY + j, j);                                 // P_j is published
      double va[4], vp[4], cd[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int idx = tid + 256 * u, r = idx / NB, c = idx % NB;
        va[u] = (ok && (is_rhs ? r == 0 : true)) ? ld_sc1(&S[(r0 + r) * np + (size_t)j * NB + c]) : 0.0;
        vp[u] = (ok && upd) ? ld_sc1(&S[((size_t)j * NB + r) * np + (size_t)(j - 1) * NB + c]) : 0.0;
      }
#pragma unroll
      for (int rg = 0; rg < 4; rg++) cd[rg] = (ok && last) ? ld_sc1(&S[(r0 + 16 * ti + (lane >> 4) + 4 * rg) * np + r0 + 16 * tj + (lane & 15)]) : 0.0;
#pragma unroll
      for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u, r = idx / NB, c = idx % NB; s_A[r][c] = va[u]; s_Mj[r][c] = vp[u]; }
      __syncthreads();
      double a[8], b[8];
#pragma unroll
      for (int ks = 0; ks < 8; ks++) a[ks] = s_A[arow][4 * ks + lk];
      if (upd) {
#pragma unroll
        for (int t = 0; t < 2; t++) {                           // (k_chol_la's apply_prev)
          double4_t acc = {a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]};
#pragma unroll
          for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_Mj[16 * t + li][4 * ks + lk], -s_Lq[arow][4 * ks + lk], acc, 0, 0, 0);
          a[4 * t] = acc[0]; a[4 * t + 1] = acc[1]; a[4 * t + 2] = acc[2]; a[4 * t + 3] = acc[3];
        }
      }
      // X_j: the only thing this step waits for on the chain
      if (ok) ok = cp_wait(flags, CP_XREADY, j + 1);
      double vx[4];
#pragma unroll
      for (int u = 0; u < 4; u++) vx[u] = ok ? ld_sc1(&Dinv[(size_t)j * NB * NB + tid + 256 * u]) : 0.0;
#pragma unroll
      for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; s_Xj[idx / NB][idx % NB] = vx[u]; }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 8; ks++) b[ks] = s_Xj[16 * tj + li][4 * ks + lk];
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[ks], acc, 0, 0, 0);
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int r = 16 * ti + (lane >> 4) + 4 * rg, c = 16 * tj + (lane & 15);
        s_Lc[r][c] = acc[rg];
        if (ok && (is_rhs ? r == 0 : true)) st_sc1(&S[(r0 + r) * np + (size_t)j * NB + c], acc[rg]);
      }
      if (!ok) s_dead = 1;
      if (last) {
        __syncthreads();
        double4_t u4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 8; ks++) u4 = __builtin_amdgcn_mfma_f64_16x16x4f64(s_Lc[16 * ti + li][4 * ks + lk], s_Lc[16 * tj + li][4 * ks + lk], u4, 0, 0, 0);
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const size_t row = r0 + 16 * ti + (lane >> 4) + 4 * rg, col = r0 + 16 * tj + (lane & 15);
          if (ok && col <= row) st_sc1(&S[row * np + col], cd[rg] - u4[rg]);
        }
      }
      HANDOFF_DRAIN();
      __syncthreads();
      if (s_dead) { if (tid == 0) cp_die(st, flags); return; }
      if (tid == 0) { cp_set(flags, F_LREADY + irow, j + 1); if (last) cp_set(flags, F_FINAL + irow, 1); }
      { double (*t)[NB + 1] = s_Lc; s_Lc = s_Lq; s_Lq = t; }
    }
    continue;                                                   // (the row is done; ring: the next one of this slot)
  }
  if (!is_rhs) {
    // ---- consumer: update j of this share's tiles (i, c), c = j + 2 .. i: C = C - L(i,j) L(c,j)^T, one 16x16 tile of every 32x32
    // tile per wave.  All flags of the step first (one lane per tile), then EVERY load of the step, then the matrix cores.
    for (int j = min(tf[irow], irow); j + 3 <= irow; j++) {                // (SKYLINE: the row's L(i, j) is zero before tile_first[i])
      const int c_first = j + 2 + ((share - (j + 2)) % W + W) % W;         // smallest c >= j + 2 with c % W == share
      bool live[CP_CH];                                                    // tile (i, c) gets update j only if L(c, j) is inside row c's envelope
#pragma unroll
      for (int t = 0; t < CP_CH; t++) { const int c = c_first + t * W; live[t] = c <= irow && tf[min(c, irow)] <= j; }
      {
        const int ct = lane < CP_CH ? c_first + lane * W : irow;            // lane CP_CH: this row's own L(i, j)
        const bool mine = lane <= CP_CH && ct <= irow && (lane == CP_CH || tf[min(ct, irow)] <= j);
        bool good = true;
        const unsigned long long t0w = __builtin_amdgcn_s_memrealtime();
        for (unsigned it = 0;; it++) {
          const bool ready = !mine || __hip_atomic_load(flags + F_LREADY + ct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= j + 1;
          if (__builtin_amdgcn_ballot_w64(!ready) == 0) break;
          if (((it & 7) == 7 && __hip_atomic_load(flags + CP_FAIL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ||
              ((it & 63) == 0 && __builtin_amdgcn_s_memrealtime() - t0w > g_cp_wait_ticks && (cp_timeout(flags), true))) { good = false; break; }
          __builtin_amdgcn_s_sleep(1);
        }
        HANDOFF_ACQUIRE();
        if (!good) s_dead = 1;
      }
      // operand tiles as whole rows into LDS (see the producer); this lane's C entries directly (64 contiguous bytes per row)
      double vl[4], vb[CP_CH][4], cpre[CP_CH][4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; vl[u] = ld_sc1(&S[(r0 + idx / NB) * np + (size_t)j * NB + idx % NB]); }
#pragma unroll
      for (int t = 0; t < CP_CH; t++) {
        const int c = c_first + t * W;
        const size_t cb = (size_t)c * NB;
#pragma unroll
        for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; vb[t][u] = live[t] ? ld_sc1(&S[(cb + idx / NB) * np + (size_t)j * NB + idx % NB]) : 0.0; }
#pragma unroll
        for (int rg = 0; rg < 4; rg++) cpre[t][rg] = live[t] ? ld_sc1(&S[(r0 + 16 * ti + (lane >> 4) + 4 * rg) * np + cb + 16 * tj + (lane & 15)]) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; s_Lc[idx / NB][idx % NB] = vl[u]; }
#pragma unroll
      for (int t = 0; t < CP_CH; t++) {
        double (*s_B)[NB + 1] = (double (*)[NB + 1])(s_dyn + (1 + t) * NB * (NB + 1));
#pragma unroll
        for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; s_B[idx / NB][idx % NB] = vb[t][u]; }
      }
      __syncthreads();
      double la[8];
#pragma unroll
      for (int ks = 0; ks < 8; ks++) la[ks] = s_Lc[16 * ti + li][4 * ks + lk];
#pragma unroll
      for (int t = 0; t < CP_CH; t++) {
        const int c = c_first + t * W;
        if (c > irow) break;
        if (!live[t]) continue;                                   // (C - 0: the tile keeps its bits)
        const size_t cb = (size_t)c * NB;
        const double (*s_B)[NB + 1] = (const double (*)[NB + 1])(s_dyn + (1 + t) * NB * (NB + 1));
        double4_t u4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 8; ks++) u4 = __builtin_amdgcn_mfma_f64_16x16x4f64(la[ks], s_B[16 * tj + li][4 * ks + lk], u4, 0, 0, 0);
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const size_t row = r0 + 16 * ti + (lane >> 4) + 4 * rg, col = cb + 16 * tj + (lane & 15);
          if (col <= row) st_sc1(&S[row * np + col], cpre[t][rg] - u4[rg]);
        }
      }
      HANDOFF_DRAIN();
      __syncthreads();
      if (s_dead) { if (tid == 0) cp_die(st, flags); return; }
      if (tid == 0) cp_set(flags, F_PROG + CP_SHARES * irow + share, j + 1);
    }
    continue;
  }
  // ---- the rhs row's consumer: z_c -= sum_m L(c, 32 j + m) z_(32 j + m) for the columns from block j + 2 on (sequential mul / add
  // per column, as k_chol_la's rhs role; the 32 loads of a column are in flight together)
  double* zrow = S + (size_t)np * np;
  double* s_z = &s_Lc[0][0];
  for (int j = 0; j + 2 < nb; j++) {
    bool ok = cp_wait(flags, F_LREADY + nb, j + 1);
    if (tid < NB) s_z[tid] = ok ? ld_sc1(&zrow[(size_t)j * NB + tid]) : 0.0;
    __syncthreads();
    for (int cc = (j + 2) * NB + tid; ok && cc < np; cc += 256) {
      if (tf[cc / NB] > j) continue;                              // (SKYLINE: L(cc, block j) is zero - z_cc minus an exact zero)
      if (!cp_wait(flags, F_LREADY + cc / NB, j + 1)) { ok = false; break; }
      const double* L = S + (size_t)cc * np + (size_t)j * NB;
      double lv[NB];
#pragma unroll
      for (int mm = 0; mm < NB; mm++) lv[mm] = ld_sc1(&L[mm]);
      const double z0 = ld_sc1(&zrow[cc]);
      double sum = 0.0;
#pragma unroll
      for (int mm = 0; mm < NB; mm++) sum += lv[mm] * s_z[mm];
      st_sc1(&zrow[cc], z0 - sum);
    }
    if (!ok) s_dead = 1;
    HANDOFF_DRAIN();
    __syncthreads();
    if (s_dead) { if (tid == 0) cp_die(st, flags); return; }
    if (tid == 0) cp_set(flags, F_PROG + CP_SHARES * nb, j + 1);
  }
  return;
  }                                                             // rows of this workgroup
}

// ---- the same for the LARGE reduced systems (two-level scheme, GlobalBA): ONE persistent launch per 128-column outer block --
// k_chol_la steps an outer block with one launch per 32-column step (panel + thin updates confined to the block + a share of
// the previous block's K = 128 update); here the <= 4 steps of a block are a loop inside one launch, with the roles of
// k_chol_persist reduced to what a block needs:
//   workgroup 0, the CHAIN (as above; the first step of a block has no pending update - everything older came with the K = 128
//     updates -, and the last one leaves the next diagonal block alone: that is the next launch's first load);
//   one workgroup per block row below (row jb0 + 2 .. nb - 1, then the rhs row): L(i, j) for the steps of this block, and the
//     thin updates of its tiles INSIDE the block (at most two per step), in the step kernels' order;
//   behind them the workgroups of the previous outer block's K = 128 update (role C of k_chol_la: every tile once).
// Flags carry ABSOLUTE step numbers and are never reset between the launches of a factorisation.  Arithmetic = the step
// kernels' operation for operation: batched calls (>= 4 problems, k_chol_la) stay bit-identical to single ones.
// chol_syrk_body's tile part with the next K stage's loads issued BEFORE the matrix-core loop of the current one: the persistent
// kernels hold one workgroup per CU (the chain role's registers), so no other workgroup hides a stage's load latency.  Same
// operations in the same order.
__device__ __forceinline__ void chol_syrk_tile_pf(const BaDev& D, int ti, int tj, int kcol, int K, int lo, double (*s_A)[NB + 1], double (*s_B)[NB + 1]) {
  const int np = D.npad, tid = threadIdx.x;
  if (kcol + K > np) return;
  double* S = D.S;
  const int r0 = lo + ti * 64, c0 = lo + tj * 64;
  if (r0 + 63 < c0 || r0 >= np || c0 >= np) return;
  const int w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int qr = (w >> 1) * 32, qc = (w & 1) * 32;
  const bool qskip = (r0 + qr + 31 < c0 + qc);
  double4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double va[8], vb[8], cpre[2][2][4];
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int i = tid + 256 * u, r = i / NB, c = i % NB;
    va[u] = (r0 + r < np) ? S[(size_t)(r0 + r) * np + kcol + c] : 0.0;
    vb[u] = (c0 + r < np) ? S[(size_t)(c0 + r) * np + kcol + c] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int row = r0 + qr + 16 * i + (lane >> 4) + 4 * rg;
        const int col = c0 + qc + 16 * j + (lane & 15);
        cpre[i][j][rg] = (!qskip && row < np && col < np && col <= row) ? S[(size_t)row * np + col] : 0.0;
      }
  for (int k0 = 0; k0 < K; k0 += NB) {
#pragma unroll
    for (int u = 0; u < 8; u++) { const int i = tid + 256 * u; s_A[i / NB][i % NB] = va[u]; s_B[i / NB][i % NB] = vb[u]; }
    __syncthreads();
    if (k0 + NB < K) {
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = tid + 256 * u, r = i / NB, c = i % NB;
        va[u] = (r0 + r < np) ? S[(size_t)(r0 + r) * np + kcol + k0 + NB + c] : 0.0;
        vb[u] = (c0 + r < np) ? S[(size_t)(c0 + r) * np + kcol + k0 + NB + c] : 0.0;
      }
    }
    if (!qskip) {
#pragma unroll
      for (int kk = 0; kk < NB; kk += 4) {
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; i++) a[i] = s_A[qr + 16 * i + li][kk + lk];
#pragma unroll
        for (int j = 0; j < 2; j++) b[j] = s_B[qc + 16 * j + li][kk + lk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (qskip) return;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int row = r0 + qr + 16 * i + (lane >> 4) + 4 * rg;
        const int col = c0 + qc + 16 * j + (lane & 15);
        if (row < np && col < np && col <= row) S[(size_t)row * np + col] = cpre[i][j][rg] - acc[i][j][rg];
      }
}
// ... and TWO vertically adjacent tiles (128 x 64) per item: the column operand of a K stage is loaded once for both, and the
// fixed cost of an item (first loads, C tile, store) is spread over twice the matrix-core work.
// (SC1: the operands and the C tiles were written / will be read by other workgroups of the SAME launch - agent-scope accesses.
// Plain cached loads behind an agent-scope acquire fence were measured too: no faster)
template <bool SC1>
__device__ __forceinline__ void chol_syrk_tile2_pf(const BaDev& D, int ti2, int tj, int kcol, int K, int lo, double* s_raw) {
  auto ldg = [](const double* q) -> double { if constexpr (SC1) return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else return *q; };
  const int np = D.npad, tid = threadIdx.x;
  if (kcol + K > np) return;
  double* S = D.S;
  const int r0 = lo + ti2 * 128, c0 = lo + tj * 64;
  if (r0 + 127 < c0 || r0 >= np || c0 >= np) return;
  double (*s_A0)[NB + 1] = (double (*)[NB + 1])s_raw;
  double (*s_B)[NB + 1] = (double (*)[NB + 1])(s_raw + 64 * (NB + 1));
  double (*s_A1)[NB + 1] = (double (*)[NB + 1])(s_raw + 128 * (NB + 1));
  const int w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int qr = (w >> 1) * 32, qc = (w & 1) * 32;
  const bool live1 = r0 + 64 < np;                              // the lower tile exists
  const bool skip0 = (r0 + qr + 31 < c0 + qc), skip1 = !live1 || (r0 + 64 + qr + 31 < c0 + qc);
  double4_t acc[2][2][2];
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[h][i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double va0[8], va1[8], vb[8], cpre[2][2][2][4];
  auto load_stage = [&](int kc) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = tid + 256 * u, r = i / NB, c = i % NB;
      va0[u] = (r0 + r < np) ? ldg(&S[(size_t)(r0 + r) * np + kc + c]) : 0.0;
      va1[u] = (r0 + 64 + r < np) ? ldg(&S[(size_t)(r0 + 64 + r) * np + kc + c]) : 0.0;
      vb[u] = (c0 + r < np) ? ldg(&S[(size_t)(c0 + r) * np + kc + c]) : 0.0;
    }
  };
  load_stage(kcol);
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int row = r0 + 64 * h + qr + 16 * i + (lane >> 4) + 4 * rg;
          const int col = c0 + qc + 16 * j + (lane & 15);
          cpre[h][i][j][rg] = (!(h ? skip1 : skip0) && row < np && col < np && col <= row) ? ldg(&S[(size_t)row * np + col]) : 0.0;
        }
  for (int k0 = 0; k0 < K; k0 += NB) {
#pragma unroll
    for (int u = 0; u < 8; u++) { const int i = tid + 256 * u; s_A0[i / NB][i % NB] = va0[u]; s_A1[i / NB][i % NB] = va1[u]; s_B[i / NB][i % NB] = vb[u]; }
    __syncthreads();
    if (k0 + NB < K) load_stage(kcol + k0 + NB);
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) {
      double b[2];
#pragma unroll
      for (int j = 0; j < 2; j++) b[j] = s_B[qc + 16 * j + li][kk + lk];
      if (!skip0) {
        double a[2];
#pragma unroll
        for (int i = 0; i < 2; i++) a[i] = s_A0[qr + 16 * i + li][kk + lk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[0][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[0][i][j], 0, 0, 0);
      }
      if (!skip1) {
        double a[2];
#pragma unroll
        for (int i = 0; i < 2; i++) a[i] = s_A1[qr + 16 * i + li][kk + lk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[1][i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[1][i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {
    if (h ? skip1 : skip0) continue;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int row = r0 + 64 * h + qr + 16 * i + (lane >> 4) + 4 * rg;
          const int col = c0 + qc + 16 * j + (lane & 15);
          if (row < np && col < np && col <= row) { if constexpr (SC1) __hip_atomic_store(&S[(size_t)row * np + col], cpre[h][i][j][rg] - acc[h][i][j][rg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else S[(size_t)row * np + col] = cpre[h][i][j][rg] - acc[h][i][j][rg]; }
        }
  }
}
#define BP_LREADY 2
struct BlkGeo { int jb0, ns, base, kend, nend, tcn, n_tiles_n, n_rhs_n, n_tiles_c, blk; };     // (blocks of NB; host values = the largest problem of the launch)
// One 64 x 64 tile of the NEXT outer block's columns: the previous outer block's K = 128 update of it (role C's share, if any),
// then THIS block's, stage by stage as its panels are published - two chol_syrk_body passes operation for operation (the
// intermediate tile stays in registers), so that the next launch's chain finds its columns complete when this one ends.
// While the panels of a stage are not published yet (all but the last stage: that one is the block's critical path) the workgroup
// takes tiles of the previous block's far update from the launch's queue (steal() processes one and returns false when none is left).
template <class Steal>
__device__ __forceinline__ void chol_tile_next(const BaDev& D, int* flags, int r0, int c0, int c_hi, bool has_prev, int kcol_prev, int k_prev, int jb0, int ns,
                                               double (*s_A)[NB + 1], double (*s_B)[NB + 1], Steal steal) {
  const int np = D.npad, nb = np / NB, tid = threadIdx.x;
  if (r0 + 63 < c0 || r0 >= np || c0 >= c_hi) return;
  double* S = D.S;
  const int w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int qr = (w >> 1) * 32, qc = (w & 1) * 32;
  const bool qskip = (r0 + qr + 31 < c0 + qc);
  double cpre[2][2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int row = r0 + qr + 16 * i + (lane >> 4) + 4 * rg;
        const int col = c0 + qc + 16 * j + (lane & 15);
        cpre[i][j][rg] = (!qskip && row < np && col < c_hi && col <= row) ? S[(size_t)row * np + col] : 0.0;
      }
  double4_t acc[2][2];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  };
  auto stage_mma = [&]() {
    if (qskip) return;
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) a[i] = s_A[qr + 16 * i + li][kk + lk];
#pragma unroll
      for (int j = 0; j < 2; j++) b[j] = s_B[qc + 16 * j + li][kk + lk];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };
  double va[8], vb[8];
  if (has_prev) {
    zero_acc();
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = tid + 256 * u, r = i / NB, c = i % NB;
      va[u] = (r0 + r < np) ? S[(size_t)(r0 + r) * np + kcol_prev + c] : 0.0;
      vb[u] = (c0 + r < c_hi) ? S[(size_t)(c0 + r) * np + kcol_prev + c] : 0.0;
    }
    for (int k0 = 0; k0 < k_prev; k0 += NB) {
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 8; u++) { const int i = tid + 256 * u; s_A[i / NB][i % NB] = va[u]; s_B[i / NB][i % NB] = vb[u]; }
      __syncthreads();
      if (k0 + NB < k_prev) {                                   // the next stage's loads fly during this stage's matrix-core loop
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int i = tid + 256 * u, r = i / NB, c = i % NB;
          va[u] = (r0 + r < np) ? S[(size_t)(r0 + r) * np + kcol_prev + k0 + NB + c] : 0.0;
          vb[u] = (c0 + r < c_hi) ? S[(size_t)(c0 + r) * np + kcol_prev + k0 + NB + c] : 0.0;
        }
      }
      stage_mma();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) cpre[i][j][rg] = cpre[i][j][rg] - acc[i][j][rg];
  }
  zero_acc();
  const int rb0 = r0 / NB, cb0 = c0 / NB;
  for (int q = 0; q < ns; q++) {
    const int need = jb0 + q + 1;                               // L(x, jb0 + q) is published
    while (q + 1 < ns) {
      bool up = __hip_atomic_load(flags + BP_LREADY + rb0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need &&
                __hip_atomic_load(flags + BP_LREADY + cb0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
      if (up && rb0 + 1 < nb) up = __hip_atomic_load(flags + BP_LREADY + rb0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
      if (up && cb0 + 1 < nb && (c0 + NB) < c_hi) up = __hip_atomic_load(flags + BP_LREADY + cb0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
      if (__syncthreads_and(up)) break;
      if (!steal()) break;                                      // (nothing left to take: wait below)
    }
    bool ok = cp_wait(flags, BP_LREADY + rb0, need) && cp_wait(flags, BP_LREADY + cb0, need);
    if (ok && rb0 + 1 < nb) ok = cp_wait(flags, BP_LREADY + rb0 + 1, need);
    if (ok && cb0 + 1 < nb && (c0 + NB) < c_hi) ok = cp_wait(flags, BP_LREADY + cb0 + 1, need);
    if (__syncthreads_count(!ok)) { if (tid == 0) cp_die(D.st, flags); return; }     // (failed pivot elsewhere, or a wait that ran out of time: recorded, nothing more to do)
    const size_t kc = (size_t)(jb0 + q) * NB;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = tid + 256 * u, r = i / NB, c = i % NB;
      va[u] = (r0 + r < np) ? ld_sc1(&S[(size_t)(r0 + r) * np + kc + c]) : 0.0;
      vb[u] = (c0 + r < c_hi) ? ld_sc1(&S[(size_t)(c0 + r) * np + kc + c]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) { const int i = tid + 256 * u; s_A[i / NB][i % NB] = va[u]; s_B[i / NB][i % NB] = vb[u]; }
    __syncthreads();
    stage_mma();
  }
  if (qskip) return;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int row = r0 + qr + 16 * i + (lane >> 4) + 4 * rg;
        const int col = c0 + qc + 16 * j + (lane & 15);
        if (row < np && col < c_hi && col <= row) S[(size_t)row * np + col] = cpre[i][j][rg] - acc[i][j][rg];
      }
}
// the augmented rhs row's entries of the next outer block's columns, the same two updates (sequential mul / add per column)
__device__ __forceinline__ void chol_rhs_next(const BaDev& D, int* flags, int c, int c_hi, bool has_prev, int kcol_prev, int k_prev, int jb0, int ns, double* s_z) {
  const int np = D.npad, nb = np / NB, tid = threadIdx.x;
  double* S = D.S;
  double* zrow = S + (size_t)np * np;
  const bool mine = c < c_hi;
  double zv = mine ? zrow[c] : 0.0;
  if (has_prev) {
    for (int i = tid; i < k_prev; i += 256) s_z[i] = zrow[kcol_prev + i];
    __syncthreads();
    if (mine) {
      const double* L = S + (size_t)c * np + kcol_prev;
      double sum = 0.0;
      for (int m = 0; m < k_prev; m++) sum += L[m] * s_z[m];
      zv -= sum;
    }
  }
  const int kend = jb0 + ns, K = ns * NB;
  bool ok = cp_wait(flags, BP_LREADY + nb, kend);               // the row's own entries of this block
  if (ok && mine) ok = cp_wait(flags, BP_LREADY + c / NB, kend);
  if (__syncthreads_count(!ok)) { if (tid == 0) cp_die(D.st, flags); return; }
  for (int i = tid; i < K; i += 256) s_z[i] = ld_sc1(&zrow[(size_t)jb0 * NB + i]);
  __syncthreads();
  if (mine) {
    const double* L = S + (size_t)c * np + (size_t)jb0 * NB;
    double sum = 0.0;
    for (int m = 0; m < K; m++) sum += ld_sc1(&L[m]) * s_z[m];
    zrow[c] = zv - sum;
  }
}
__global__ __launch_bounds__(256) void k_chol_persist_blk(const BaDev* __restrict__ Dv, BlkGeo geo, CholWide wd) {
  const int jb0 = geo.jb0, ns = geo.ns, rolec_base = geo.base;
  const BaDev D = Dv[blockIdx.y];
  if (D.chol_la) return;
  BaState* st = D.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.valid || F.chol_fail) return;
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int np = D.npad, nb = np / NB, tid = threadIdx.x, bx = (int)blockIdx.x;
  if (jb0 >= nb) return;
  const int kend = min(jb0 + ns, nb);                           // steps jb0 .. kend - 1; thin updates touch the column blocks < kend
  const int w = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int ti = w >> 1, tj = w & 1;
  double* S = D.S;
  double* Dinv = D.Dinv;
  int* flags = D.cflags;
  const int R = nb + 2;
  const int FIN = BP_LREADY + R;                                // FINAL flags behind the LREADY flags
  if (bx >= rolec_base) {
    // ---- the previous outer block's K = 128 update of everything right of this block (role C of k_chol_la)
    double (*s_A)[NB + 1] = (double (*)[NB + 1])s_dyn;
    double (*s_B)[NB + 1] = (double (*)[NB + 1])(s_dyn + 64 * (NB + 1));
    // ---- the pool: the owners of the next outer block's tiles, and whoever else fits on the device.  The rest of the previous
    // block's K = 128 update (the columns right of the next outer block; every tile once, any order) is a QUEUE all of them draw
    // from - the owners while their panels are not published yet, everybody until it is empty: with one workgroup per CU (the
    // chain role's registers) a workgroup that only spins is a CU that does nothing.
    const int wi = bx - rolec_base;
    const bool has_prev = wd.total > 0;
    const int c_hi_n = min(geo.nend * NB, np);
    const int tcr = wd.tiles_c - geo.tcn;
    const int n_items = has_prev ? (tcr > 0 ? geo.n_tiles_c : 0) + wd.nrhs : 0, n_tile_items = has_prev && tcr > 0 ? geo.n_tiles_c : 0;
    int* qctr = flags + BP_LREADY + 2 * R + geo.blk;              // this launch's queue head (zeroed with the flags; one per outer block, blk < nb)
    __shared__ int s_item;
    auto steal = [&]() -> bool {
      if (n_items <= 0) return false;
      __syncthreads();
      if (tid == 0) s_item = __hip_atomic_fetch_add(qctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const int it = s_item;
      if (it >= n_items) return false;
      if (it < n_tile_items) { const int ti_c = it / tcr, tj_c = geo.tcn + (it - ti_c * tcr); chol_syrk_tile2_pf<false>(D, ti_c, tj_c, wd.kcol, wd.K, wd.lo, s_dyn); }
      else chol_syrk_body(D, st, wd.total + (it - n_tile_items), wd.kcol, wd.K, wd.lo, wd.lo, INT_MAX, wd.tiles_c, wd.total, s_A, s_B, geo.n_tiles_n > 0 ? geo.nend * NB : 0);
      return true;
    };
    if (geo.kend == kend) {                                     // (else a smaller problem of the launch: this is its last block)
      if (wi < geo.n_tiles_n) {                                 // the next outer block's columns: the previous block's update, then this one's
        const int ti_n = wi / geo.tcn, tj_n = wi - ti_n * geo.tcn;
        chol_tile_next(D, flags, geo.kend * NB + 64 * ti_n, geo.kend * NB + 64 * tj_n, c_hi_n, has_prev, wd.kcol, wd.K, jb0, ns, s_A, s_B, steal);
      } else if (wi < geo.n_tiles_n + geo.n_rhs_n) {
        __syncthreads();
        chol_rhs_next(D, flags, geo.kend * NB + 256 * (wi - geo.n_tiles_n) + tid, c_hi_n, has_prev, wd.kcol, wd.K, jb0, ns, &s_A[0][0]);
      }
    }
    while (steal()) {}
    return;
  }
  if (bx == 0) {
    // ------------------------------------------------------------------------------------------------ the chain
    double (*s_L)[NB + 1] = (double (*)[NB + 1])s_dyn;
    double (*s_X)[NB + 1] = (double (*)[NB + 1])(s_dyn + NB * (NB + 1));
    double (*s_P)[NB + 1] = (double (*)[NB + 1])(s_dyn + 2 * NB * (NB + 1));
    double (*s_A1)[NB + 1] = (double (*)[NB + 1])(s_dyn + 3 * NB * (NB + 1));
    double (*s_Lp)[NB + 1] = (double (*)[NB + 1])(s_dyn + 4 * NB * (NB + 1));
    double* s_share = s_dyn + 5 * NB * (NB + 1);
    double (*s_T)[64] = (double (*)[64])(s_dyn + 6 * NB * (NB + 1));
    __shared__ int s_fail, s_arrive, s_arrive2, s_grp;
    {
      const size_t d0 = (size_t)jb0 * NB;
#pragma unroll
      for (int u = 0; u < 4; u++) { const int i = tid + 256 * u, r = i / NB, c = i % NB; s_L[r][c] = (c <= r) ? S[(d0 + r) * np + d0 + c] : 0.0; }
    }
    if (tid == 0) { s_fail = 0; s_arrive = 0; s_arrive2 = 0; s_grp = 0; }
    const int di = (w == 1) ? 0 : 1, dj = (w == 3) ? 1 : 0;
    const int ai = (w <= 1) ? 0 : 1;
    int n_grp = 0;
    __syncthreads();
    for (int k = jb0; k < kend; k++) {
      const bool upd = k > jb0, next = k + 1 < nb, nextD = next && k + 1 < kend;
      const int kr = k - jb0;
      CHOL_PROF_BEGIN(k);
      double c2[4] = {0.0, 0.0, 0.0, 0.0};
      double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (tid < 64) {
        const int fail = diag_factor_invert_nw<1>(s_L, s_X, &s_T[0][0], nullptr, nullptr, nullptr, 0, 0);
        if (fail && tid == 0) s_fail = 1;
        CHOL_STAMP(0);                                          // factor + inverse
      } else if (next) {
        // Row k + 1 is needed in two instalments: its tiles (k+1, k) and L(k+1, k-1) for the update beside the factor - final as
        // soon as the row has PUBLISHED L(k+1, k-1) (the thin updates of tile (k+1, k) belong to earlier steps) -, its diagonal
        // tile only behind the factor.  The row finishes that tile (its last thin update: a load, eight MFMAs, a store) 2 - 3 us
        // after the publication; waiting for everything at once put that on the chain (9.1 -> 7.9 us per step).
        bool ok = true;
        if (upd) ok = cp_wait(flags, BP_LREADY + k + 1, k);
        const size_t rb = (size_t)(k + 1) * NB;
        {
          // (all twelve loads of a lane are requested before the first LDS store: the load -> store loop it used to be cost the
          // staging waves six dependent global round trips per step, most of the chain's "stall")
          double ta[6], tl[6];
#pragma unroll
          for (int u = 0; u < 6; u++) {
            const int i = tid - 64 + 192 * u, r = i / NB, c = i % NB;
            ta[u] = i < NB * NB ? ld_sc1(&S[(rb + r) * np + (size_t)k * NB + c]) : 0.0;
            tl[u] = (upd && i < NB * NB) ? ld_sc1(&S[(rb + r) * np + (size_t)(k - 1) * NB + c]) : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 6; u++) {
            const int i = tid - 64 + 192 * u, r = i / NB, c = i % NB;
            if (i < NB * NB) { s_A1[r][c] = ta[u]; s_Lp[r][c] = tl[u]; }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        n_grp += 3;
        if (lane == 0) __hip_atomic_fetch_add(&s_grp, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (int it = 0; it < CP_SPIN_CAP && __hip_atomic_load(&s_grp, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < n_grp; it++) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
        for (int ks = 0; ks < 8; ks++) a[ks] = s_A1[16 * ai + li][4 * ks + lk];
        if (upd) {
#pragma unroll
          for (int t = 0; t < 2; t++) {
            double4_t acc = {a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]};
#pragma unroll
            for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * t + li][4 * ks + lk], -s_Lp[16 * ai + li][4 * ks + lk], acc, 0, 0, 0);
            a[4 * t] = acc[0]; a[4 * t + 1] = acc[1]; a[4 * t + 2] = acc[2]; a[4 * t + 3] = acc[3];
          }
        }
        if (w == 1) {
#pragma unroll
          for (int ks = 0; ks < 8; ks++) s_share[lane * 8 + ks] = a[ks];
        }
        if (nextD) {                                            // the diagonal tile of row k + 1, behind the row's last thin update
          if (upd && ok) ok = cp_wait(flags, FIN + k + 1, 1);
#pragma unroll
          for (int rg = 0; rg < 4; rg++) {
            const int r = 16 * di + (lane >> 4) + 4 * rg, c = 16 * dj + (lane & 15);
            c2[rg] = (c <= r) ? ld_sc1(&S[(rb + r) * np + rb + c]) : 0.0;
          }
        }
        if (!ok) s_fail = 2;
      }
      __syncthreads();
      CHOL_STAMP(1);                                            // barrier: what the staging waves are late by
      if (s_fail) { if (tid == 0) cp_die(st, flags); return; }
      {
        double* Di = Dinv + (size_t)k * NB * NB;
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = tid + 256 * u; st_sc1(&Di[i], s_X[i / NB][i % NB]); }
      }
      CHOL_STAMP(2);                                            // X stores issued
      if (next) {
        if (w == 0) {
#pragma unroll
          for (int ks = 0; ks < 8; ks++) a[ks] = s_share[lane * 8 + ks];
        }
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], s_X[16 * tj + li][4 * ks + lk], acc, 0, 0, 0);
        const size_t rb = (size_t)(k + 1) * NB;
#pragma unroll
        for (int rg = 0; rg < 4; rg++) s_P[16 * ti + (lane >> 4) + 4 * rg][16 * tj + (lane & 15)] = acc[rg];
        HANDOFF_DRAIN();
        if (lane == 0 && __hip_atomic_fetch_add(&s_arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 4 * kr + 3) cp_set(flags, CP_XREADY, k + 1);
#pragma unroll
        for (int rg = 0; rg < 4; rg++) st_sc1(&S[(rb + 16 * ti + (lane >> 4) + 4 * rg) * np + (size_t)k * NB + 16 * tj + (lane & 15)], acc[rg]);
        __syncthreads();
        CHOL_STAMP(3);                                          // L(k+1, k) + publication of X
        if (w >= 1 && nextD) {
          double4_t a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ks = 0; ks < 8; ks++) a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(s_P[16 * di + li][4 * ks + lk], s_P[16 * dj + li][4 * ks + lk], a2, 0, 0, 0);
#pragma unroll
          for (int rg = 0; rg < 4; rg++) {
            const int r = 16 * di + (lane >> 4) + 4 * rg, c = 16 * dj + (lane & 15);
            if (c <= r) s_L[r][c] = c2[rg] - a2[rg];
          }
        }
        HANDOFF_DRAIN();
        if (lane == 0 && __hip_atomic_fetch_add(&s_arrive2, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == 4 * kr + 3) cp_set(flags, BP_LREADY + k + 1, k + 1);
        CHOL_STAMP(4);                                          // D update + publication of L
      }
      if (!next) {
        HANDOFF_DRAIN();
        __syncthreads();
        if (tid == 0) cp_set(flags, CP_XREADY, k + 1);
      }
      __syncthreads();
      CHOL_STAMP(5);                                            // barrier
    }
    return;
  }
  // -------------------------------------------------------------------------------------------------- a row
  const int nrow = max(nb - (jb0 + 2), 0);
  int irow; bool is_rhs = false;
  if (bx <= nrow) irow = jb0 + 1 + bx;                          // bx 1 -> row jb0 + 2
  else if (bx == nrow + 1) { irow = nb; is_rhs = true; }
  else return;
  const size_t r0 = is_rhs ? (size_t)np : (size_t)irow * NB;
  double (*s_Lc)[NB + 1] = (double (*)[NB + 1])s_dyn;
  double (*s_Lq)[NB + 1] = (double (*)[NB + 1])(s_dyn + NB * (NB + 1));
  double (*s_A)[NB + 1] = (double (*)[NB + 1])(s_dyn + 2 * NB * (NB + 1));
  double (*s_Xj)[NB + 1] = (double (*)[NB + 1])(s_dyn + 3 * NB * (NB + 1));
  double (*s_Pj)[NB + 1] = (double (*)[NB + 1])(s_dyn + 4 * NB * (NB + 1));
  __shared__ int s_dead;
  if (tid == 0) s_dead = 0;
  __syncthreads();
  const int arow = 16 * ti + li;
  const int jend = is_rhs ? kend : min(kend, irow - 1);         // the producer's steps of this block: j <= i - 2 (the chain forms L(i, i-1))
  for (int j = jb0; j < jend; j++) {
    const bool upd = j > jb0;
    bool ok = true;
    if (upd) ok = cp_wait(flags, BP_LREADY + j, j);             // P_j = L(j, j-1) is published
    double va[4], vp[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int idx = tid + 256 * u, r = idx / NB, c = idx % NB;
      va[u] = (ok && (is_rhs ? r == 0 : true)) ? ld_sc1(&S[(r0 + r) * np + (size_t)j * NB + c]) : 0.0;
      vp[u] = (ok && upd) ? ld_sc1(&S[((size_t)j * NB + r) * np + (size_t)(j - 1) * NB + c]) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u, r = idx / NB, c = idx % NB; s_A[r][c] = va[u]; s_Pj[r][c] = vp[u]; }
    __syncthreads();
    double a[8], b[8];
#pragma unroll
    for (int ks = 0; ks < 8; ks++) a[ks] = s_A[arow][4 * ks + lk];
    if (upd) {
#pragma unroll
      for (int t = 0; t < 2; t++) {
        double4_t acc = {a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3]};
#pragma unroll
        for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_Pj[16 * t + li][4 * ks + lk], -s_Lq[arow][4 * ks + lk], acc, 0, 0, 0);
        a[4 * t] = acc[0]; a[4 * t + 1] = acc[1]; a[4 * t + 2] = acc[2]; a[4 * t + 3] = acc[3];
      }
    }
    if (ok) ok = cp_wait(flags, CP_XREADY, j + 1);
    double vx[4];
#pragma unroll
    for (int u = 0; u < 4; u++) vx[u] = ok ? ld_sc1(&Dinv[(size_t)j * NB * NB + tid + 256 * u]) : 0.0;
#pragma unroll
    for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; s_Xj[idx / NB][idx % NB] = vx[u]; }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ks++) b[ks] = s_Xj[16 * tj + li][4 * ks + lk];
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[ks], acc, 0, 0, 0);
#pragma unroll
    for (int rg = 0; rg < 4; rg++) {
      const int r = 16 * ti + (lane >> 4) + 4 * rg, c = 16 * tj + (lane & 15);
      s_Lc[r][c] = acc[rg];
      if (ok && (is_rhs ? r == 0 : true)) st_sc1(&S[(r0 + r) * np + (size_t)j * NB + c], acc[rg]);
    }
    if (!ok) s_dead = 1;
    HANDOFF_DRAIN();
    __syncthreads();
    if (s_dead) { if (tid == 0) cp_die(st, flags); return; }
    if (tid == 0) cp_set(flags, BP_LREADY + irow, j + 1);
    // update j of this row's tiles inside the block (k_chol_la's role B confined by c_cap): column blocks j + 2 .. kend - 1, not beyond the diagonal
    if (!is_rhs) {
      double la[8];
#pragma unroll
      for (int ks = 0; ks < 8; ks++) la[ks] = s_Lc[16 * ti + li][4 * ks + lk];
      for (int c = j + 2; c < kend && c <= irow; c++) {
        const size_t cb = (size_t)c * NB;
        bool okc = true;
        if (c < irow) okc = cp_wait(flags, BP_LREADY + c, j + 1);
        double vb[4], cpre[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; vb[u] = (okc && c < irow) ? ld_sc1(&S[(cb + idx / NB) * np + (size_t)j * NB + idx % NB]) : 0.0; }
#pragma unroll
        for (int rg = 0; rg < 4; rg++) cpre[rg] = okc ? ld_sc1(&S[(r0 + 16 * ti + (lane >> 4) + 4 * rg) * np + cb + 16 * tj + (lane & 15)]) : 0.0;
        __syncthreads();                                        // (s_Xj is free again: everybody has its X operands)
        if (c < irow) {
#pragma unroll
          for (int u = 0; u < 4; u++) { const int idx = tid + 256 * u; s_Xj[idx / NB][idx % NB] = vb[u]; }
        }
        __syncthreads();
        double4_t u4 = {0.0, 0.0, 0.0, 0.0};
        if (c < irow) {
#pragma unroll
          for (int ks = 0; ks < 8; ks++) u4 = __builtin_amdgcn_mfma_f64_16x16x4f64(la[ks], s_Xj[16 * tj + li][4 * ks + lk], u4, 0, 0, 0);
        } else {
#pragma unroll
          for (int ks = 0; ks < 8; ks++) u4 = __builtin_amdgcn_mfma_f64_16x16x4f64(la[ks], s_Lc[16 * tj + li][4 * ks + lk], u4, 0, 0, 0);
        }
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const size_t row = r0 + 16 * ti + (lane >> 4) + 4 * rg, col = cb + 16 * tj + (lane & 15);
          if (okc && col <= row) st_sc1(&S[row * np + col], cpre[rg] - u4[rg]);
        }
        if (!okc) s_dead = 1;
      }
    } else {
      double* zrow = S + (size_t)np * np;
      for (int cc = (j + 2) * NB + tid; cc < kend * NB; cc += 256) {
        if (!cp_wait(flags, BP_LREADY + cc / NB, j + 1)) { s_dead = 1; break; }
        const double* L = S + (size_t)cc * np + (size_t)j * NB;
        double lv[NB];
#pragma unroll
        for (int mm = 0; mm < NB; mm++) lv[mm] = ld_sc1(&L[mm]);
        const double z0 = ld_sc1(&zrow[cc]);
        double sum = 0.0;
#pragma unroll
        for (int mm = 0; mm < NB; mm++) sum += lv[mm] * s_Lc[0][mm];
        st_sc1(&zrow[cc], z0 - sum);
      }
    }
    HANDOFF_DRAIN();
    __syncthreads();
    if (s_dead) { if (tid == 0) cp_die(st, flags); return; }
    // the chain needs this row once it is the next one: L(i, i-2) and the row's tiles in the column blocks i - 1 and i are final
    if (tid == 0 && !is_rhs && j == irow - 2) cp_set(flags, FIN + irow, 1);
    { double (*t)[NB + 1] = s_Lc; s_Lc = s_Lq; s_Lq = t; }
  }
}

// (the one-launch two-level kernel k_chol_persist_2l - bit-identical, measured slower - lives in tools/experiments/chol_persist_2l.inc (outside the package; tools/build_experiments.sh adds -Itools):
// ORBHIP_EXPERIMENTS builds, ORBHIP_BA_PERSIST=2)
#ifdef ORBHIP_EXPERIMENTS
#include "experiments/chol_persist_2l.inc"
#endif

// backward substitution L^T x = z (z = augmented row, produced by the factorisation itself), in super-blocks
// of 256 rows processed from the bottom: k_chol_bsolve_diag solves one super-block with a single 1024-thread
// workgroup, then k_chol_bsolve_update subtracts its contribution from every earlier entry with many workgroups
// (fixed-order LDS reductions -> deterministic).
// Everything k_chol_bsolve_diag reads from the factor - the <= 8 stored L11^-1 blocks and the <= 28 off-diagonal 32x32
// blocks of the super-block - is independent of the running solution, so it is requested up front, one element of every
// block per thread (28 + 8 doubles in registers); the <= 8 sequential block steps then run on LDS and registers only
// (35 us -> see DESIGN.md; the first version re-read global memory twice per step).
#define SBLK 256
#define SB_NBLK (SBLK / NB)
#define BS_SKY_BAND 4                  /* skyline (tiles) up to which the backward substitution is ONE launch of one workgroup per problem (k_chol_bsolve_sky) */
// (bodies shared by the per-super-block kernels and by k_chol_bsolve_sky: the same loads, products and LDS sums in the same order)
__device__ __forceinline__ void bsolve_diag_body(const BaDev& D, const StFlags& F, const int kb, double* s_y, double* s_x, double (*s_p)[SBLK - NB], const bool flags_checked) {
  const int np = D.npad, tid = threadIdx.x;
  const int ke = min(kb + SBLK, np), first = (kb + SBLK >= np);
  const int nblk = (ke - kb) / NB;
  const int r = tid >> 5, c = tid & 31;
  const double* S = D.S;
  double di[SB_NBLK], sv[SB_NBLK * (SB_NBLK - 1) / 2];
#pragma unroll
  for (int bb = 0; bb < SB_NBLK; bb++)
    di[bb] = (bb < nblk) ? D.Dinv[((size_t)(kb / NB + bb) * NB + r) * NB + c] : 0.0;
#pragma unroll
  for (int bb = 1; bb < SB_NBLK; bb++)
#pragma unroll
    for (int cb = 0; cb < bb; cb++)
      sv[bb * (bb - 1) / 2 + cb] = (bb < nblk) ? S[(size_t)(kb + NB * bb + r) * np + kb + NB * cb + c] : 0.0;
  if (!flags_checked && (F.done || !F.valid || F.chol_fail)) return;
  const double* src = first ? (D.S + (size_t)np * np) : D.rhs;      // the first (bottom) super-block starts from z
  if (first) for (int i = tid; i < kb; i += 1024) D.rhs[i] = src[i];  // seed the running vector for the rows above
  if (tid < ke - kb) s_y[tid] = src[kb + tid];
  __syncthreads();
#pragma unroll
  for (int bb = SB_NBLK - 1; bb >= 0; bb--) {
    if (bb < nblk) {                                                // (uniform)
      // x = Linv^T y_b : x[c] = sum_r Linv[r][c] y[r]   (Linv is lower triangular: the r < c terms are exact zeros)
      s_p[r][c] = di[bb] * s_y[NB * bb + r];
      __syncthreads();
      if (tid < NB) {
        double sum = 0.0;
#pragma unroll
        for (int rr = 0; rr < NB; rr++) sum += s_p[rr][tid];
        s_x[tid] = sum;
        s_y[NB * bb + tid] = sum;
      }
      __syncthreads();
      if (bb > 0) {
        // rows of this super-block above block bb: y[cc] -= sum_r L[block bb row r][cc] x[r]
        const double xr = s_x[r];
#pragma unroll
        for (int cb = 0; cb < bb; cb++) s_p[r][NB * cb + c] = sv[bb * (bb - 1) / 2 + cb] * xr;
        __syncthreads();
        if (tid < NB * bb) {
          double sum = 0.0;
#pragma unroll
          for (int rr = 0; rr < NB; rr++) sum += s_p[rr][tid];
          s_y[tid] -= sum;
        }
        __syncthreads();
      }
    }
  }
  if (tid < ke - kb) D.rhs[kb + tid] = s_y[tid];
}
__global__ __launch_bounds__(1024) void k_chol_bsolve_diag(const BaDev* __restrict__ Dv, int kb) {
  const BaDev D = Dv[blockIdx.y];
  const StFlags F = ld_flags(D.st);
  __shared__ double s_y[SBLK], s_x[NB];
  __shared__ double s_p[NB][SBLK - NB];                             // partial products, [row of the block][column above the block]
  if (kb >= D.npad) return;                                         // batched launch: super-block beyond this problem
  bsolve_diag_body(D, F, kb, s_y, s_x, s_p, false);
}

// columns 64 bx .. 64 bx + 63 (< kb) of the running vector minus the contribution of the super-block at kb
__device__ __forceinline__ void bsolve_update_body(const BaDev& D, const StFlags& F, const int kb, const int bx, double* s_x, double (*s_p)[64], const bool flags_checked) {
  const int np = D.npad, tid = threadIdx.x;
  const int ke = min(kb + SBLK, np);
  const int nr = ke - kb;
  const int cl = tid & 63, rg = tid >> 6;                           // 64 columns x 16 row groups, 16 rows each, all loads in flight
  const int c = bx * 64 + cl;
  double lv[SBLK / 16];
#pragma unroll
  for (int u = 0; u < SBLK / 16; u++) {
    const int rr = rg + 16 * u;
    lv[u] = (c < kb && rr < nr) ? D.S[(size_t)(kb + rr) * np + c] : 0.0;
  }
  if (!flags_checked && (F.done || !F.valid || F.chol_fail)) return;
  if (tid < nr) s_x[tid] = D.rhs[kb + tid];
  __syncthreads();
  double sum = 0.0;
#pragma unroll
  for (int u = 0; u < SBLK / 16; u++) { const int rr = rg + 16 * u; if (rr < nr) sum += lv[u] * s_x[rr]; }
  s_p[rg][cl] = sum;
  __syncthreads();
  if (tid < 64 && c < kb) {
    double t = 0.0;
#pragma unroll
    for (int g = 0; g < 16; g++) t += s_p[g][tid];
    D.rhs[c] -= t;
  }
}
__global__ __launch_bounds__(1024) void k_chol_bsolve_update(const BaDev* __restrict__ Dv, int kb) {
  const BaDev D = Dv[blockIdx.y];
  const StFlags F = ld_flags(D.st);
  __shared__ double s_x[SBLK], s_p[16][64];
  if (kb >= D.npad || (int)blockIdx.x * 64 >= kb) return;
  bsolve_update_body(D, F, kb, (int)blockIdx.x, s_x, s_p, false);
}

// The whole backward substitution of a system with a NARROW skyline as ONE launch of one workgroup (round 5): super-block after
// super-block from the bottom, the diagonal part as k_chol_bsolve_diag makes it, then the contribution to the rows above for the
// 64-column chunks that can hold a non-zero of the super-block's rows - the columns before the first tile column of its tile rows
// (tile_first) have zero L entries, their running values would have an exact zero subtracted.  Same bodies, same order per entry:
// the bits of the solution do not change.  A C5-size GlobalBA (12 super-blocks, band 3) walked 23 launches of 4.7 - 13.8 us.
__global__ __launch_bounds__(1024) void k_chol_bsolve_sky(const BaDev* __restrict__ Dv) {
  const BaDev D = Dv[blockIdx.y];
  const StFlags F = ld_flags(D.st);
  if (F.done || !F.valid || F.chol_fail) return;
  __shared__ double s_y[SBLK], s_x[NB];
  __shared__ __attribute__((aligned(16))) double s_raw[NB * (SBLK - NB)];      // the diagonal part's partial products; the update's s_x [256] + s_p [16][64] alias it
  double (*s_p)[SBLK - NB] = (double (*)[SBLK - NB])s_raw;
  double* u_x = s_raw; double (*u_p)[64] = (double (*)[64])(s_raw + SBLK);
  const int np = D.npad;
  for (int kb = ((np - 1) / SBLK) * SBLK; kb >= 0; kb -= SBLK) {
    bsolve_diag_body(D, F, kb, s_y, s_x, s_p, true);
    __syncthreads();                                                // (the super-block's solution is in D.rhs for every thread of the workgroup)
    if (kb > 0) {
      int fmin = kb / NB;
      for (int i = kb / NB; i < min(kb + SBLK, np) / NB; i++) fmin = min(fmin, D.tile_first[i]);
      for (int bx = (fmin * NB) / 64; bx * 64 < kb; bx++) { bsolve_update_body(D, F, kb, bx, u_x, u_p, true); __syncthreads(); }
    }
  }
}

// ---- the same substitution on a few WAVES (round 6) -------------------------------------------------------------------------------
// k_chol_bsolve_sky spends its time at barriers: per 32-row block step a 1024-thread workgroup makes four of them (products -> LDS, 32
// sequential adds by 32 threads, products for the rows above, their sums), 1.7 us per step - 34 us of a single C4 solve's 237 per
// iteration, 176 of a C5 GlobalBA's 970.  Here a step is two matrix-vector products by single (half-)waves and two four-wave barriers:
//   wave 0 (lanes 0 - 31, lane = column c):   x[c] = sum_r Linv_T[r][c] y[r]            - the 32 terms added in order, as the 32 threads did
//   waves 1, 2 (two half-waves each, one tile column cb = T - 1 .. T - 4 of the row's envelope per half-wave):  y_cb[c] -= sum_r L(T, cb)[r][c] x[r]
// The 32 x 32 blocks of a step do not depend on the running solution: every wave copies ITS blocks of step T - 2 into its own LDS slot
// with direct-to-LDS loads (global_load_lds_dwordx4: 1 KB per instruction, no registers, nothing the compiler waits for) while steps T
// and T - 1 run; a slot is read column-wise two steps later behind a hand-written s_waitcnt vmcnt(N) that lets the younger copies stay in
// flight.  (A first version held the blocks in registers, requested ahead with ordinary loads: the compiler's wait before the first use
// was vmcnt(0) - every step then waited for the loads issued at the end of the previous one, 2 us per step.)
// THE BITS ARE k_chol_bsolve_sky's.  Every entry receives the same products in the same order: inside a 256-row super-block the blocks
// from the bottom, a block's 32 terms summed from zero in row order and subtracted once; between super-blocks the contribution of a whole
// super-block to a column above it summed as bsolve_update_body does - sixteen groups of rows g, g + 16, g + 32, ... each from zero, the
// groups added in order, one subtraction.  What is left out are products with the exact zeros outside the skyline (tile_first, and the
// rows of a super-block that a band of <= 4 tiles cannot connect to the columns above it): a sum that starts at +0.0 does not change
// when +-0.0 is added.  tools/bsolve_ab.py and tests/test_gpu_ba.py compare the two kernels' solutions bit for bit.
#define BW_TPB 256
#define BW_SLOTS 3
#define BW_BLK (NB * NB)                 /* doubles per block in a slot: row-major, 256-byte rows */
typedef const double __attribute__((address_space(1))) * gcdp;
#define BW_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
static_assert(BS_SKY_BAND <= 4, "k_chol_bsolve_sky4 walks four tile columns per tile row");
__global__ __launch_bounds__(BW_TPB) void k_chol_bsolve_sky4(const BaDev* __restrict__ Dv) {
  const BaDev D = Dv[blockIdx.y];
  const StFlags F = ld_flags(D.st);
  if (F.done || !F.valid || F.chol_fail) return;
  __shared__ double s_y[SBLK], s_x[NB], s_grp[16][4 * NB];
  __shared__ int s_tf[1024];
  __shared__ __attribute__((aligned(1024))) double s_blk[BW_SLOTS][5 * BW_BLK];      // per slot: wave 0's block, wave 1's two, wave 2's two
  const int np = D.npad, nbt = np / NB, tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, h = lane >> 5, c = lane & 31;
  const gcdp S = (gcdp)D.S, Dinv = (gcdp)D.Dinv;
  const bool tf_lds = nbt <= 1024;
  if (tf_lds) for (int i = tid; i < nbt; i += BW_TPB) s_tf[i] = D.tile_first[i];
  __syncthreads();
  auto tfv = [&](int T) -> int { return tf_lds ? s_tf[T] : D.tile_first[T]; };
  // this half-wave's tile column of tile row T (waves 1, 2), or -1: inside T's super-block and inside its envelope
  auto col_of = [&](int T) -> int {
    const int kbt = (T / SB_NBLK) * SB_NBLK, cb = T - 1 - 2 * (w - 1) - h;
    return ((w == 1 || w == 2) && cb >= kbt && cb >= tfv(T)) ? cb : -1;
  };
  // the copy of this wave's blocks of step T into its part of slot T % 3 (wave 0: eight instructions of four rows; waves 1, 2: sixteen
  // of two rows per half-wave - block h's row r lands at (r >> 1) * 128 + h * 64 + (r & 1) * 32 doubles)
  auto issue = [&](int T) -> bool {                              // returns whether this WAVE issued copies for step T (wave-uniform)
    if (T < 0 || w > 2) return false;
    double* slot = &s_blk[T % BW_SLOTS][w == 0 ? 0 : (2 * w - 1) * BW_BLK];
    if (w == 0) {
      const gcdp src = Dinv + ((size_t)T * NB + (lane >> 4)) * NB + 2 * (lane & 15);
#pragma unroll
      for (int j = 0; j < 8; j++)
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + (size_t)4 * j * NB),
                                         (void __attribute__((address_space(3)))*)(slot + 128 * j), 16, 0, 0);
      return true;
    } else {
      const int cb = col_of(T);
      const gcdp src = S + ((size_t)T * NB + ((lane & 31) >> 4)) * np + (size_t)max(cb, 0) * NB + 2 * (lane & 15);
#pragma unroll
      for (int j = 0; j < 16; j++)
        if (cb >= 0)                                             // (an inactive half-wave writes nothing; the instruction count per step stays 16)
          __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + (size_t)2 * j * np),
                                           (void __attribute__((address_space(3)))*)(slot + 128 * j), 16, 0, 0);
      return __any(cb >= 0) != 0;
    }
  };
#ifdef BW_PROF
  unsigned long long bw_t = __builtin_amdgcn_s_memrealtime();
  unsigned long long* bw_acc = &g_df_stamp[0][0] + (w == 1 ? 8 : 0);
  const bool bw_on = (w == 0 || w == 1) && lane == 0 && blockIdx.y == 0;
#define BW_ST(k) do { if (bw_on) { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); bw_acc[k] += t_ - bw_t; bw_t = t_; } } while (0)
#else
#define BW_ST(k) do { } while (0)
#endif
  int T = nbt - 1;
  issue(T);
  bool act1 = issue(T - 1);                                     // did this wave issue copies for the step after the current one
  const gcdp zrow = S + (size_t)np * np;
  // The running values a super-block starts from: its lower 128 rows have had the super-block below subtracted (a band of <= 4 tiles
  // reaches no further) - they come out of that super-block's end, through LDS; its upper 128 rows are still z, and so is what the lower
  // ones had before that subtraction: both are requested a super-block ahead.  (k_chol_bsolve_sky seeds D.rhs with z and sends every
  // running value through it: a store, a barrier and a load between super-blocks.)
  double z_up = 0.0, z_lo = 0.0;                                // z of row (first row of the NEXT super-block) + tid, tid < 128 / of the row 128 further down
  {
    const int kb0 = (T / SB_NBLK) * SB_NBLK * NB;
    if (tid < np - kb0) s_y[tid] = zrow[kb0 + tid];
    if (kb0 > 0 && tid < 4 * NB) { z_up = zrow[kb0 - SBLK + tid]; z_lo = zrow[kb0 - 4 * NB + tid]; }
  }
  __syncthreads();
  BW_ST(0);                                                     // prologue
#pragma unroll 1
  for (; T >= 0; T--) {
    const int kbt = (T / SB_NBLK) * SB_NBLK, kb = kbt * NB, bb = T - kbt;
    const int ke = min(kb + SBLK, np), nr = ke - kb;
    // (waves 1, 2 request their blocks of step T - 2 while wave 0 multiplies, wave 0 while they do: nobody's copy sits on the chain)
    // This step's blocks have landed when at most the YOUNGER copies are outstanding - counted exactly: a wave whose two half-waves have no
    // tile column in a step issues no copy for it (waves 1, 2: sixteen instructions per step in which either half has one; wave 0: eight for
    // every T >= 0, and at this point only step T - 1's are younger).  A fixed vmcnt(32) / vmcnt(8) would let a step through with its own
    // copies in flight whenever the younger steps issued none (the first rows of a super-block for wave 2; the last step for wave 0).
    bool act2 = false;
    if (w != 0) {
      act2 = issue(T - 2);
      const int younger = (act1 ? 1 : 0) + (act2 ? 1 : 0);
      if (younger == 2) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (act1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    BW_ST(1);                                                   // top of the step: copies requested (waves 1, 2), this step's landed
    const double* slot = &s_blk[T % BW_SLOTS][w == 0 ? 0 : (2 * (w > 2 ? 2 : w) - 1) * BW_BLK];
    if (w == 0) {
      if (h == 0) {
        // (all 48 LDS reads first, waited for once: left to the compiler they are issued two at a time between the products, and the
        // 32-term chain pays the LDS latency sixteen times - 610 ns per step instead of ~250)
        double m[NB], yv[NB];
#pragma unroll
        for (int r = 0; r < NB; r++) m[r] = slot[NB * r + c];
#pragma unroll
        for (int r = 0; r < NB; r++) yv[r] = s_y[NB * bb + r];
        pin8(m); pin8(m + 8); pin8(m + 16); pin8(m + 24); pin8(yv); pin8(yv + 8); pin8(yv + 16); pin8(yv + 24);
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < NB; r++) sum += m[r] * yv[r];
        s_x[c] = sum; s_y[NB * bb + c] = sum;                   // (the wave's reads of y_T are all behind it)
      }
    }
    BW_ST(2);                                                   // wave 0: x = Linv^T y
    BW_LDS_BARRIER();
    BW_ST(3);                                                   // first barrier
    if (w == 0) act2 = issue(T - 2);
    {
      const int cb = col_of(T);
      if (cb >= 0) {
        double m[NB], xv[NB];
#pragma unroll
        for (int r = 0; r < NB; r++) m[r] = slot[(r >> 1) * 128 + h * 64 + (r & 1) * 32 + c];
#pragma unroll
        for (int r = 0; r < NB; r++) xv[r] = s_x[r];
        double yo = s_y[NB * (cb - kbt) + c];
        pin8(m); pin8(m + 8); pin8(m + 16); pin8(m + 24); pin8(xv); pin8(xv + 8); pin8(xv + 16); pin8(xv + 24); asm volatile("" : "+v"(yo));
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < NB; r++) sum += m[r] * xv[r];
        s_y[NB * (cb - kbt) + c] = yo - sum;
      }
    }
    BW_ST(4);                                                   // waves 1, 2: the updates (wave 0: its copies)
    BW_LDS_BARRIER();
    BW_ST(5);                                                   // second barrier
    if (bb == 0) {                                              // the super-block ends: solution out, its share of the rows above
      if (tid < nr) D.rhs[kb + tid] = s_y[tid];
      if (kb > 0) {                                             // a band of <= 4 tiles: rows 0 .. 127 of the super-block reach columns kb - 128 .. kb - 1
        const int q8 = (tid >> 7) * 8, cl = tid & 127, cg = kb - 4 * NB + cl;
        double lv[8][8];                                        // eight of the sixteen row groups per thread, all 64 entries requested together
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
          for (int i = 0; i < 4; i++) {                         // (no branches around the loads: a row beyond the system reads the last one and counts as zero)
            const int r0 = NB * i + q8 + j, r1 = r0 + 16;
            lv[j][2 * i] = S[((size_t)kb + min(r0, nr - 1)) * np + cg];
            lv[j][2 * i + 1] = S[((size_t)kb + min(r1, nr - 1)) * np + cg];
          }
        // what the super-block after the next one starts from (in flight across the sums below)
        const double run = z_lo, up = z_up;
        if (kb >= 2 * SBLK && tid < 4 * NB) { z_up = zrow[kb - 2 * SBLK + tid]; z_lo = zrow[kb - SBLK - 4 * NB + tid]; }
        // (the solution's entries a thread multiplies with: read together, in two batches, before the chains - see the steps above)
#pragma unroll
        for (int jh = 0; jh < 8; jh += 4) {
          double xs[4][8];
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int r0 = NB * i + q8 + jh + j, r1 = r0 + 16;
              xs[j][2 * i] = s_y[min(r0, SBLK - 1)]; xs[j][2 * i + 1] = s_y[min(r1, SBLK - 1)];
            }
          pin8(xs[0]); pin8(xs[1]); pin8(xs[2]); pin8(xs[3]);
          if (jh == 0) { pin8(lv[0]); pin8(lv[1]); pin8(lv[2]); pin8(lv[3]); pin8(lv[4]); pin8(lv[5]); pin8(lv[6]); pin8(lv[7]); }
#pragma unroll
          for (int j = 0; j < 4; j++) {
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int r0 = NB * i + q8 + jh + j, r1 = r0 + 16;
              if (r0 < nr) sum += lv[jh + j][2 * i] * xs[j][2 * i];
              if (r1 < nr) sum += lv[jh + j][2 * i + 1] * xs[j][2 * i + 1];
            }
            s_grp[q8 + jh + j][cl] = sum;
          }
        }
        __syncthreads();                                        // (the sums are out; everybody has read the solution in s_y)
        if (tid < 4 * NB) {
          double gs[16];
#pragma unroll
          for (int g = 0; g < 16; g++) gs[g] = s_grp[g][tid];
          pin8(gs); pin8(gs + 8);
          double t = 0.0;
#pragma unroll
          for (int g = 0; g < 16; g++) t += gs[g];
          s_y[4 * NB + tid] = run - t;                          // the next super-block's rows 128 .. 255
          s_y[tid] = up;                                        // ... and 0 .. 127
        }
      }
      __syncthreads();
      BW_ST(6);                                                 // end of a super-block
    }
    act1 = act2;
  }
  BW_ST(7);
}
