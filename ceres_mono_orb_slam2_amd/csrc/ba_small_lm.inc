// PoseOptimization and OptimizeSim3 - part of the translation unit ba_solver.hip (textually included there; not compiled on its own).
// whole-solve-in-one-workgroup LM kernels (k_pose_lm, k_sim3_lm).

// ============================================================================ PoseOptimization
// upper-triangle index of a symmetric 6x6 stored as 21 values
__device__ __forceinline__ int sym6(int a, int b) { return a <= b ? a * 6 - a * (a - 1) / 2 + (b - a) : b * 6 - b * (b - 1) / 2 + (a - b); }

#ifdef ORBHIP_CHOL_PROF
__device__ unsigned long long g_pose_ticks[8];
#define POSE_T(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); g_pose_ticks[i] += t_ - pt_; pt_ = t_; } } while (0)
#else
#define POSE_T(i) do { } while (0)
#endif
#define POSE_R 8
__global__ __launch_bounds__(256) void k_pose_lm(const double* __restrict__ K4s, double* __restrict__ poses,
                                                 const double* __restrict__ Xw, const double* __restrict__ uv,
                                                 const float* __restrict__ inv_sigma2, const int* __restrict__ offsets,
                                                 uint8_t* __restrict__ outlier, int* __restrict__ n_inliers,
                                                 ba_summary* __restrict__ summaries, int max_iters, double huber) {
  __shared__ double s_red[4 * 28], s_sum[28];
  __shared__ double s_x[7], s_cand[7], s_scale[6], s_H[21], s_g[6];
  __shared__ double s_radius, s_dec, s_xcost, s_xnorm, s_mcc, s_stepnorm, s_init;
  __shared__ int s_iter, s_term, s_done, s_valid, s_accept, s_invalid, s_succ, s_nbad;
  const int p = blockIdx.x, tid = threadIdx.x;
#ifdef ORBHIP_CHOL_PROF
  unsigned long long pt_ = __builtin_amdgcn_s_memrealtime();
#endif
  const int lo = offsets[p], n = offsets[p + 1] - lo;
  const double* K4 = K4s + 4 * p;
  double* pose = poses + 7 * p;
  if (n < 3) {                                              // src/CeresOptimizer.cc:330
    if (tid == 0) {
      n_inliers[p] = 0;
      if (summaries) { ba_summary s; memset(&s, 0, sizeof(s)); summaries[p] = s; }
    }
    return;
  }
  if (tid < 7) s_x[tid] = pose[tid];
  if (tid == 0) { s_radius = 1e4; s_dec = 2.0; s_iter = 0; s_term = 0; s_done = 0; s_invalid = 0; s_succ = 0; s_nbad = 0; }
  // The observations never change during the solve: up to POSE_R per thread (frames of up to 2048 map points) are read
  // ONCE into registers; every evaluation of the LM loop - two passes over the observations per iteration - then runs
  // without a global load.  (One workgroup per frame = one wave per SIMD: the per-iteration loads were pure exposed latency.)
  const bool in_regs = n <= 256 * POSE_R;
  double oX[POSE_R][3], oU[POSE_R][2], oW[POSE_R];
  if (in_regs) {
#pragma unroll
    for (int u = 0; u < POSE_R; u++) {
      const int i = tid + 256 * u;
      const size_t g = (size_t)lo + (size_t)min(i, n - 1);
      oX[u][0] = Xw[3 * g]; oX[u][1] = Xw[3 * g + 1]; oX[u][2] = Xw[3 * g + 2];
      oU[u][0] = uv[2 * g]; oU[u][1] = uv[2 * g + 1];
      oW[u] = (double)inv_sigma2[g];
    }
  }
  const double k4r[4] = {K4[0], K4[1], K4[2], K4[3]};
  // f(i, X, u, v, w) over this thread's observations
  auto for_obs = [&](auto f) {
    if (in_regs) {
#pragma unroll
      for (int u = 0; u < POSE_R; u++) { const int i = tid + 256 * u; if (i < n) f(i, oX[u], oU[u][0], oU[u][1], oW[u]); }
    } else {
      for (int i = tid; i < n; i += 256) {
        const size_t g = (size_t)lo + i;
        const double X[3] = {Xw[3 * g], Xw[3 * g + 1], Xw[3 * g + 2]};
        f(i, X, uv[2 * g], uv[2 * g + 1], (double)inv_sigma2[g]);
      }
    }
  };
  __syncthreads();

  // cost, gradient and Gauss-Newton block of the residuals at pose xe, reduced into s_sum[0 .. 27] (all threads)
  auto accumulate = [&](const double* xe) {
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    for_obs([&](int, const double* X, double u0, double v0, double w) {
      double r[2], Jc[12];
      double rho = reproj_eval(k4r, xe, X, u0, v0, w, 1, huber, r, Jc, nullptr);
      acc[0] += 0.5 * rho;
#pragma unroll
      for (int a = 0; a < 6; a++) {
        acc[1 + a] += Jc[a] * r[0] + Jc[6 + a] * r[1];
#pragma unroll
        for (int b = a; b < 6; b++) acc[7 + sym6(a, b)] += Jc[a] * Jc[b] + Jc[6 + a] * Jc[6 + b];
      }
    });
    block_reduce_dpp<28>(acc, s_red, s_sum);
  };
  // thread 0: the sums become the state at s_x (the iterate they were evaluated at)
  auto adopt = [&](bool first) {
    s_xcost = s_sum[0];
    for (int a = 0; a < 6; a++) s_g[a] = s_sum[1 + a];
    for (int k = 0; k < 21; k++) s_H[k] = s_sum[7 + k];
    if (first) {
      for (int a = 0; a < 6; a++) s_scale[a] = 1.0 / (1.0 + sqrt(s_H[sym6(a, a)]));
      s_init = s_xcost;
    }
    double xn = 0;
    for (int k = 0; k < 7; k++) xn += s_x[k] * s_x[k];
    s_xnorm = sqrt(xn);
    // gradient max norm = || x - Plus(x, -g) ||_inf
    double gmax = 0;
    for (int k = 0; k < 3; k++) gmax = fmax(gmax, fabs(s_g[k]));
    double d[3] = {-s_g[3], -s_g[4], -s_g[5]}, qn[4];
    quat_plus(s_x + 3, d, qn);
    for (int k = 0; k < 4; k++) gmax = fmax(gmax, fabs(s_x[3 + k] - qn[k]));
    if (gmax <= 1e-10) { s_term = 1; s_done = 1; }
  };

  accumulate(s_x);
  if (tid == 0) adopt(true);
  __syncthreads();
  POSE_T(0);                               // loads + first evaluation
  int done = s_done;
  while (!done) {
    __syncthreads();                       // every thread has consumed the previous flags
    if (tid < 64) {
      // Wave 0 solves the damped 6x6 system with lanes 0..5 holding one row each: a column of the Cholesky factor costs one
      // sqrt and ONE division latency instead of (5 - j) dependent ones (fp64 division ~ 30 dependent instructions on a
      // lone wave; the serial thread-0 version spent 2.7 us per iteration here).  Every sum keeps the serial order of
      // small_chol_solve, so the step is bit-identical to it; scalars are computed redundantly by all lanes, lane 0 stores.
      const int r = min(tid, 5);
      const int iter = s_iter;
      const double radius = s_radius;
      if (tid == 0) { s_valid = 0; s_accept = 0; }
      if (iter >= max_iters) { if (tid == 0) { s_term = 0; s_done = 1; } }
      else if (radius <= 1e-32) { if (tid == 0) { s_term = 6; s_done = 1; } }
      else {
        if (tid == 0) s_iter = iter + 1;
        double hs[6], L[6];
        const double sr = s_scale[r];
        const double gsr = s_g[r] * sr;
        double hrr = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) { hs[c] = s_H[sym6(r, c)] * sr * s_scale[c]; L[c] = hs[c]; if (c == r) hrr = hs[c]; }
        const double damp = fmin(fmax(hrr, 1e-6), 1e32) / radius;
#pragma unroll
        for (int c = 0; c < 6; c++) if (c == r) L[c] += damp;
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; j++) {
          double t = L[j];
#pragma unroll
          for (int k = 0; k < j; k++) t -= L[k] * lane_bcast(L[k], j);
          const double dj = lane_bcast(t, j);
          if (!(dj > 0.0) || !isfinite(dj)) { ok = false; break; }
          const double d = sqrt(dj);
          L[j] = (r == j) ? d : t / d;
        }
        POSE_T(5);
        double y[6];
        if (ok) {
          double Lu[6][6];
#pragma unroll
          for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int k = 0; k <= i; k++) Lu[i][k] = lane_bcast(L[k], i);
          }
#pragma unroll
          for (int i = 0; i < 6; i++) { double t = lane_bcast(gsr, i); for (int k = 0; k < i; k++) t -= Lu[i][k] * y[k]; y[i] = t / Lu[i][i]; }
#pragma unroll
          for (int i = 5; i >= 0; i--) { double t = y[i]; for (int k = i + 1; k < 6; k++) t -= Lu[k][i] * y[k]; y[i] = t / Lu[i][i]; }
        }
        double mcc = 0;
        if (ok) {
          double hsum = 0, yr = 0;
#pragma unroll
          for (int c = 0; c < 6; c++) { hsum += hs[c] * (-y[c]); if (c == r) yr = y[c]; }
          const double term = (-yr) * (gsr + 0.5 * hsum);
#pragma unroll
          for (int c = 0; c < 6; c++) mcc -= lane_bcast(term, c);
        }
        POSE_T(6);
        if (!ok || !(mcc > 0.0)) {
          if (tid == 0) {
            if (++s_invalid >= 5) { s_term = 5; s_done = 1; }                 // HandleInvalidStep returns BEFORE StepIsInvalid: the radius stays
            else { s_radius = radius / s_dec; s_dec *= 2; }
          }
        } else {
          double d[3], cand[7];
          for (int k = 0; k < 3; k++) cand[k] = s_x[k] + (-y[k]) * s_scale[k];
          for (int k = 0; k < 3; k++) d[k] = (-y[3 + k]) * s_scale[3 + k];
          quat_plus(s_x + 3, d, cand + 3);
          double sn = 0;
          for (int k = 0; k < 7; k++) { double e = s_x[k] - cand[k]; sn += e * e; }
          if (tid == 0) {
            s_invalid = 0; s_valid = 1; s_mcc = mcc;
            for (int k = 0; k < 7; k++) s_cand[k] = cand[k];
            s_stepnorm = sqrt(sn);
          }
        }
        POSE_T(7);
      }
    }
    __syncthreads();
    POSE_T(1);                             // thread 0: damped solve, candidate
    done = s_done;
    const int valid = s_valid;
    if (done) break;
    if (!valid) continue;
    // The candidate is evaluated IN FULL - cost, gradient and Gauss-Newton block in one pass over the observations: nearly
    // every step is accepted, and the sums are then the next iteration's state (a cost-only pass followed by a second, full
    // pass at the same pose cost a third of the kernel's 47 us at 1500 observations; a rejected step wastes the Jacobians)
    accumulate(s_cand);
    POSE_T(2);                             // evaluation at the candidate
    if (tid == 0) {
      double cand_cost = s_sum[0];
      if (!isfinite(cand_cost)) cand_cost = DBL_MAX;
      if (s_stepnorm <= 1e-8 * (s_xnorm + 1e-8)) { s_term = 2; s_done = 1; }
      else {
        double cost_change = s_xcost - cand_cost;
        if (fabs(cost_change) <= 1e-6 * s_xcost) { s_term = 3; s_done = 1; }
        else {
          double rel = cost_change / s_mcc;
          if (rel > 1e-3) {
            s_accept = 1; s_succ++;
            for (int k = 0; k < 7; k++) s_x[k] = s_cand[k];
            const double c3 = 2.0 * rel - 1.0;               // pow(c3, 3) as two products: the generic fp64 pow costs
            s_radius = fmin(1e16, s_radius / fmax(1.0 / 3.0, 1.0 - c3 * c3 * c3));   // ~1 us of lone-thread time per iteration
            s_dec = 2.0;
            adopt(false);
          } else {
            s_radius /= s_dec; s_dec *= 2.0;
          }
        }
      }
    }
    __syncthreads();
    POSE_T(3);                             // thread 0: decision, new state
    done = s_done;
  }
  __syncthreads();
  // CheckOutliers with the un-normalised quaternion (:333), then normalise for SetPose (:336)
  int bad = 0;
  for_obs([&](int i, const double* X, double u0, double v0, double w) {
    int o = check_outlier(k4r, s_x, X, u0, v0, w, 5.991, nullptr);
    outlier[lo + i] = (uint8_t)o;
    bad += o;
  });
  if (bad) atomicAdd(&s_nbad, bad);
  __syncthreads();
  if (tid == 0) {
    double* q = s_x + 3;
    double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 3; k++) pose[k] = s_x[k];
    for (int k = 0; k < 4; k++) pose[3 + k] = q[k] / nq;
    n_inliers[p] = n - s_nbad;
    if (summaries) {
      ba_summary s;
      s.initial_cost = s_init; s.final_cost = s_xcost; s.iterations = s_iter; s.successful_steps = s_succ;
      s.termination = s_term; s.final_radius = s_radius;
      summaries[p] = s;
    }
  }
  POSE_T(4);                               // outlier check, write-back
}


// ============================================================================ OptimizeSim3
// The WHOLE solve of one keyframe pair inside one workgroup, as k_pose_lm: 2n Sim3ErrorTerm residual blocks on a single
// 7-parameter block (tangent of S12), HuberLoss(sqrt(th2)), Sim3Parameterization::Plus, <= 100 iterations
// (src/CeresOptimizer.cc:601-735).  One workgroup per problem; offsets[] delimits the correspondences.
__device__ __forceinline__ int sym7(int a, int b) { return a <= b ? a * 7 - a * (a - 1) / 2 + (b - a) : b * 7 - b * (b - 1) / 2 + (a - b); }

__device__ bool chol7_solve(double* A, double* b) {
  const int n = 7;
  for (int j = 0; j < n; j++) {
    double d = A[j * n + j];
    for (int k = 0; k < j; k++) d -= A[j * n + k] * A[j * n + k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    d = sqrt(d);
    A[j * n + j] = d;
    for (int i = j + 1; i < n; i++) {
      double s = A[i * n + j];
      for (int k = 0; k < j; k++) s -= A[i * n + k] * A[j * n + k];
      A[i * n + j] = s / d;
    }
  }
  for (int i = 0; i < n; i++) { double s = b[i]; for (int k = 0; k < i; k++) s -= A[i * n + k] * b[k]; b[i] = s / A[i * n + i]; }
  for (int i = n - 1; i >= 0; i--) { double s = b[i]; for (int k = i + 1; k < n; k++) s -= A[k * n + i] * b[k]; b[i] = s / A[i * n + i]; }
  return true;
}

__global__ __launch_bounds__(256) void k_sim3_lm(const double* __restrict__ K1s, const double* __restrict__ K2s, double* __restrict__ s12s,
                                                 const double* __restrict__ P3D2c, const double* __restrict__ obs1,
                                                 const float* __restrict__ w1, const double* __restrict__ P3D1c,
                                                 const double* __restrict__ obs2, const float* __restrict__ w2,
                                                 const int* __restrict__ offsets, const double* __restrict__ th2s,
                                                 uint8_t* __restrict__ outlier, int* __restrict__ n_inliers,
                                                 ba_summary* __restrict__ summaries, int max_iters) {
  __shared__ double s_red[4 * 36], s_sum[36];
  __shared__ double s_x[7], s_cand[7], s_S[7], s_Si[7], s_scale[7], s_H[28], s_g[7];
  __shared__ double s_radius, s_dec, s_xcost, s_xnorm, s_mcc, s_stepnorm, s_init;
  __shared__ int s_iter, s_term, s_done, s_valid, s_accept, s_invalid, s_succ, s_nbad;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int lo = offsets[p], n = offsets[p + 1] - lo;
  const double* K1 = K1s + 4 * p;
  const double* K2 = K2s + 4 * p;
  const double huber = sqrt(th2s[p]);                         // :619
  if (tid == 0) {
    s3_log(s12s + 7 * p, s_x);                                // :605
    s3_exp(s_x, s_S); s3_inverse(s_S, s_Si);
    s_radius = 1e4; s_dec = 2.0; s_iter = 0; s_term = 0; s_done = (n == 0); s_invalid = 0; s_succ = 0; s_nbad = 0;
    s_xcost = 0.0; s_init = 0.0;
  }
  __syncthreads();

  auto evaluate = [&](bool first) {          // expects s_S / s_Si = exp(s_x) and its inverse
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; k++) acc[k] = 0.0;
    for (int i = tid; i < 2 * n; i += 256) {
      const int g = lo + (i >> 1), inv = i & 1;              // residual-block order: forward then inverse term per match
      double r[2], J[14];
      const double rho = inv ? s3_term_eval(K2, s_Si, P3D1c + 3 * (size_t)g, obs2[2 * (size_t)g], obs2[2 * (size_t)g + 1], (double)w2[g], huber, r, J)
                             : s3_term_eval(K1, s_S, P3D2c + 3 * (size_t)g, obs1[2 * (size_t)g], obs1[2 * (size_t)g + 1], (double)w1[g], huber, r, J);
      acc[0] += 0.5 * rho;
#pragma unroll
      for (int a = 0; a < 7; a++) {
        acc[1 + a] += J[a] * r[0] + J[7 + a] * r[1];
#pragma unroll
        for (int b = a; b < 7; b++) acc[8 + sym7(a, b)] += J[a] * J[b] + J[7 + a] * J[7 + b];
      }
    }
    block_reduce<36>(acc, s_red, s_sum);
    if (tid == 0) {
      s_xcost = s_sum[0];
      for (int a = 0; a < 7; a++) s_g[a] = s_sum[1 + a];
      for (int k = 0; k < 28; k++) s_H[k] = s_sum[8 + k];
      if (first) {
        for (int a = 0; a < 7; a++) s_scale[a] = 1.0 / (1.0 + sqrt(s_H[sym7(a, a)]));
        s_init = s_xcost;
      }
      double xn = 0;
      for (int k = 0; k < 7; k++) xn += s_x[k] * s_x[k];
      s_xnorm = sqrt(xn);
      double mg[7], xp[7], gmax = 0;                          // gradient max norm = || x - Plus(x, -g) ||_inf
      for (int k = 0; k < 7; k++) mg[k] = -s_g[k];
      s3_plus(s_x, mg, xp);
      for (int k = 0; k < 7; k++) gmax = fmax(gmax, fabs(s_x[k] - xp[k]));
      if (gmax <= 1e-10) { s_term = 1; s_done = 1; }
    }
    __syncthreads();
  };

  int done = s_done;
  if (!done) { evaluate(true); done = s_done; }
  while (!done) {
    __syncthreads();
    if (tid == 0) {
      s_valid = 0; s_accept = 0;
      if (s_iter >= max_iters) { s_term = 0; s_done = 1; }
      else if (s_radius <= 1e-32) { s_term = 6; s_done = 1; }
      else {
        s_iter++;
        double A[49], y[7], Hs[49], gs[7];
        for (int a = 0; a < 7; a++) {
          gs[a] = s_g[a] * s_scale[a];
          for (int b = 0; b < 7; b++) Hs[a * 7 + b] = s_H[sym7(a, b)] * s_scale[a] * s_scale[b];
        }
        for (int k = 0; k < 49; k++) A[k] = Hs[k];
        for (int a = 0; a < 7; a++) A[a * 8] += fmin(fmax(Hs[a * 8], 1e-6), 1e32) / s_radius;
        for (int a = 0; a < 7; a++) y[a] = gs[a];
        bool ok = chol7_solve(A, y);
        double mcc = 0;
        if (ok) {
          for (int a = 0; a < 7; a++) {
            double hs = 0;
            for (int b = 0; b < 7; b++) hs += Hs[a * 7 + b] * (-y[b]);
            mcc -= (-y[a]) * (gs[a] + 0.5 * hs);
          }
        }
        if (!ok || !(mcc > 0.0)) {
          if (++s_invalid >= 5) { s_term = 5; s_done = 1; }                   // (as k_pose_lm: the fifth invalid step ends the solve, the radius stays)
          else { s_radius /= s_dec; s_dec *= 2; }
        } else {
          s_invalid = 0; s_valid = 1; s_mcc = mcc;
          double d[7];
          for (int k = 0; k < 7; k++) d[k] = (-y[k]) * s_scale[k];
          s3_plus(s_x, d, s_cand);
          double sn = 0;
          for (int k = 0; k < 7; k++) { double e = s_x[k] - s_cand[k]; sn += e * e; }
          s_stepnorm = sqrt(sn);
          s3_exp(s_cand, s_S); s3_inverse(s_S, s_Si);        // candidate transform for the cost pass
        }
      }
    }
    __syncthreads();
    done = s_done;
    const int valid = s_valid;
    if (done) break;
    if (!valid) continue;
    double acc[1] = {0.0};
    for (int i = tid; i < 2 * n; i += 256) {
      const int g = lo + (i >> 1), inv = i & 1;
      double r[2];
      acc[0] += 0.5 * (inv ? s3_term_eval(K2, s_Si, P3D1c + 3 * (size_t)g, obs2[2 * (size_t)g], obs2[2 * (size_t)g + 1], (double)w2[g], huber, r, nullptr)
                           : s3_term_eval(K1, s_S, P3D2c + 3 * (size_t)g, obs1[2 * (size_t)g], obs1[2 * (size_t)g + 1], (double)w1[g], huber, r, nullptr));
    }
    block_reduce<1>(acc, s_red, s_sum);
    if (tid == 0) {
      double cand_cost = s_sum[0];
      if (!isfinite(cand_cost)) cand_cost = DBL_MAX;
      if (s_stepnorm <= 1e-8 * (s_xnorm + 1e-8)) { s_term = 2; s_done = 1; }
      else {
        const double cost_change = s_xcost - cand_cost;
        if (fabs(cost_change) <= 1e-6 * s_xcost) { s_term = 3; s_done = 1; }
        else {
          const double rel = cost_change / s_mcc;
          if (rel > 1e-3) {
            s_accept = 1; s_succ++;
            for (int k = 0; k < 7; k++) s_x[k] = s_cand[k];   // s_S / s_Si already hold exp(cand)
            s_radius = fmin(1e16, s_radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rel - 1.0, 3)));
            s_dec = 2.0;
          } else {
            s_radius /= s_dec; s_dec *= 2.0;
          }
        }
      }
    }
    __syncthreads();
    done = s_done;
    const int accept = s_accept;
    if (done) break;
    if (accept) { evaluate(false); done = s_done; }
  }
  __syncthreads();
  if (tid == 0) { s3_exp(s_x, s_S); s3_inverse(s_S, s_Si); }  // S12 = exp(sim12) (:691), S21 (:703)
  __syncthreads();
  const double thres = huber * huber;                         // deltaHuber * deltaHuber (:701)
  int bad = 0;
  for (int i = tid; i < n; i += 256) {
    const int g = lo + i;
    const int o12 = s3_check_outlier(K1, s_S, P3D2c + 3 * (size_t)g, obs1[2 * (size_t)g], obs1[2 * (size_t)g + 1], w1[g], thres);
    const int o21 = s3_check_outlier(K2, s_Si, P3D1c + 3 * (size_t)g, obs2[2 * (size_t)g], obs2[2 * (size_t)g + 1], w2[g], thres);
    if (outlier) outlier[g] = (uint8_t)(o12 | o21);
    bad += (o12 | o21);
  }
  if (bad) atomicAdd(&s_nbad, bad);
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < 7; k++) s12s[7 * p + k] = s_S[k];
    const int good = n - s_nbad;
    n_inliers[p] = good < 10 ? 0 : good;                      // :731
    if (summaries) {
      ba_summary s;
      s.initial_cost = s_init; s.final_cost = s_xcost; s.iterations = s_iter; s.successful_steps = s_succ;
      s.termination = s_term; s.final_radius = s_radius;
      summaries[p] = s;
    }
  }
}
