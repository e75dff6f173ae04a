// OptimizeEssentialGraph and the batch bookkeeping kernels - part of the translation unit ba_solver.hip (textually included there; not compiled on its own).
// k_pg_*, k_ba_init, k_ba_collect.

// ============================================================================ OptimizeEssentialGraph (pose graph over Sim(3))
// CeresOptimizer::OptimizeEssentialGraph (src/CeresOptimizer.cc:737-957): vertices = Sim(3) tangents under
// Sim3Parameterization, edges = EssentialGraphErrorTerm (include/CeresOptimizer.h:266-330).  The LM controller, the dense
// Cholesky (k_chol_*) and the step logic (k_ba_iter_begin / k_ba_iter_end) are the bundle-adjustment ones, driven through a
// BaDev "view" that only carries S / rhs / Dinv / npad / part / state; the kernels below are the graph-specific parts.
// ---- start of a solve: the LM state, zeroed rhs / partial sums of every problem in ONE launch (a 64-problem batch issued 64
// state copies and 128 fills), and its end: state, poses, points and erase flags of every problem gathered into one block for
// ONE download (192 - 256 copies before) - a batched solve spent 9 % of its GPU time in 4-us copy kernels.
__device__ __forceinline__ size_t out_align(size_t b) { return (b + 255) & ~(size_t)255; }
__global__ __launch_bounds__(256) void k_ba_init(const BaDev* __restrict__ Dv, BaState st0) {
  const BaDev D = Dv[blockIdx.y];
  const int n = gridDim.x * 256, i0 = blockIdx.x * 256 + threadIdx.x;
  for (int i = i0; i < D.npad; i += n) D.rhs[i] = 0.0;
  for (int i = i0; i < 6 * D.nparts; i += n) D.part[i] = 0.0;
  if (D.pt_in_eval && !D.fix_points) {                        // (k_ba_eval<0> writes the blocks of the landmarks that have observations; the others read as zero, as the separate pass left them)
    for (int i = i0; i < 6 * D.npts; i += n) D.C[i] = 0.0;
    for (int i = i0; i < 3 * D.npts; i += n) D.gp[i] = 0.0;
  }
  if (i0 == 0) { *D.st = st0; if (D.ae_ticket) *D.ae_ticket = 0u; }
}
__global__ __launch_bounds__(256) void k_ba_collect(const BaDev* __restrict__ Dv, int with_erase) {
  const BaDev D = Dv[blockIdx.y];
  const int n = gridDim.x * 256, i0 = blockIdx.x * 256 + threadIdx.x;
  unsigned char* o = D.out;
  if (i0 < (int)(sizeof(BaState) / 4)) ((int*)o)[i0] = ((const int*)D.st)[i0];
  o += out_align(sizeof(BaState));
  double* op = (double*)o;
  for (int i = i0; i < 7 * D.ncam; i += n) op[i] = D.poses[i];
  o += out_align(7 * (size_t)D.ncam * sizeof(double));
  double* ox = (double*)o;
  for (int i = i0; i < 3 * D.npts; i += n) ox[i] = D.pts[i];
  o += out_align(3 * (size_t)D.npts * sizeof(double));
  if (with_erase && D.erase) for (int i = i0; i < D.nobs; i += n) o[i] = D.erase[i];
}

struct PgDev {
  int n, nf, n7, npad, ne, nblk, nparts;
  double* x; double* cand; const int* col;                 // [n][7] tangents, reduced column of every vertex (-1 = constant)
  const int* ej; const int* ei; const double* Sji;          // edges: vertex j, vertex i, measurement (qt7)
  double* r; double* J;                                     // [ne][7], [ne][49] (J_i; J_j = -J_i)
  double* g; double* scale;                                 // [n7] gradient (unscaled), Jacobi scaling
  const int* v_off; const int* v_edge; const signed char* v_sign;   // per vertex: incident edges in insertion order, +1 = it is i, -1 = it is j
  const int* blk_a; const int* blk_b; const int* blk_off; const int* blk_edge;    // off-diagonal blocks (col_a > col_b) and their edges
  double* vpart;                                            // per vertex: |x|^2, gmax
  double* S; double* rhs; double* part; BaState* st;
};

// residuals (+ Jacobians) of every edge: mode 0 at x, mode 1 cost only at the candidate
__global__ __launch_bounds__(128) void k_pg_eval(PgDev P, int mode) {
  __shared__ double s_red[4], s_out[1];
  const BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done) return;
  if (mode == 0 && !F.need_eval) return;
  if (mode == 1 && !F.valid) return;
  const int e = blockIdx.x * 128 + threadIdx.x;
  double acc = 0.0;
  if (e < P.ne) {
    const double* X = mode ? P.cand : P.x;
    double r[7];
    s3_graph_edge(X + 7 * (size_t)P.ej[e], X + 7 * (size_t)P.ei[e], P.Sji + 7 * (size_t)e, r, mode == 0 ? P.J + 49 * (size_t)e : nullptr);
#pragma unroll
    for (int k = 0; k < 7; k++) acc += 0.5 * r[k] * r[k];
    if (mode == 0)
#pragma unroll
      for (int k = 0; k < 7; k++) P.r[7 * (size_t)e + k] = r[k];
  }
  // 128-thread block sum (2 waves)
  double v = acc;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) { s_out[0] = s_red[0] + s_red[1]; P.part[(mode ? 1 : 0) * P.nparts + blockIdx.x] = s_out[0]; }
}

// per free vertex (thread): gradient, (first time) Jacobi scale, |x|^2 and its gradient-max-norm term
__global__ __launch_bounds__(128) void k_pg_vertex(PgDev P) {
  const BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.need_eval) return;
  const int v = blockIdx.x * 128 + threadIdx.x;
  if (v >= P.n) return;
  const int c = P.col[v];
  if (c < 0) { P.vpart[2 * v] = 0.0; P.vpart[2 * v + 1] = 0.0; return; }
  double g[7] = {0, 0, 0, 0, 0, 0, 0}, n2[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int q = P.v_off[v]; q < P.v_off[v + 1]; q++) {
    const int e = P.v_edge[q];
    const double sgn = (double)P.v_sign[q];
    const double* J = P.J + 49 * (size_t)e; const double* r = P.r + 7 * (size_t)e;
    for (int a = 0; a < 7; a++) {
      double s = 0, m = 0;
      for (int k = 0; k < 7; k++) { s += J[k * 7 + a] * r[k]; m += J[k * 7 + a] * J[k * 7 + a]; }
      g[a] += sgn * s; n2[a] += m;
    }
  }
  double xn = 0, mg[7], xp[7], gmax = 0;
  for (int a = 0; a < 7; a++) {
    P.g[7 * c + a] = g[a];
    if (st->first) P.scale[7 * c + a] = 1.0 / (1.0 + sqrt(n2[a]));
    const double xv = P.x[7 * (size_t)v + a];
    xn += xv * xv; mg[a] = -g[a];
  }
  s3_plus(P.x + 7 * (size_t)v, mg, xp);
  for (int a = 0; a < 7; a++) gmax = fmax(gmax, fabs(P.x[7 * (size_t)v + a] - xp[a]));
  P.vpart[2 * v] = xn; P.vpart[2 * v + 1] = gmax;
}

__global__ __launch_bounds__(256) void k_pg_after_eval(PgDev P) {
  __shared__ double s_red[4 * 2], s_out[2], s_max[4];
  BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.need_eval) return;
  const int tid = threadIdx.x;
  double acc[2] = {0.0, 0.0};
  double m = 0.0;
  for (int b = tid; b < P.nparts; b += 256) acc[0] += P.part[b];
  for (int v = tid; v < P.n; v += 256) { acc[1] += P.vpart[2 * v]; m = fmax(m, P.vpart[2 * v + 1]); }
  for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
  block_reduce<2>(acc, s_red, s_out);
  if (tid == 0) {
    st->x_cost = s_out[0]; st->x_norm = sqrt(s_out[1]);
    st->gmax = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
    if (st->first) st->initial_cost = s_out[0];
    st->first = 0; st->need_eval = 0;
    if (st->gmax <= 1e-10) { st->termination = 1; st->done = 1; }
  }
}

// scaled normal equations into the dense lower triangle: one 64-thread workgroup per diagonal block (free vertex) and per
// off-diagonal block; every block sums its edges in list order (deterministic), element (u, v) per lane
__global__ __launch_bounds__(64) void k_pg_build(PgDev P) {
  const BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.valid) return;
  const int np = P.npad, tid = threadIdx.x;
  const int u = tid / 7, w = tid - 7 * u;
  if ((int)blockIdx.x < P.n) {                         // diagonal block + rhs of vertex v
    const int v = blockIdx.x, c = P.col[v];
    if (c < 0) return;
    if (tid < 49) {
      double acc = 0.0;
      for (int q = P.v_off[v]; q < P.v_off[v + 1]; q++) {
        const double* J = P.J + 49 * (size_t)P.v_edge[q];
        double s = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) s += J[k * 7 + u] * J[k * 7 + w];
        acc += s;
      }
      double hs = acc * P.scale[7 * c + u] * P.scale[7 * c + w];
      if (u == w) hs += fmin(fmax(hs, 1e-6), 1e32) / st->radius;
      if (w <= u) P.S[(size_t)(7 * c + u) * np + 7 * c + w] = hs;
    }
    if (tid < 7) {
      const double gs = P.g[7 * c + tid] * P.scale[7 * c + tid];
      P.rhs[7 * c + tid] = gs;
      P.S[(size_t)np * np + 7 * c + tid] = gs;           // augmented row: forward substitution rides the factorisation
    }
  } else {                                              // off-diagonal block (a, b), col_a > col_b:  - sum_e J_e^T J_e
    const int blk = blockIdx.x - P.n;
    if (blk >= P.nblk || tid >= 49) return;
    const int ca = P.blk_a[blk], cb = P.blk_b[blk];
    double acc = 0.0;
    for (int q = P.blk_off[blk]; q < P.blk_off[blk + 1]; q++) {
      const double* J = P.J + 49 * (size_t)P.blk_edge[q];
      double s = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) s += J[k * 7 + u] * J[k * 7 + w];
      acc += s;
    }
    P.S[(size_t)(7 * ca + u) * np + 7 * cb + w] = -acc * P.scale[7 * ca + u] * P.scale[7 * cb + w];
  }
}

// padding rows (identity) of the reduced system, written once per solve
__global__ void k_pg_pad(PgDev P) {
  const int np = P.npad, i = P.n7 + blockIdx.x;
  if (i >= np) return;
  for (int j = threadIdx.x; j < np; j += blockDim.x) P.S[(size_t)i * np + j] = (i == j) ? 1.0 : 0.0;
  if (threadIdx.x == 0) { P.rhs[i] = 0.0; P.S[(size_t)np * np + i] = 0.0; }
}

// candidate x+ = Plus(x, -y * scale) per vertex, partial |dx|^2 -> part[2 * nparts + block]
__global__ __launch_bounds__(128) void k_pg_step(PgDev P) {
  __shared__ double s_red[2];
  const BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.valid) return;
  const int v = blockIdx.x * 128 + threadIdx.x;
  double acc = 0.0;
  if (v < P.n) {
    const int c = P.col[v];
    const double* x = P.x + 7 * (size_t)v; double* xc = P.cand + 7 * (size_t)v;
    if (c < 0 || st->chol_fail) { for (int k = 0; k < 7; k++) xc[k] = x[k]; }
    else {
      double d[7];
      for (int k = 0; k < 7; k++) d[k] = (-P.rhs[7 * c + k]) * P.scale[7 * c + k];
      s3_plus(x, d, xc);
      for (int k = 0; k < 7; k++) { const double e = x[k] - xc[k]; acc += e * e; }
    }
  }
  double vv = acc;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) vv += __shfl_xor(vv, o);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = vv;
  __syncthreads();
  if (threadIdx.x == 0) P.part[2 * P.nparts + blockIdx.x] = s_red[0] + s_red[1];
}

// model cost change -(J s).(r + J s / 2) per edge -> part[3 * nparts + block]; part[4 * nparts + block] = 0
__global__ __launch_bounds__(128) void k_pg_mcc(PgDev P) {
  __shared__ double s_red[2];
  const BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.valid) return;
  const int e = blockIdx.x * 128 + threadIdx.x;
  double acc = 0.0;
  if (e < P.ne && !st->chol_fail) {
    const int ci = P.col[P.ei[e]], cj = P.col[P.ej[e]];
    double d[7];
    for (int a = 0; a < 7; a++) {
      double di = 0, dj = 0;
      if (ci >= 0) di = (-P.rhs[7 * ci + a]) * P.scale[7 * ci + a];
      if (cj >= 0) dj = (-P.rhs[7 * cj + a]) * P.scale[7 * cj + a];
      d[a] = di - dj;
    }
    const double* J = P.J + 49 * (size_t)e; const double* r = P.r + 7 * (size_t)e;
    for (int k = 0; k < 7; k++) {
      double m = 0;
      for (int a = 0; a < 7; a++) m += J[k * 7 + a] * d[a];
      acc -= m * (r[k] + m / 2);
    }
  }
  double vv = acc;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) vv += __shfl_xor(vv, o);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = vv;
  __syncthreads();
  if (threadIdx.x == 0) { P.part[3 * P.nparts + blockIdx.x] = s_red[0] + s_red[1]; P.part[4 * P.nparts + blockIdx.x] = 0.0; }
}

__global__ __launch_bounds__(256) void k_pg_apply(PgDev P) {
  const BaState* st = P.st;
  const StFlags F = ld_flags(st);
  if (F.done || !F.accepted) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 7 * P.n) P.x[i] = P.cand[i];
}

// write-back arithmetic (src/CeresOptimizer.cc:916-956): Tiw = [R | t / s] per keyframe; P' = Swr_corrected * (Srw_original * P)
__global__ __launch_bounds__(128) void k_pg_poses(const double* __restrict__ lie_opt, int n, double* __restrict__ Tiw) {
  const int v = blockIdx.x * 128 + threadIdx.x;
  if (v >= n) return;
  double S[7];
  s3_exp(lie_opt + 7 * (size_t)v, S);
  double T[12];
  s3_to_pose34(S, T);
  for (int i = 0; i < 12; i++) Tiw[12 * (size_t)v + i] = T[i];
}
__global__ __launch_bounds__(256) void k_pg_points(const double* __restrict__ lie_orig, const double* __restrict__ lie_opt,
                                                   const int* __restrict__ pt_ref, double* __restrict__ pts, int npts) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const int rk = pt_ref[p];
  double S0[7], S1[7], S1i[7], Pc[3], Pw[3];
  s3_exp(lie_orig + 7 * (size_t)rk, S0);
  s3_exp(lie_opt + 7 * (size_t)rk, S1);
  s3_inverse(S1, S1i);
  s3_act(S0, pts + 3 * (size_t)p, Pc);
  s3_act(S1i, Pc, Pw);
  pts[3 * (size_t)p] = Pw[0]; pts[3 * (size_t)p + 1] = Pw[1]; pts[3 * (size_t)p + 2] = Pw[2];
}
