// ============================================================================
// orb_kfdb.inc -- KeyFrameDatabase on the device (reference src/KeyFrameDatabase.cc, all of it; DESIGN.md section 2 "KeyFrameDatabase",
// section 4 "orb_kfdb"): DetectLoopCandidates / DetectRelocalizationCandidates as a SCAN of every stored BowVector against the
// query instead of the CPU's inverted file - the inverted file exists to avoid the scan, and the scan is a streaming read.
// Textually included by orb_vocab.hip.
//
// Resident per slot (= keyframe): its BowVector (ascending words, double values) in a growing arena, the `add` sequence number
// (0 = not in the database), reloc_query / reloc_score (the two fields of the reference's KeyFrame that carry state from one
// relocalisation query to the next) and up to 10 best covisible slots.
//
//   k_kfdb_scan     one wave per (slot, query), the query's words in LDS (up to KFDB_LDS_WORDS; a longer query is searched
//                   in global memory): lanes take the slot's words and binary-search the query.  Per pair: common-word count and
//                   smallest common word (0 for a slot connected to a loop query: the reference neither stamps nor lists it);
//                   per query the maximum count and the sharing-list length (one atomic per wave).
//   k_kfdb_pick     minCommonWords = int(maxCommonWords * 0.8f); the pairs above it, as an unordered list.
//   k_kfdb_score    one wave per listed pair: L1Scoring::score - the common terms found 64 words at a time (ascending) and added in lane
//                   order, so the double sum is the reference's sum and its float is the same float.
//   per query, in stream order (the relocalisation state makes query q+1 depend on query q):
//   k_kfdb_state    relocalisation: reloc_query of every sharing slot, reloc_score of every scored slot.
//   k_kfdb_rank     the kept pairs (loop: score >= minScore) ranked by (smallest common word, sequence number) = the reference's
//                   first-touch order, by counting smaller keys.
//   k_kfdb_accum    per kept pair the float adds over its neighbours in neighbour order, best neighbour on a strict '>'.
//   k_kfdb_select   best accumulated score, 0.75f threshold (strict '>'), duplicates dropped (first kept), ordered compaction.
// ============================================================================

namespace orbhip {

constexpr int KFDB_LDS_WORDS = 4096;        // query words held in LDS by k_kfdb_scan (16 KB); longer queries are searched in global memory
constexpr int KFDB_WAVE_SLOTS = 8;          // slots per wave of k_kfdb_scan (32 per block: the query tile is loaded once per 32 slots)
constexpr int KFDB_MAX_NEIGH = 10;
constexpr int KFDB_LOOP = 0, KFDB_RELOC = 1;

struct KfSlot { long long off; int n; uint32_t seq; };                  // seq == 0: not in the database
struct KfState { long long reloc_query; float reloc_score; int pad; };
struct KfNeigh { int n; int s[11]; };

// lower-bound search of w in the ascending q[0 .. n); position or -1
__device__ __forceinline__ int kfdb_find(const uint32_t* q, int n, uint32_t w) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (q[mid] < w) lo = mid + 1; else hi = mid; }
  return (lo < n && q[lo] == w) ? lo : -1;
}

__device__ __forceinline__ void kfdb_scan_slots(const uint32_t* qw, int nq, const KfSlot* __restrict__ slots, int S, const uint32_t* __restrict__ aw,
                                                const int* __restrict__ conn, int nconn, int* __restrict__ count, uint32_t* __restrict__ minw,
                                                orbv_db_query_info* info) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int wmax = 0, wshare = 0;
  for (int k = 0; k < KFDB_WAVE_SLOTS; k++) {
    const int slot = (blockIdx.x * 4 + wv) * KFDB_WAVE_SLOTS + k;
    if (slot >= S) break;
    const KfSlot sl = slots[slot];
    int cnt = 0; uint32_t mw = 0xFFFFFFFFu;
    if (sl.seq != 0) {
      bool con = false;
      for (int i = lane; i < nconn; i += 64) con |= conn[i] == slot;
      if (!__any(con)) {
        for (int i = lane; i < sl.n; i += 64) {
          const uint32_t w = aw[sl.off + i];
          if (kfdb_find(qw, nq, w) >= 0) { cnt++; mw = min(mw, w); }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { cnt += __shfl_xor(cnt, o); mw = min(mw, (uint32_t)__shfl_xor((int)mw, o)); }
      }
    }
    if (lane == 0) { count[slot] = cnt; minw[slot] = mw; }
    wmax = max(wmax, cnt); wshare += cnt > 0;
  }
  if (lane == 0 && wshare) { atomicMax(&info->max_common, wmax); atomicAdd(&info->n_sharing, wshare); }
}

__global__ __launch_bounds__(256) void k_kfdb_scan(const KfSlot* __restrict__ slots, int S, const uint32_t* __restrict__ aw, const int* __restrict__ q_off,
                                                   const uint32_t* __restrict__ q_words, const int* __restrict__ conn_off, const int* __restrict__ conn,
                                                   int* __restrict__ count, uint32_t* __restrict__ minw, orbv_db_query_info* __restrict__ info) {
  __shared__ uint32_t lq[KFDB_LDS_WORDS];
  const int q = blockIdx.y;
  const int q0 = q_off[q], nq = q_off[q + 1] - q0;
  const uint32_t* gq = q_words + q0;
  const int c0 = conn_off ? conn_off[q] : 0, nconn = conn_off ? conn_off[q + 1] - c0 : 0;
  int* cq = count + (size_t)q * S; uint32_t* mq = minw + (size_t)q * S;
  if (nq <= KFDB_LDS_WORDS) {                                             // (uniform over the block)
    for (int i = threadIdx.x; i < nq; i += 256) lq[i] = gq[i];
    __syncthreads();
    kfdb_scan_slots(lq, nq, slots, S, aw, conn + c0, nconn, cq, mq, info + q);
  } else {
    kfdb_scan_slots(gq, nq, slots, S, aw, conn + c0, nconn, cq, mq, info + q);
  }
}

__global__ __launch_bounds__(256) void k_kfdb_pick(int S, const int* __restrict__ count, orbv_db_query_info* info, int* __restrict__ scored) {
  const int q = blockIdx.y, slot = blockIdx.x * 256 + threadIdx.x;
  const int minc = (int)((float)info[q].max_common * 0.8f);              // int minCommonWords = maxCommonWords * 0.8f (:118, :241)
  if (slot == 0) info[q].min_common = minc;
  if (slot < S && count[(size_t)q * S + slot] > minc) scored[(size_t)q * S + atomicAdd(&info[q].n_scored, 1)] = slot;
}

// L1Scoring::score(query, keyframe) by one wave: every lane returns the same double
__device__ __forceinline__ double kfdb_score_wave(const uint32_t* __restrict__ qw, const double* __restrict__ qv, int nq, const uint32_t* __restrict__ sw,
                                                  const double* __restrict__ sv, int ns, int lane) {
  double s = 0.0;
  for (int base = 0; base < ns; base += 64) {
    const int i = base + lane;
    double term = 0.0; bool hit = false;
    if (i < ns) {
      const int p = kfdb_find(qw, nq, sw[i]);
      if (p >= 0) { const double vi = qv[p], wi = sv[i]; term = fabs(vi - wi) - fabs(vi) - fabs(wi); hit = true; }
    }
    unsigned long long m = __ballot(hit);
    while (m) { const int l = __ffsll((long long)m) - 1; s += __shfl(term, l); m &= m - 1; }      // ascending word id, as the reference's merge
  }
  return -s / 2.0;
}

__global__ __launch_bounds__(256) void k_kfdb_score(const KfSlot* __restrict__ slots, int S, const uint32_t* __restrict__ aw, const double* __restrict__ av,
                                                    const int* __restrict__ q_off, const uint32_t* __restrict__ q_words, const double* __restrict__ q_values,
                                                    const orbv_db_query_info* __restrict__ info, const int* __restrict__ scored, float* __restrict__ score) {
  const int q = blockIdx.y, lane = threadIdx.x & 63;
  const int q0 = q_off[q], nq = q_off[q + 1] - q0, ns = info[q].n_scored;
  for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < ns; p += gridDim.x * 4) {
    const int slot = scored[(size_t)q * S + p];
    const KfSlot sl = slots[slot];
    const double s = kfdb_score_wave(q_words + q0, q_values + q0, nq, aw + sl.off, av + sl.off, sl.n, lane);
    if (lane == 0) score[(size_t)q * S + slot] = (float)s;
  }
}

// orbv_db_min_score: the query against n listed slots, one wave each
__global__ __launch_bounds__(256) void k_kfdb_score_list(const KfSlot* __restrict__ slots, const uint32_t* __restrict__ aw, const double* __restrict__ av,
                                                         const uint32_t* __restrict__ qw, const double* __restrict__ qv, int nq, const int* __restrict__ list, int n,
                                                         float* __restrict__ out) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= n) return;
  const KfSlot sl = slots[list[p]];
  const double s = kfdb_score_wave(qw, qv, nq, aw + sl.off, av + sl.off, sl.n, lane);
  if (lane == 0) out[p] = (float)s;
}

__global__ __launch_bounds__(256) void k_kfdb_state(int S, const int* __restrict__ count, const float* __restrict__ score, const orbv_db_query_info* __restrict__ info,
                                                    long long qid, KfState* __restrict__ st) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= S) return;
  const int c = count[slot];
  if (c > 0) { st[slot].reloc_query = qid; if (c > info->min_common) st[slot].reloc_score = score[slot]; }
}

__global__ __launch_bounds__(256) void k_kfdb_rank(const KfSlot* __restrict__ slots, const uint32_t* __restrict__ minw, const float* __restrict__ score,
                                                   const int* __restrict__ scored, orbv_db_query_info* __restrict__ info, int kind, const float* __restrict__ min_score,
                                                   int* __restrict__ ord_slot, float* __restrict__ ord_score) {
  const int ns = info->n_scored;
  const float ms = kind == KFDB_LOOP ? *min_score : 0.0f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < ns; p += gridDim.x * 256) {
    const int slot = scored[p];
    const float sc = score[slot];
    if (kind == KFDB_LOOP && !(sc >= ms)) continue;                      // if (score >= minScore) (:136); relocalisation keeps every scored one
    const unsigned long long key = ((unsigned long long)minw[slot] << 32) | slots[slot].seq;
    int rank = 0;
    for (int j = 0; j < ns; j++) {
      const int sj = scored[j];
      if (kind == KFDB_LOOP && !(score[sj] >= ms)) continue;
      rank += ((((unsigned long long)minw[sj] << 32) | slots[sj].seq) < key);
    }
    ord_slot[rank] = slot; ord_score[rank] = sc;
    atomicAdd(&info->n_kept, 1);
  }
}

// rows == NULL: the resident neighbour table; else rows[r][10] / row_n[r] per kept pair, as the caller's GetBestCovisibilityKeyFrames(10) gave them
__global__ __launch_bounds__(256) void k_kfdb_accum(const KfSlot* __restrict__ slots, int S, int S_query, const KfNeigh* __restrict__ neigh, const int* __restrict__ rows,
                                                    const int* __restrict__ row_n, const int* __restrict__ count, const float* __restrict__ score,
                                                    const KfState* __restrict__ st, const orbv_db_query_info* __restrict__ info, int kind, long long qid,
                                                    const int* __restrict__ ord_slot, const float* __restrict__ ord_score, float* __restrict__ acc, int* __restrict__ best) {
  const int k = info->n_kept, minc = info->min_common;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < k; r += gridDim.x * 256) {
    const int slot = ord_slot[r];
    const int* row = rows ? rows + (size_t)r * KFDB_MAX_NEIGH : neigh[slot].s;
    const int nn = min(rows ? row_n[r] : neigh[slot].n, KFDB_MAX_NEIGH);
    float best_score = ord_score[r], a = best_score;
    int b = slot;
    for (int i = 0; i < nn; i++) {
      const int j = row[i];
      if (j < 0 || j >= S || slots[j].seq == 0) continue;               // a neighbour that is not in the database contributes nothing
      float sj;
      if (kind == KFDB_LOOP) { if (j >= S_query || !(count[j] > minc)) continue; sj = score[j]; }      // stamped by this query and above minCommonWords (:163-164)
      else { if (st[j].reloc_query != qid) continue; sj = st[j].reloc_score; }                         // merely stamped (:282): the score may be an earlier query's
      a += sj;
      if (sj > best_score) { b = j; best_score = sj; }
    }
    acc[r] = a; best[r] = b;
  }
}

__global__ __launch_bounds__(1024) void k_kfdb_select(orbv_db_query_info* __restrict__ info, int kind, const float* __restrict__ min_score, const float* __restrict__ acc,
                                                      const int* __restrict__ best, int* __restrict__ flag, int cap, int* __restrict__ cand) {
  __shared__ float red[16];
  __shared__ int wsum[16];
  const int k = info->n_kept, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (k == 0) return;                                                     // (n_cand, best_acc stay 0)
  float m = kind == KFDB_LOOP ? *min_score : 0.0f;                        // bestAccScore = minScore (:146) / 0 (:267)
  for (int r = tid; r < k; r += 1024) if (acc[r] > m) m = acc[r];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const float x = __shfl_xor(m, o); if (x > m) m = x; }
  if (lane == 0) red[wv] = m;
  __syncthreads();
  for (int i = 0; i < 16; i++) if (red[i] > m) m = red[i];
  const float thr = 0.75f * m;                                            // minScoreToRetain
  for (int r = tid; r < k; r += 1024) {
    int f = acc[r] > thr;
    if (f) { const int b = best[r]; for (int j = 0; j < r; j++) if (best[j] == b && acc[j] > thr) { f = 0; break; } }
    flag[r] = f;
  }
  __syncthreads();
  // ordered compaction, twice: the first pass counts, so that a result beyond `cap` writes nothing
  for (int pass = 0; pass < 2; pass++) {
    int base = 0;
    for (int c0 = 0; c0 < k; c0 += 1024) {
      const int r = c0 + tid;
      const int f = r < k ? flag[r] : 0;
      const unsigned long long bm = __ballot(f);
      if (lane == 0) wsum[wv] = __popcll(bm);
      __syncthreads();
      int off = 0, tot = 0;
      for (int i = 0; i < 16; i++) { if (i < wv) off += wsum[i]; tot += wsum[i]; }
      if (pass && f) cand[base + off + __popcll(bm & ((1ull << lane) - 1ull))] = best[r];
      base += tot;
      __syncthreads();
    }
    if (pass == 0) {
      if (tid == 0) { info->n_cand = base; info->best_acc = m; info->status = base > cap ? ORBHIP_ECAP : 0; }
      if (base > cap) return;
    }
  }
}

// arena compaction: the live slots' BowVectors copied to their new offsets, one block per slot
__global__ __launch_bounds__(256) void k_kfdb_compact(const KfSlot* __restrict__ old_slots, const KfSlot* __restrict__ new_slots, const uint32_t* __restrict__ ow,
                                                      const double* __restrict__ ov, uint32_t* __restrict__ nw, double* __restrict__ nv) {
  const KfSlot a = old_slots[blockIdx.x], b = new_slots[blockIdx.x];
  if (b.seq == 0) return;
  for (int i = threadIdx.x; i < b.n; i += 256) { nw[b.off + i] = ow[a.off + i]; nv[b.off + i] = ov[a.off + i]; }
}

}  // namespace orbhip

struct orbv_db {
  int device = 0, n_words = 0;
  bool dev_ready = false;
  hipStream_t s = nullptr;
  // host bookkeeping (slot = the caller's keyframe index)
  std::vector<orbhip::KfSlot> slots;                 // [S], S = highest slot touched + 1
  int n_live = 0; uint32_t next_seq = 1;
  long long arena_used = 0, arena_dead = 0, arena_cap = 0;
  int64_t last_query[2] = {0, 0};
  // device
  int cap_slots = 0;
  orbhip::DevBuf d_slots, d_state, d_neigh, d_aw, d_av, ws, qin;
  orbhip::PinnedHost hin, hout;
  // a query between begin and finish
  int pend_kind = -1, pend_S = 0; int64_t pend_qid = 0; int pend_kept = 0; float pend_min_score = 0.0f;
};

namespace orbhip {

struct KfdbLayout {
  size_t count, minw, score, scored, ord_slot, ord_score, acc, best, flag, info, total;     // (info: the host entries' own orbv_db_query_info)
  KfdbLayout(int S, int Q) {
    const size_t pair = align256((size_t)S * Q * 4), one = align256((size_t)S * 4);
    size_t o = 0;
    count = o; o += pair; minw = o; o += pair; score = o; o += pair; scored = o; o += pair;
    ord_slot = o; o += one; ord_score = o; o += one; acc = o; o += one; best = o; o += one; flag = o; o += one;
    info = o; total = o + 256;
  }
};

static int kfdb_device(orbv_db* c) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (the HIP path has no CPU fallback)"); return ORBHIP_ENODEV; }
  ORBHIP_REQUIRE(c->device < ndev, ORBHIP_EINVAL, "bad device index");
  VCHK(hipSetDevice(c->device));
  if (!c->dev_ready) {
    VCHK(hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking));
    c->dev_ready = true;
  }
  return 0;
}

// buffer grown to `need` bytes with its first `keep` bytes preserved and the rest zeroed
static int kfdb_grow(orbv_db* c, DevBuf& b, size_t keep, size_t need) {
  if (need <= b.bytes) return 0;
  DevBuf nb;
  if (int rc = nb.ensure(std::max(need, b.bytes * 2))) return rc;
  hipError_t e = hipMemsetAsync(nb.p, 0, nb.bytes, c->s);
  if (e == hipSuccess && keep) e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->s);
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e != hipSuccess) { nb.release(); set_error("keyframe database: growing a device table failed: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  b.release(); b = nb;
  return 0;
}

static int kfdb_reserve_slots(orbv_db* c, int S) {
  if (S > (int)c->slots.size()) c->slots.resize(S, KfSlot{0, 0, 0});
  if (S <= c->cap_slots) return 0;
  const int cap = std::max(S, std::max(1024, c->cap_slots * 2));
  int rc = 0;
  if ((rc = kfdb_grow(c, c->d_slots, (size_t)c->cap_slots * sizeof(KfSlot), (size_t)cap * sizeof(KfSlot))) ||
      (rc = kfdb_grow(c, c->d_state, (size_t)c->cap_slots * sizeof(KfState), (size_t)cap * sizeof(KfState))) ||
      (rc = kfdb_grow(c, c->d_neigh, (size_t)c->cap_slots * sizeof(KfNeigh), (size_t)cap * sizeof(KfNeigh)))) return rc;
  c->cap_slots = cap;
  return 0;
}

static int kfdb_put(orbv_db* c, void* dst, const void* src, size_t bytes) {      // small synchronous upload on the database's stream
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->s);
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e != hipSuccess) { set_error("keyframe database: upload failed: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  return 0;
}

// room for n more arena entries: erased space is reclaimed by compaction once it is more than half of what is used, else the arena grows
static int kfdb_arena_room(orbv_db* c, int n) {
  if (c->arena_used + n <= c->arena_cap) return 0;
  const int S = (int)c->slots.size();
  if (c->arena_dead * 2 > c->arena_used && S > 0) {
    std::vector<KfSlot> ns(c->slots);
    long long o = 0;
    for (KfSlot& s : ns) if (s.seq) { s.off = o; o += s.n; }
    const long long cap = std::max<long long>(c->arena_cap, o + n);
    DevBuf nw, nv, dns;
    int rc = 0;
    if ((rc = nw.ensure((size_t)cap * 4)) || (rc = nv.ensure((size_t)cap * 8)) || (rc = dns.ensure((size_t)S * sizeof(KfSlot))) ||
        (rc = kfdb_put(c, dns.p, ns.data(), (size_t)S * sizeof(KfSlot)))) { nw.release(); nv.release(); dns.release(); return rc; }
    hipLaunchKernelGGL(k_kfdb_compact, dim3(S), dim3(256), 0, c->s, c->d_slots.as<KfSlot>(), dns.as<KfSlot>(), c->d_aw.as<uint32_t>(), c->d_av.as<double>(),
                       nw.as<uint32_t>(), nv.as<double>());
    hipError_t e = hipMemcpyAsync(c->d_slots.p, dns.p, (size_t)S * sizeof(KfSlot), hipMemcpyDeviceToDevice, c->s);
    if (e == hipSuccess) e = hipStreamSynchronize(c->s);
    dns.release();
    if (e != hipSuccess) { nw.release(); nv.release(); set_error("keyframe database: arena compaction failed: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
    c->d_aw.release(); c->d_av.release(); c->d_aw = nw; c->d_av = nv;
    c->slots.swap(ns); c->arena_used = o; c->arena_dead = 0; c->arena_cap = cap;
    return 0;
  }
  const long long cap = std::max<long long>(c->arena_used + n, std::max<long long>(1 << 20, c->arena_cap * 2));
  int rc = 0;
  if ((rc = kfdb_grow(c, c->d_aw, (size_t)c->arena_used * 4, (size_t)cap * 4)) || (rc = kfdb_grow(c, c->d_av, (size_t)c->arena_used * 8, (size_t)cap * 8))) return rc;
  c->arena_cap = cap;
  return 0;
}

static int kfdb_check_bow(const orbv_db* c, const uint32_t* words, const double* values, int n) {
  ORBHIP_REQUIRE(n >= 0 && (n == 0 || (words && values)), ORBHIP_EINVAL, "NULL BowVector");
  for (int i = 0; i < n; i++) {
    ORBHIP_REQUIRE(words[i] < (uint32_t)c->n_words, ORBHIP_EINVAL, "word id not below n_words");
    ORBHIP_REQUIRE(i == 0 || words[i] > words[i - 1], ORBHIP_EINVAL, "word ids must ascend");
  }
  return 0;
}

// Q queries enqueued on `s`.  stage: 0 = everything, 1 = up to the ordered kept list (begin), 2 = from the kept list on (finish; Q == 1)
static int kfdb_enqueue(orbv_db* c, int kind, int Q, int stage, const int* q_off, const uint32_t* q_words, const double* q_values, const int* conn_off,
                        const int* conn, const float* min_score, int64_t first_qid, int S, const int* rows, const int* row_n, uint8_t* ws,
                        orbv_db_query_info* info, int* cand, int cap, hipStream_t s) {
  const KfdbLayout L(S, Q);
  int* count = (int*)(ws + L.count); uint32_t* minw = (uint32_t*)(ws + L.minw); float* score = (float*)(ws + L.score); int* scored = (int*)(ws + L.scored);
  int* ord_slot = (int*)(ws + L.ord_slot); float* ord_score = (float*)(ws + L.ord_score); float* acc = (float*)(ws + L.acc);
  int* best = (int*)(ws + L.best); int* flag = (int*)(ws + L.flag);
  const KfSlot* slots = c->d_slots.as<KfSlot>();
  if (stage != 2) {
    VCHK(hipMemsetAsync(info, 0, (size_t)Q * sizeof(orbv_db_query_info), s));
    if (S == 0) return 0;
    hipLaunchKernelGGL(k_kfdb_scan, dim3((S + 4 * KFDB_WAVE_SLOTS - 1) / (4 * KFDB_WAVE_SLOTS), Q), dim3(256), 0, s, slots, S, c->d_aw.as<uint32_t>(), q_off, q_words,
                       kind == KFDB_LOOP ? conn_off : nullptr, conn, count, minw, info);
    hipLaunchKernelGGL(k_kfdb_pick, dim3((S + 255) / 256, Q), dim3(256), 0, s, S, count, info, scored);
    hipLaunchKernelGGL(k_kfdb_score, dim3(std::min((S + 3) / 4, 256), Q), dim3(256), 0, s, slots, S, c->d_aw.as<uint32_t>(), c->d_av.as<double>(), q_off, q_words,
                       q_values, info, scored, score);
  }
  if (S == 0) return 0;
  const int g = std::min((S + 255) / 256, 64);
  for (int q = 0; q < Q; q++) {
    const size_t o = (size_t)q * S;
    const long long qid = first_qid + q;
    if (stage != 2) {
      if (kind == KFDB_RELOC) hipLaunchKernelGGL(k_kfdb_state, dim3((S + 255) / 256), dim3(256), 0, s, S, count + o, score + o, info + q, qid, c->d_state.as<KfState>());
      hipLaunchKernelGGL(k_kfdb_rank, dim3(g), dim3(256), 0, s, slots, minw + o, score + o, scored + o, info + q, kind, min_score ? min_score + q : nullptr, ord_slot,
                         ord_score);
    }
    if (stage != 1) {
      hipLaunchKernelGGL(k_kfdb_accum, dim3(g), dim3(256), 0, s, slots, (int)c->slots.size(), S, c->d_neigh.as<KfNeigh>(), rows, row_n, count + o, score + o,
                         c->d_state.as<KfState>(), info + q, kind, qid, ord_slot, ord_score, acc, best);
      hipLaunchKernelGGL(k_kfdb_select, dim3(1), dim3(1024), 0, s, info + q, kind, min_score ? min_score + q : nullptr, acc, best, flag, cap, cand + (size_t)q * cap);
    }
  }
  VCHK(hipGetLastError());
  return 0;
}

static int kfdb_take_id(orbv_db* c, int kind, int64_t first, int Q) {             // ids are consumed once the arguments have passed
  ORBHIP_REQUIRE(first > 0 && first > c->last_query[kind], ORBHIP_EINVAL, "query_id must be positive and greater than the last one of its kind");
  c->last_query[kind] = first + Q - 1;
  return 0;
}

struct KfdbStaged { int* q_off; uint32_t* q_words; double* q_values; int* conn_off; int* conn; float* min_score; int* rows; int* row_n; orbv_db_query_info* info; int* cand;
                    uint8_t* hout; size_t o_info, o_cand, o_slot, o_score, o_acc, o_best, out_bytes; int n_copy; };

// one host query: inputs staged through pinned memory in one copy, outputs brought back in one copy after the kernels
static int kfdb_host_query(orbv_db* c, int kind, int stage, const uint32_t* words, const double* values, int n, const int* conn, int n_conn, float min_score,
                           int64_t qid, const int* rows, const int* row_n, int n_rows, int cap, bool want_kept, KfdbStaged* st) {
  const int S = stage == 2 ? c->pend_S : (int)c->slots.size();
  const KfdbLayout L(S, 1);
  int rc = 0;
  if ((rc = c->ws.ensure(L.total))) return rc;
  Carve qb;                                                    // the query block: inputs, then the candidate list
  const size_t i_off = qb.take(8), i_w = qb.take((size_t)n * 4), i_v = qb.take((size_t)n * 8), i_coff = qb.take(8), i_conn = qb.take((size_t)n_conn * 4), i_ms = qb.take(4);
  const size_t i_rows = qb.take((size_t)n_rows * orbhip::KFDB_MAX_NEIGH * 4), i_rn = qb.take((size_t)n_rows * 4);
  const size_t in_bytes = qb.total;
  const int ncand = std::max(std::min(cap, S), 0), nkept = want_kept ? S : 0;
  st->o_cand = qb.take((size_t)std::max(ncand, 1) * 4);
  const size_t dev_total = qb.total;
  if ((rc = c->qin.ensure(dev_total)) || (rc = c->hin.ensure(in_bytes))) return rc;
  uint8_t* h = (uint8_t*)c->hin.p; uint8_t* d = c->qin.as<uint8_t>();
  const int qo[2] = {0, n}, co[2] = {0, n_conn};
  std::memcpy(h + i_off, qo, 8); std::memcpy(h + i_coff, co, 8); std::memcpy(h + i_ms, &min_score, 4);
  if (n) { std::memcpy(h + i_w, words, (size_t)n * 4); std::memcpy(h + i_v, values, (size_t)n * 8); }
  if (n_conn) std::memcpy(h + i_conn, conn, (size_t)n_conn * 4);
  if (n_rows) { std::memcpy(h + i_rows, rows, (size_t)n_rows * orbhip::KFDB_MAX_NEIGH * 4); std::memcpy(h + i_rn, row_n, (size_t)n_rows * 4); }
  if (ws_copy(d, h, in_bytes, hipMemcpyHostToDevice, c->s) != hipSuccess) { set_error("keyframe database: query upload failed"); return ORBHIP_ENODEV; }
  st->info = (orbv_db_query_info*)(c->ws.as<uint8_t>() + L.info); st->cand = (int*)(d + st->o_cand);
  if ((rc = kfdb_enqueue(c, kind, 1, stage, (int*)(d + i_off), (uint32_t*)(d + i_w), (double*)(d + i_v), (int*)(d + i_coff), (int*)(d + i_conn), (float*)(d + i_ms), qid, S,
                         n_rows || stage == 2 ? (int*)(d + i_rows) : nullptr, (int*)(d + i_rn), c->ws.as<uint8_t>(), st->info, st->cand, cap, c->s))) return rc;
  // outputs: info, candidates and (trace / begin) the kept list with its scores, one pinned block
  Carve hc;
  const size_t h_info = hc.take(sizeof(orbv_db_query_info)), h_cand = hc.take((size_t)ncand * 4), h_slot = hc.take((size_t)nkept * 4), h_score = hc.take((size_t)nkept * 4);
  const size_t h_acc = hc.take((size_t)nkept * 4), h_best = hc.take((size_t)nkept * 4);
  if ((rc = c->hout.ensure(hc.total))) return rc;
  uint8_t* hb = (uint8_t*)c->hout.p;
  hipError_t e = ws_copy(hb + h_info, st->info, sizeof(orbv_db_query_info), hipMemcpyDeviceToHost, c->s);
  if (e == hipSuccess && ncand && stage != 1) e = ws_copy(hb + h_cand, st->cand, (size_t)ncand * 4, hipMemcpyDeviceToHost, c->s);
  if (e == hipSuccess && nkept) {
    uint8_t* w = c->ws.as<uint8_t>();
    e = ws_copy(hb + h_slot, w + L.ord_slot, (size_t)nkept * 4, hipMemcpyDeviceToHost, c->s);
    if (e == hipSuccess) e = ws_copy(hb + h_score, w + L.ord_score, (size_t)nkept * 4, hipMemcpyDeviceToHost, c->s);
    if (e == hipSuccess && stage != 1) e = ws_copy(hb + h_acc, w + L.acc, (size_t)nkept * 4, hipMemcpyDeviceToHost, c->s);
    if (e == hipSuccess && stage != 1) e = ws_copy(hb + h_best, w + L.best, (size_t)nkept * 4, hipMemcpyDeviceToHost, c->s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_error("keyframe database query failed: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  st->hout = hb; st->o_info = h_info; st->o_cand = h_cand; st->o_slot = h_slot; st->o_score = h_score; st->o_acc = h_acc; st->o_best = h_best;
  return 0;
}

// results of a finished host query handed to the caller; nothing is written when anything does not fit
static int kfdb_deliver(const KfdbStaged& st, int32_t* cand, int cap, int32_t* n_cand, const orbv_db_trace* tr) {
  const orbv_db_query_info* info = (const orbv_db_query_info*)(st.hout + st.o_info);
  if (info->status == ORBHIP_ECAP || info->n_cand > cap) { set_error("keyframe database: %d candidates, capacity %d", info->n_cand, cap); return ORBHIP_ECAP; }
  if (tr && info->n_kept > tr->kept_cap) { set_error("keyframe database: %d kept keyframes, trace capacity %d", info->n_kept, tr->kept_cap); return ORBHIP_ECAP; }
  if (info->n_cand) std::memcpy(cand, st.hout + st.o_cand, (size_t)info->n_cand * 4);
  *n_cand = info->n_cand;
  if (tr) {
    if (tr->info) *tr->info = *info;
    const size_t b = (size_t)info->n_kept * 4;
    if (tr->kept_slot && b) std::memcpy(tr->kept_slot, st.hout + st.o_slot, b);
    if (tr->kept_score && b) std::memcpy(tr->kept_score, st.hout + st.o_score, b);
    if (tr->kept_acc && b) std::memcpy(tr->kept_acc, st.hout + st.o_acc, b);
    if (tr->kept_best && b) std::memcpy(tr->kept_best, st.hout + st.o_best, b);
  }
  return 0;
}

static int kfdb_detect(orbv_db* c, int kind, const uint32_t* words, const double* values, int n, const int32_t* conn, int n_conn, float min_score, int64_t qid,
                       int32_t* cand, int cap, int32_t* n_cand, const orbv_db_trace* tr) {
  ORBHIP_REQUIRE(c && n_cand && cap >= 0 && (cap == 0 || cand) && n_conn >= 0 && (n_conn == 0 || conn), ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(!tr || tr->kept_cap >= 0, ORBHIP_EINVAL, "bad trace capacity");
  if (int rc = kfdb_check_bow(c, words, values, n)) return rc;
  if (int rc = kfdb_take_id(c, kind, qid, 1)) return rc;
  if (int rc = kfdb_device(c)) return rc;
  c->pend_kind = -1;
  KfdbStaged st{};
  if (int rc = kfdb_host_query(c, kind, 0, words, values, n, conn, n_conn, min_score, qid, nullptr, nullptr, 0, cap, tr != nullptr, &st)) return rc;
  return kfdb_deliver(st, cand, cap, n_cand, tr);
}

static int kfdb_begin(orbv_db* c, int kind, const uint32_t* words, const double* values, int n, const int32_t* conn, int n_conn, float min_score, int64_t qid,
                      int32_t* kept, int kept_cap, int32_t* n_kept) {
  ORBHIP_REQUIRE(c && n_kept && kept_cap >= 0 && (kept_cap == 0 || kept) && n_conn >= 0 && (n_conn == 0 || conn), ORBHIP_EINVAL, "NULL argument");
  if (int rc = kfdb_check_bow(c, words, values, n)) return rc;
  if (int rc = kfdb_take_id(c, kind, qid, 1)) return rc;
  if (int rc = kfdb_device(c)) return rc;
  c->pend_kind = -1;
  KfdbStaged st{};
  if (int rc = kfdb_host_query(c, kind, 1, words, values, n, conn, n_conn, min_score, qid, nullptr, nullptr, 0, 0, true, &st)) return rc;
  const orbv_db_query_info* info = (const orbv_db_query_info*)(st.hout + st.o_info);
  if (info->n_kept > kept_cap) { set_error("keyframe database: %d kept keyframes, capacity %d", info->n_kept, kept_cap); return ORBHIP_ECAP; }
  if (info->n_kept) std::memcpy(kept, st.hout + st.o_slot, (size_t)info->n_kept * 4);
  *n_kept = info->n_kept;
  c->pend_kind = kind; c->pend_S = (int)c->slots.size(); c->pend_qid = qid; c->pend_kept = info->n_kept; c->pend_min_score = min_score;
  return 0;
}

}  // namespace orbhip

extern "C" {

int orbv_db_create(int n_words, int device, orbv_db** out) {
  ORBHIP_REQUIRE(out && n_words > 0 && device >= 0, ORBHIP_EINVAL, "bad argument");
  orbv_db* c = new orbv_db();
  c->n_words = n_words; c->device = device;
  *out = c;
  return 0;
}

int orbv_db_destroy(orbv_db* c) {
  if (!c) return 0;
  if (c->dev_ready) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->s); (void)hipStreamDestroy(c->s);
    c->d_slots.release(); c->d_state.release(); c->d_neigh.release(); c->d_aw.release(); c->d_av.release(); c->ws.release(); c->qin.release();
    if (c->hin.p) (void)hipHostFree(c->hin.p);
    if (c->hout.p) (void)hipHostFree(c->hout.p);
  }
  delete c;
  return 0;
}

int orbv_db_clear(orbv_db* c) {
  ORBHIP_REQUIRE(c, ORBHIP_EINVAL, "NULL argument");
  c->slots.clear(); c->n_live = 0; c->next_seq = 1; c->arena_used = c->arena_dead = 0; c->last_query[0] = c->last_query[1] = 0; c->pend_kind = -1;
  if (!c->dev_ready || c->cap_slots == 0) return 0;
  VCHK(hipSetDevice(c->device));
  hipError_t e = hipMemsetAsync(c->d_slots.p, 0, c->d_slots.bytes, c->s);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_state.p, 0, c->d_state.bytes, c->s);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_neigh.p, 0, c->d_neigh.bytes, c->s);
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e != hipSuccess) { set_error("orbv_db_clear: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  return 0;
}

int orbv_db_add(orbv_db* c, int slot, const uint32_t* words, const double* values, int n) {
  ORBHIP_REQUIRE(c && slot >= 0, ORBHIP_EINVAL, "bad argument");
  if (int rc = kfdb_check_bow(c, words, values, n)) return rc;
  ORBHIP_REQUIRE(slot >= (int)c->slots.size() || c->slots[slot].seq == 0, ORBHIP_EINVAL, "slot is already in the database");
  if (int rc = kfdb_device(c)) return rc;
  c->pend_kind = -1;
  if (int rc = kfdb_reserve_slots(c, slot + 1)) return rc;
  if (int rc = kfdb_arena_room(c, n)) return rc;
  const KfSlot s{c->arena_used, n, c->next_seq};
  if (n) {
    hipError_t e = hipMemcpyAsync(c->d_aw.as<uint32_t>() + s.off, words, (size_t)n * 4, hipMemcpyHostToDevice, c->s);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_av.as<double>() + s.off, values, (size_t)n * 8, hipMemcpyHostToDevice, c->s);
    if (e != hipSuccess) { set_error("orbv_db_add: upload failed: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  }
  if (int rc = kfdb_put(c, c->d_slots.as<KfSlot>() + slot, &s, sizeof s)) return rc;
  c->slots[slot] = s; c->arena_used += n; c->next_seq++; c->n_live++;
  return 0;
}

int orbv_db_erase(orbv_db* c, int slot) {
  ORBHIP_REQUIRE(c && slot >= 0, ORBHIP_EINVAL, "bad argument");
  if (slot >= (int)c->slots.size() || c->slots[slot].seq == 0) return 0;       // not in the database: nothing to do, as the reference
  if (int rc = kfdb_device(c)) return rc;
  c->pend_kind = -1;
  const KfSlot s{0, 0, 0};
  if (int rc = kfdb_put(c, c->d_slots.as<KfSlot>() + slot, &s, sizeof s)) return rc;
  c->arena_dead += c->slots[slot].n; c->slots[slot] = s; c->n_live--;
  return 0;
}

int orbv_db_size(const orbv_db* c) {
  ORBHIP_REQUIRE(c, ORBHIP_EINVAL, "NULL argument");
  return c->n_live;
}

int orbv_db_set_best_covisibles(orbv_db* c, int slot, const int32_t* neigh, int n) {
  ORBHIP_REQUIRE(c && slot >= 0 && n >= 0 && n <= KFDB_MAX_NEIGH && (n == 0 || neigh), ORBHIP_EINVAL, "bad argument (at most 10 neighbours)");
  for (int i = 0; i < n; i++) ORBHIP_REQUIRE(neigh[i] >= 0, ORBHIP_EINVAL, "negative neighbour slot");
  if (int rc = kfdb_device(c)) return rc;
  c->pend_kind = -1;
  if (int rc = kfdb_reserve_slots(c, slot + 1)) return rc;
  KfNeigh r{}; r.n = n;
  for (int i = 0; i < n; i++) r.s[i] = neigh[i];
  return kfdb_put(c, c->d_neigh.as<KfNeigh>() + slot, &r, sizeof r);
}

int orbv_db_get_state(orbv_db* c, const int32_t* slots, int n, int64_t* reloc_query, float* reloc_score) {
  ORBHIP_REQUIRE(c && n >= 0 && (n == 0 || (slots && reloc_query && reloc_score)), ORBHIP_EINVAL, "NULL argument");
  for (int i = 0; i < n; i++) ORBHIP_REQUIRE(slots[i] >= 0 && slots[i] < (int)c->slots.size(), ORBHIP_EINVAL, "slot out of range");
  if (n == 0) return 0;
  if (int rc = kfdb_device(c)) return rc;
  std::vector<KfState> st(c->slots.size());
  hipError_t e = hipMemcpyAsync(st.data(), c->d_state.p, st.size() * sizeof(KfState), hipMemcpyDeviceToHost, c->s);
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e != hipSuccess) { set_error("orbv_db_get_state: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  for (int i = 0; i < n; i++) { reloc_query[i] = st[slots[i]].reloc_query; reloc_score[i] = st[slots[i]].reloc_score; }
  return 0;
}

int orbv_db_min_score(orbv_db* c, const uint32_t* words, const double* values, int n, const int32_t* slots, int n_slots, float* min_score) {
  ORBHIP_REQUIRE(c && min_score && n_slots >= 0 && (n_slots == 0 || slots), ORBHIP_EINVAL, "NULL argument");
  if (int rc = kfdb_check_bow(c, words, values, n)) return rc;
  for (int i = 0; i < n_slots; i++)
    ORBHIP_REQUIRE(slots[i] >= 0 && slots[i] < (int)c->slots.size() && c->slots[slots[i]].seq != 0, ORBHIP_EINVAL, "slot is not in the database");
  if (n_slots == 0) { *min_score = 1.0f; return 0; }
  if (int rc = kfdb_device(c)) return rc;
  Carve qb;
  const size_t o_w = qb.take((size_t)n * 4), o_v = qb.take((size_t)n * 8), o_l = qb.take((size_t)n_slots * 4), in_bytes = qb.total, o_out = in_bytes;
  int rc = 0;
  if ((rc = c->qin.ensure(o_out + (size_t)n_slots * 4)) || (rc = c->hin.ensure(in_bytes)) || (rc = c->hout.ensure((size_t)n_slots * 4))) return rc;
  uint8_t* h = (uint8_t*)c->hin.p; uint8_t* d = c->qin.as<uint8_t>();
  if (n) { std::memcpy(h + o_w, words, (size_t)n * 4); std::memcpy(h + o_v, values, (size_t)n * 8); }
  std::memcpy(h + o_l, slots, (size_t)n_slots * 4);
  hipError_t e = ws_copy(d, h, in_bytes, hipMemcpyHostToDevice, c->s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_kfdb_score_list, dim3((n_slots + 3) / 4), dim3(256), 0, c->s, c->d_slots.as<KfSlot>(), c->d_aw.as<uint32_t>(), c->d_av.as<double>(),
                       (const uint32_t*)(d + o_w), (const double*)(d + o_v), n, (const int*)(d + o_l), n_slots, (float*)(d + o_out));
    e = ws_copy(c->hout.p, d + o_out, (size_t)n_slots * 4, hipMemcpyDeviceToHost, c->s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_error("orbv_db_min_score: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  float m = 1.0f;                                                             // float minScore = 1; if (score < minScore) minScore = score (LoopClosing.cc:127-139)
  const float* sc = (const float*)c->hout.p;
  for (int i = 0; i < n_slots; i++) if (sc[i] < m) m = sc[i];
  *min_score = m;
  return 0;
}

int orbv_db_detect_loop_candidates(orbv_db* c, const uint32_t* words, const double* values, int n, const int32_t* connected, int n_connected, float min_score,
                                   int64_t query_id, int32_t* cand, int cap, int32_t* n_cand, const orbv_db_trace* trace) {
  return kfdb_detect(c, KFDB_LOOP, words, values, n, connected, n_connected, min_score, query_id, cand, cap, n_cand, trace);
}

int orbv_db_detect_relocalization_candidates(orbv_db* c, const uint32_t* words, const double* values, int n, int64_t query_id, int32_t* cand, int cap,
                                             int32_t* n_cand, const orbv_db_trace* trace) {
  return kfdb_detect(c, KFDB_RELOC, words, values, n, nullptr, 0, 0.0f, query_id, cand, cap, n_cand, trace);
}

int orbv_db_detect_loop_candidates_begin(orbv_db* c, const uint32_t* words, const double* values, int n, const int32_t* connected, int n_connected, float min_score,
                                         int64_t query_id, int32_t* kept, int kept_cap, int32_t* n_kept) {
  return kfdb_begin(c, KFDB_LOOP, words, values, n, connected, n_connected, min_score, query_id, kept, kept_cap, n_kept);
}

int orbv_db_detect_relocalization_candidates_begin(orbv_db* c, const uint32_t* words, const double* values, int n, int64_t query_id, int32_t* kept, int kept_cap,
                                                   int32_t* n_kept) {
  return kfdb_begin(c, KFDB_RELOC, words, values, n, nullptr, 0, 0.0f, query_id, kept, kept_cap, n_kept);
}

int orbv_db_detect_candidates_finish(orbv_db* c, const int32_t* rows, const int32_t* row_n, int32_t* cand, int cap, int32_t* n_cand,
                                     const orbv_db_trace* trace) {
  ORBHIP_REQUIRE(c && n_cand && cap >= 0 && (cap == 0 || cand), ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(c->pend_kind >= 0, ORBHIP_EINVAL, "no query pending: call a _begin entry first (add / erase / set_best_covisibles / clear cancel it)");
  ORBHIP_REQUIRE(c->pend_kept == 0 || (rows && row_n), ORBHIP_EINVAL, "NULL neighbour rows");
  ORBHIP_REQUIRE(!trace || trace->kept_cap >= 0, ORBHIP_EINVAL, "bad trace capacity");
  for (int i = 0; i < c->pend_kept; i++) ORBHIP_REQUIRE(row_n[i] >= 0 && row_n[i] <= KFDB_MAX_NEIGH, ORBHIP_EINVAL, "a row has at most 10 neighbours");
  if (int rc = kfdb_device(c)) return rc;
  const int kind = c->pend_kind;
  c->pend_kind = -1;
  KfdbStaged st{};
  if (int rc = kfdb_host_query(c, kind, 2, nullptr, nullptr, 0, nullptr, 0, c->pend_min_score, c->pend_qid, rows, row_n, c->pend_kept, cap, trace != nullptr, &st)) return rc;
  return kfdb_deliver(st, cand, cap, n_cand, trace);
}

int orbv_db_pending_fields(orbv_db* c, orbv_db_query_info* info, int32_t* n_common, float* score, int cap) {
  ORBHIP_REQUIRE(c && info && cap >= 0 && (cap == 0 || (n_common && score)), ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(c->pend_kind >= 0, ORBHIP_EINVAL, "no query pending: call a _begin entry first (add / erase / set_best_covisibles / clear cancel it)");
  const int S = c->pend_S;
  if (S > cap) { set_error("keyframe database: %d slots, capacity %d", S, cap); return ORBHIP_ECAP; }
  if (int rc = kfdb_device(c)) return rc;
  const KfdbLayout L(S, 1);
  const uint8_t* w = c->ws.as<uint8_t>();
  hipError_t e = hipMemcpyAsync(info, w + L.info, sizeof *info, hipMemcpyDeviceToHost, c->s);
  if (e == hipSuccess && S) e = hipMemcpyAsync(n_common, w + L.count, (size_t)S * 4, hipMemcpyDeviceToHost, c->s);
  if (e == hipSuccess && S) e = hipMemcpyAsync(score, w + L.score, (size_t)S * 4, hipMemcpyDeviceToHost, c->s);
  if (e == hipSuccess) e = hipStreamSynchronize(c->s);
  if (e != hipSuccess) { set_error("orbv_db_pending_fields: %s", hipGetErrorString(e)); return ORBHIP_ENODEV; }
  return 0;
}

int orbv_db_detect_workspace(const orbv_db* c, int n_queries, size_t* bytes) {
  ORBHIP_REQUIRE(c && bytes && n_queries >= 1 && n_queries <= 65535, ORBHIP_EINVAL, "bad argument (1 to 65535 queries)");
  *bytes = KfdbLayout((int)c->slots.size(), n_queries).total;
  return 0;
}

static int kfdb_batch(orbv_db* c, int kind, int Q, const int32_t* q_off, const uint32_t* q_words, const double* q_values, const int32_t* conn_off, const int32_t* conn,
                      const float* min_score, int64_t first_qid, orbv_db_query_info* info, int32_t* cand, int cap, void* ws, size_t ws_bytes, void* stream) {
  ORBHIP_REQUIRE(c && Q >= 1 && Q <= 65535 && q_off && q_words && q_values && info && cap >= 0 && (cap == 0 || cand) && ws, ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(kind == KFDB_RELOC || (conn_off && conn && min_score), ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(ws_bytes >= KfdbLayout((int)c->slots.size(), Q).total, ORBHIP_EINVAL, "workspace smaller than orbv_db_detect_workspace() asks for");
  if (int rc = kfdb_take_id(c, kind, first_qid, Q)) return rc;
  if (int rc = kfdb_device(c)) return rc;
  c->pend_kind = -1;
  return kfdb_enqueue(c, kind, Q, 0, q_off, q_words, q_values, conn_off, conn, min_score, first_qid, (int)c->slots.size(), nullptr, nullptr, (uint8_t*)ws, info, cand,
                      cap, (hipStream_t)stream);
}

int orbv_db_detect_loop_candidates_batch_device(orbv_db* c, int n_queries, const int32_t* d_q_off, const uint32_t* d_q_words, const double* d_q_values,
                                                const int32_t* d_conn_off, const int32_t* d_conn, const float* d_min_score, int64_t first_query_id,
                                                orbv_db_query_info* d_info, int32_t* d_cand, int cap, void* d_workspace, size_t workspace_bytes, void* stream) {
  return kfdb_batch(c, KFDB_LOOP, n_queries, d_q_off, d_q_words, d_q_values, d_conn_off, d_conn, d_min_score, first_query_id, d_info, d_cand, cap, d_workspace,
                    workspace_bytes, stream);
}

int orbv_db_detect_relocalization_candidates_batch_device(orbv_db* c, int n_queries, const int32_t* d_q_off, const uint32_t* d_q_words, const double* d_q_values,
                                                          int64_t first_query_id, orbv_db_query_info* d_info, int32_t* d_cand, int cap, void* d_workspace,
                                                          size_t workspace_bytes, void* stream) {
  return kfdb_batch(c, KFDB_RELOC, n_queries, d_q_off, d_q_words, d_q_values, nullptr, nullptr, nullptr, first_query_id, d_info, d_cand, cap, d_workspace, workspace_bytes,
                    stream);
}

}  // extern "C"
