// host driver - part of the translation unit ba_solver.hip (textually included there; not compiled on its own).
// workspace, structure pass, lockstep batch driver, pose-graph driver (anonymous namespaces).

// ============================================================================ host driver
namespace {

// growable device workspace, reused across calls on the same host thread (slot order = allocation order)
struct PinnedBuf {
  void* p = nullptr; size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return 0;
    if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
    size_t want = need + need / 4;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; set_error("hipHostMalloc(%zu) failed", want); return ORBHIP_ENOMEM; }
    bytes = want;
    return 0;
  }
};
struct BaWorkspace {
  std::vector<DevBuf> slots;
  std::vector<PinnedBuf> hslots;
  // no destructor: freeing device memory from a thread_local destructor can run after the HIP runtime has
  // shut down (observed as a hang at process exit under rocprofv3); the process teardown reclaims it.
};
static thread_local BaWorkspace g_ws;
// the workspace of this thread still holds the complete prepared batch of the last ba_solve_batch_impl call (structure
// arrays, block lists, workspace, final poses / points): LocalBA's second pass solves the SAME observation set and
// reuses it.  Every new walk over the workspace slots (any HostBA) invalidates it.
static thread_local bool g_batch_valid = false;
// one non-blocking stream per host thread: independent solves issued from different threads overlap on the GPU
static thread_local hipStream_t g_stream = nullptr;
static thread_local int g_stream_device = -1;
struct GraphCacheEntry { std::vector<BaDev> D; const BaDev* Dv = nullptr; hipGraphExec_t exec = nullptr; unsigned long long stamp = 0; int mode = 0; };
// Persistent factorisations need their waiting workgroups RESIDENT (the chain waits for rows with larger block indices; the
// one-launch two-level kernel needs its whole grid): the launches in flight on a device are accounted in workgroup slots, and a
// solve that does not get its slots takes the step kernels instead - the results are the same bits either way.
static std::atomic<int> g_persist_used[16];
struct PersistLease {
  int n = 0, dev = 0;
  bool take(int device, int need, int cap) {
    dev = device & 15;
    int cur = g_persist_used[dev].load();
    while (cur + need <= cap)
      if (g_persist_used[dev].compare_exchange_weak(cur, cur + need)) { n = need; return true; }
    return false;
  }
  ~PersistLease() { if (n) g_persist_used[dev].fetch_sub(n); }
};
static thread_local std::vector<GraphCacheEntry> g_graphs;      // instantiated per-iteration graphs of this thread (<= 4, LRU)
static thread_local unsigned long long g_graph_clock = 0;
// pinned, device-mapped byte through which the kernels see the caller's stop flag (a plain bool somewhere in host memory):
// the host copies *stop_flag into it while it waits for the stream, k_ba_iter_begin reads it before every iteration
static thread_local unsigned char* g_stop_host = nullptr;
static thread_local unsigned char* g_stop_dev = nullptr;
static int stop_mirror(unsigned char** host, const volatile unsigned char** dev) {
  if (!g_stop_host) {
    void* h = nullptr; void* d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess || hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      set_error("hipHostMalloc(stop flag mirror) failed"); return ORBHIP_ENOMEM;
    }
    g_stop_host = (unsigned char*)h; g_stop_dev = (unsigned char*)d;
  }
  *host = g_stop_host; *dev = g_stop_dev;
  return 0;
}
// wait for the stream; while waiting, forward the caller's stop flag to the device mirror
static hipError_t wait_stream_forwarding_stop(hipStream_t s, const volatile uint8_t* stop, unsigned char* mirror) {
  if (!stop || !mirror) return hipStreamSynchronize(s);
  // the first 150 us are polled with yield (PoseOptimization-sized solves end inside them), after that the thread sleeps
  // ~50 us between polls: a LocalBA / GlobalBA no longer burns a host core for its whole duration, and the stop flag still
  // reaches the device within one LM iteration
  const auto t0 = std::chrono::steady_clock::now();
  bool spin = true;
  for (;;) {
    if (*stop) __atomic_store_n(mirror, (unsigned char)1, __ATOMIC_RELEASE);
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return hipSuccess;
    if (q != hipErrorNotReady) return q;
    if (spin) {
      std::this_thread::yield();
      spin = std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(150);
    } else {
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
  }
}
// measurement hook (ba_set_profiling / ba_get_profile): device time of the solves of this host thread, HIP events on its stream
static std::atomic<int> g_ba_profiling{0};
static thread_local hipEvent_t g_prof_ev[2] = {nullptr, nullptr};
static thread_local double g_prof_ms = 0.0;
static thread_local int g_prof_solves = 0, g_prof_iters = 0;
static hipStream_t thread_stream() {
  const int dev = g_default_device.load();
  if (g_stream && g_stream_device != dev) {            // the default device changed: drop the old stream and workspace
    (void)hipStreamDestroy(g_stream); g_stream = nullptr;
    g_ws.slots.clear(); g_ws.hslots.clear();           // (buffers of the previous device are intentionally leaked)
    g_graphs.clear();
    g_batch_valid = false;
    g_stop_host = nullptr; g_stop_dev = nullptr;       // the mirror's device pointer belongs to the old device: re-derive it
  }
  static thread_local int prio_cur = 0;
  const int prio_want = thread_ws().prio_want;           // orbhip_set_thread_priority (the Tracking thread's PoseOptimization beside another thread's LocalBA)
  if (g_stream && prio_cur != prio_want) { (void)hipStreamSynchronize(g_stream); (void)hipStreamDestroy(g_stream); g_stream = nullptr; g_graphs.clear(); }
  if (!g_stream) {
    int lo = 0, hi = 0;
    hipError_t e;
    if (prio_want && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo) e = hipStreamCreateWithPriority(&g_stream, hipStreamNonBlocking, hi);
    else e = hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking);
    if (e != hipSuccess) g_stream = nullptr;
    g_stream_device = dev; prio_cur = prio_want;
  }
  return g_stream;
}

struct HostBA {
  HostBA() { g_batch_valid = false; }
  size_t next = 0, hnext = 0;
  // pinned host staging (reused across calls): structure arrays are built straight into it so that the
  // H2D copies are true async DMA and never touch freshly mmap'ed pageable pages
  template <typename T> T* pinned(size_t count, int* rc) {
    if (hnext >= g_ws.hslots.size()) g_ws.hslots.resize(hnext + 1);
    PinnedBuf& b = g_ws.hslots[hnext++];
    int r = b.ensure(std::max<size_t>(count * sizeof(T), 16));
    if (r && !*rc) *rc = r;
    return (T*)b.p;
  }
  template <typename T> T* alloc(size_t count, int* rc) {
    if (next >= g_ws.slots.size()) g_ws.slots.resize(next + 1);
    DevBuf& b = g_ws.slots[next++];
    int r = b.ensure(std::max<size_t>(count * sizeof(T), 16));
    if (r && !*rc) *rc = r;
    return b.as<T>();
  }
  template <typename T> T* upload(const T* src, size_t count, int* rc, hipStream_t st = 0) {
    T* d = alloc<T>(count, rc);
    if (!*rc && count) { if (hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess) { set_error("hipMemcpy H2D failed"); *rc = ORBHIP_ENODEV; } }
    return d;
  }
  // Upload arena: the arrays of one problem whose sizes are known up front are built (or copied) into ONE pinned block at
  // 256-byte-aligned offsets and reach the device with ONE copy into a device block of the same layout - a problem used to
  // issue ~23 small H2D copies (a batched solve spent 10 % of its GPU time in 4-us copy kernels).
  uint8_t* ar_h = nullptr; uint8_t* ar_d = nullptr; size_t ar_off = 0, ar_cap = 0;
  int begin_arena(size_t bytes) {
    int rc = 0;
    ar_h = pinned<uint8_t>(bytes, &rc); ar_d = alloc<uint8_t>(bytes, &rc);
    ar_off = 0; ar_cap = bytes;
    return rc;
  }
  static size_t arena_need(size_t count, size_t elem) { return align256(count * elem); }
  template <typename T> T* arena_host(size_t count, int* rc) {
    const size_t need = arena_need(std::max<size_t>(count, 1), sizeof(T));
    if (ar_off + need > ar_cap) { if (!*rc) { set_error("internal: upload arena too small"); *rc = ORBHIP_EINVAL; } return nullptr; }
    T* h = (T*)(ar_h + ar_off); ar_off += need;
    return h;
  }
  template <typename T> T* arena_copy(const T* src, size_t count, int* rc) {       // caller memory -> arena (host side)
    T* h = arena_host<T>(count, rc);
    if (h && count) std::memcpy(h, src, count * sizeof(T));
    return h;
  }
  template <typename T> T* arena_dev(const T* host_ptr) const { return host_ptr ? (T*)(ar_d + ((const uint8_t*)host_ptr - ar_h)) : nullptr; }
  // defer: a helper thread of a lockstep batch (BaPrepPool) builds the arenas but leaves the copies to the calling thread, which
  // issues them after the join - several host threads inside hipMemcpyAsync at once is what the runtime handles worst (common.h)
  struct Pending { void* d; const void* h; size_t bytes; };
  std::vector<Pending>* defer = nullptr;
  int flush_arena(hipStream_t st) {
    if (ar_off && defer) { defer->push_back({ar_d, ar_h, ar_off}); return 0; }
    if (ar_off && hipMemcpyAsync(ar_d, ar_h, ar_off, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("hipMemcpy H2D failed"); return ORBHIP_ENODEV; }
    return 0;
  }
  // second arena of a problem: the arrays whose sizes are known only after the pair lists have been counted (block lists, pair
  // lists) - they were seven separate copies per problem
  uint8_t* a2_h = nullptr; uint8_t* a2_d = nullptr; size_t a2_off = 0, a2_cap = 0;
  int begin_arena2(size_t bytes) {
    int rc = 0;
    a2_h = pinned<uint8_t>(bytes, &rc); a2_d = alloc<uint8_t>(bytes, &rc);
    a2_off = 0; a2_cap = bytes;
    return rc;
  }
  template <typename T> T* arena2_host(size_t count, int* rc) {
    const size_t need = arena_need(std::max<size_t>(count, 1), sizeof(T));
    if (a2_off + need > a2_cap) { if (!*rc) { set_error("internal: second upload arena too small"); *rc = ORBHIP_EINVAL; } return nullptr; }
    T* h = (T*)(a2_h + a2_off); a2_off += need;
    return h;
  }
  template <typename T> T* arena2_copy(const T* src, size_t count, int* rc) {
    T* h = arena2_host<T>(count, rc);
    if (h && count) std::memcpy(h, src, count * sizeof(T));
    return h;
  }
  template <typename T> T* arena2_dev(const T* host_ptr) const { return host_ptr ? (T*)(a2_d + ((const uint8_t*)host_ptr - a2_h)) : nullptr; }
  int flush_arena2(hipStream_t st) {
    if (a2_off && defer) { defer->push_back({a2_d, a2_h, a2_off}); return 0; }
    if (a2_off && hipMemcpyAsync(a2_d, a2_h, a2_off, hipMemcpyHostToDevice, st) != hipSuccess) { set_error("hipMemcpy H2D failed"); return ORBHIP_ENODEV; }
    return 0;
  }
  // for host data that does NOT outlive the enqueue (function-local vectors, stack structs): an asynchronous copy from
  // pageable memory may read its source after the call returned, so the data is first copied into this thread's pinned
  // staging, which stays valid until the solve has drained
  template <typename T> T* upload_staged(const T* src, size_t count, int* rc, hipStream_t st) {
    T* h = pinned<T>(count, rc);
    if (*rc) return nullptr;
    if (count) std::memcpy(h, src, count * sizeof(T));
    return upload(h, count, rc, st);
  }
};

// ---- one problem: validation, structure (host, O(nobs)), uploads, device workspace -----------------------------------
struct BaInputs {
  const double* K4; double* poses7; const uint8_t* cam_fixed; int ncam; double* pts3; int npts;
  const int32_t* obs_cam; const int32_t* obs_pt; const double* obs_uv; const double* obs_w; const uint8_t* obs_robust; int nobs;
  const uint8_t* cam_local = nullptr;   // LocalBA only: cameras whose observations are classified after the solve
};
struct BaPrepared { BaDev D; int nb_obs, nb_cam, nb_pt; size_t npairs; double t_struct_ms; std::vector<int> perm; uint8_t* h_rob; BaState* h_st; };
struct BaBatch {
  std::vector<BaPrepared> P; std::vector<BaDev> Dh; const BaDev* Dv = nullptr;
  int g_obs, g_cam, g_pt, g_ptc, g_blk, g_npad, g_pad, g_n6, g_camcount, g_apply; size_t g_zero;     // g_ptc: landmark workgroups of k_ba_cam_blocks (0 when k_ba_eval<0> sums every problem's landmark blocks)
  int g_npad_la, g_npad_2l;         // largest reduced system factored by the look-ahead kernel / by the two-level scheme (0: none)
  int g_band;                       // widest skyline of the batch's systems, in 32-column tiles
  int g_persist_nwg; bool g_la_persist_ok, g_la_large, g_wg_ok;      // g_wg_ok: every look-ahead system fits k_chol_wg's list of active rows (<= 32 block rows, or a band <= CW_BAND_MAX)      // k_chol_persist: workgroups of the largest look-ahead system; every look-ahead system fits its flag layout; one has more than 32 block rows
  unsigned char* out_d = nullptr; unsigned char* out_h = nullptr; size_t out_bytes = 0; std::vector<size_t> out_off;      // k_ba_collect's block (device, pinned host)
};
static thread_local BaBatch g_batch;

static double ba_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the plan of a call: which member of the factorisation family the reduced systems of the batch take -------------------------
// ONE function decides (ba_plan_factorisation below; INTEGRATION.md section 7 has the same table); the launch code only reads the plan,
// and ba_get_last_plan hands it to the caller (bench_ba.py and the tests report / assert the form that ran).
//   per problem, ba_prepare:  chol_la = ORBHIP_BA_LOOKAHEAD != 0 && (npad <= ORBHIP_BA_LA_MAX (1024)
//                                        || (persist_nwg <= 160 && wg_rows <= 34 && block rows <= 1024))      "look-ahead family", else "two-level"
//   look-ahead family:  LA_PERSIST  the lease granted the persistent launch (<= 16 problems per call, every system fits the flag layout)
//                       LA_WG       lockstep batch of >= 32 problems; >= 4 problems when one system has > 1024 unknowns; ANY call whose
//                                   large narrow system did not get the lease (the step kernels would walk its dense trailing matrix per step)
//                       LA_STEPS    one launch per 32-column step (what the bit-identity tests compare the others with)
//   two-level family:   TL_PERSIST_BLK (lease granted) / TL_HYBRID_STEPS / TL_CLASSIC (experiments) / TL_ONE_LAUNCH (experiments)
//   backward substitution:  BS_SKY when every system of the call has a band <= BS_SKY_BAND tiles, else BS_SUPERBLOCKS
enum { LA_NONE = 0, LA_PERSIST = 1, LA_WG = 2, LA_STEPS = 3 };
enum { TL_NONE = 0, TL_PERSIST_BLK = 1, TL_HYBRID_STEPS = 2, TL_CLASSIC = 3, TL_ONE_LAUNCH = 4 };
enum { BS_SKY = 1, BS_SUPERBLOCKS = 2 };
struct BaPlan { int ny, la_form, tl_form, bsolve_form, npad_la, npad_2l, band, persist_nwg, persist_mode, la_large, wg_ok, reserved; };
static thread_local BaPlan g_last_plan = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static int ba_prepare(HostBA& H, hipStream_t s, const BaInputs& in, const ba_options* opts, BaPrepared* out) {
  const int ncam = in.ncam, npts = in.npts, nobs = in.nobs;
  ORBHIP_REQUIRE(ncam > 0 && npts >= 0 && nobs >= 0, ORBHIP_EINVAL, "bad sizes");
  ORBHIP_REQUIRE(in.K4 && in.poses7 && in.cam_fixed && (npts == 0 || in.pts3), ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(nobs == 0 || (in.obs_cam && in.obs_pt && in.obs_uv && in.obs_w && in.obs_robust), ORBHIP_EINVAL, "NULL observation arrays");
  for (int i = 0; i < nobs; i++)
    ORBHIP_REQUIRE(in.obs_cam[i] >= 0 && in.obs_cam[i] < ncam && in.obs_pt[i] >= 0 && in.obs_pt[i] < npts, ORBHIP_EINVAL, "observation index out of range");
  const double t_start = ba_now_ms();
  // group observations by point (stable), per-camera lists
  int rc = 0;
  {
    typedef HostBA A;
    const size_t no = (size_t)nobs, nc = (size_t)ncam, npt = (size_t)npts;
    const size_t bytes = A::arena_need(npt + 1, 4) + 5 * A::arena_need(no, 4) + A::arena_need(2 * no, 8) + A::arena_need(no, 8) + A::arena_need(no, 1) +
                         A::arena_need(nc + 1, 4) + A::arena_need(4 * nc, 8) + 2 * A::arena_need(nc, 1) + A::arena_need(nc, 4) + A::arena_need(7 * nc, 8) +
                         A::arena_need(3 * npt, 8) + A::arena_need(1, sizeof(BaState)) + 16 * 256;
    if (int r = H.begin_arena(bytes)) return r;
  }
  int* pt_off = H.arena_host<int>(npts + 1, &rc);
  int* oc = H.arena_host<int>(nobs, &rc); int* op = H.arena_host<int>(nobs, &rc);
  double* ouv = H.arena_host<double>(2 * (size_t)nobs, &rc); double* ow = H.arena_host<double>(nobs, &rc);
  uint8_t* orb = H.arena_host<uint8_t>(nobs, &rc);
  int* cam_off = H.arena_host<int>(ncam + 1, &rc); int* cam_obs = H.arena_host<int>(nobs, &rc); int* cam_obs_pt = H.arena_host<int>(nobs, &rc);
  if (rc) return rc;
  for (int p = 0; p <= npts; p++) pt_off[p] = 0;
  for (int i = 0; i < nobs; i++) pt_off[in.obs_pt[i] + 1]++;
  for (int p = 0; p < npts; p++) pt_off[p + 1] += pt_off[p];
  std::vector<int> perm(nobs), fill(pt_off, pt_off + npts);
  for (int i = 0; i < nobs; i++) perm[fill[in.obs_pt[i]]++] = i;
  for (int j = 0; j < nobs; j++) {
    const int i = perm[j];
    oc[j] = in.obs_cam[i]; op[j] = in.obs_pt[i]; ouv[2 * (size_t)j] = in.obs_uv[2 * (size_t)i]; ouv[2 * (size_t)j + 1] = in.obs_uv[2 * (size_t)i + 1];
    ow[j] = in.obs_w[i]; orb[j] = in.obs_robust[i];
  }
  for (int c = 0; c <= ncam; c++) cam_off[c] = 0;
  for (int j = 0; j < nobs; j++) cam_off[oc[j] + 1]++;
  for (int c = 0; c < ncam; c++) cam_off[c + 1] += cam_off[c];
  std::vector<int> cfill(cam_off, cam_off + ncam);
  int* cam_pos = H.arena_host<int>(nobs, &rc);
  if (rc) return rc;
  for (int j = 0; j < nobs; j++) { int e = cfill[oc[j]]++; cam_obs[e] = j; cam_obs_pt[e] = op[j]; cam_pos[j] = e; }
  const double t_lists = ba_now_ms();
  std::vector<int> cam_col(ncam, -1), free_cams;
  for (int c = 0; c < ncam; c++) if (!in.cam_fixed[c] && cam_off[c + 1] > cam_off[c]) { cam_col[c] = (int)free_cams.size(); free_cams.push_back(c); }
  const int nfc = (int)free_cams.size();
  // ---- optional: a fill-reducing order of the free keyframes (round 6; ORBHIP_BA_ORDER=rcm, read once per process; default: the caller's
  // order, `id`).  The reduced system is factored in the order of its columns and the block Cholesky walks its SKYLINE: a map whose
  // keyframe ids follow the covisibility chain is banded as it comes, one whose ids do not (keyframes inserted out of order, a merged map,
  // a shuffled list) fills the whole triangle.  Reverse Cuthill - McKee over the covisibility graph of the free keyframes (an edge = a
  // shared landmark): breadth-first from a pseudo-peripheral keyframe of every component, neighbours by ascending degree, the whole order
  // reversed - deterministic (ties by the caller's index).  Only the ORDER OF ELIMINATION changes: the summation order of the solve with it,
  // so results agree with the `id` order to rounding (the oracle bars hold: tests/test_gpu_ba_structures.py), not bit for bit.
  static const int order_mode = []() { const char* e = std::getenv("ORBHIP_BA_ORDER"); return (e && std::strcmp(e, "rcm") == 0) ? 1 : 0; }();
  if (order_mode == 1 && nfc > 2 && !opts->fix_points) {
    const int W = (nfc + 63) / 64;
    std::vector<unsigned long long> adj((size_t)nfc * W, 0ull);
    std::vector<int> cs;
    for (int p = 0; p < npts; p++) {
      cs.clear();
      for (int i = pt_off[p]; i < pt_off[p + 1]; i++) { const int c = cam_col[oc[i]]; if (c >= 0) cs.push_back(c); }
      for (size_t i = 0; i < cs.size(); i++)
        for (size_t j = i + 1; j < cs.size(); j++)
          if (cs[i] != cs[j]) { adj[(size_t)cs[i] * W + (cs[j] >> 6)] |= 1ull << (cs[j] & 63); adj[(size_t)cs[j] * W + (cs[i] >> 6)] |= 1ull << (cs[i] & 63); }
    }
    std::vector<int> deg(nfc, 0);
    for (int a = 0; a < nfc; a++) for (int w = 0; w < W; w++) deg[a] += __builtin_popcountll(adj[(size_t)a * W + w]);
    std::vector<int> order; order.reserve(nfc);
    std::vector<char> seen(nfc, 0);
    std::vector<int> level, nb;
    // breadth-first levels from `root` inside its component (seen[] untouched): returns the last level's node of least degree
    auto far_node = [&](int root, std::vector<char>& mark) -> int {
      level.assign(1, root); mark[root] = 1;
      int last_best = root;
      std::vector<int> cur(1, root), nxt;
      while (!cur.empty()) {
        nxt.clear();
        int best = -1;
        for (int a : cur) { if (best < 0 || deg[a] < deg[best] || (deg[a] == deg[best] && a < best)) best = a; }
        last_best = best;
        for (int a : cur)
          for (int w = 0; w < W; w++) {
            unsigned long long m = adj[(size_t)a * W + w];
            while (m) { const int b = 64 * w + __builtin_ctzll(m); m &= m - 1; if (!mark[b]) { mark[b] = 1; nxt.push_back(b); } }
          }
        cur.swap(nxt);
      }
      return last_best;
    };
    for (int s0 = 0; s0 < nfc; s0++) {
      if (seen[s0]) continue;
      // the component's start: least degree, then two sweeps towards a pseudo-peripheral keyframe
      int root = s0;
      { std::vector<char> mark(seen.begin(), seen.end()); const int f1 = far_node(root, mark); std::vector<char> mark2(seen.begin(), seen.end()); root = far_node(f1, mark2); }
      std::vector<int> queue(1, root); seen[root] = 1;
      for (size_t q = 0; q < queue.size(); q++) {
        const int a = queue[q];
        order.push_back(a);
        nb.clear();
        for (int w = 0; w < W; w++) {
          unsigned long long m = adj[(size_t)a * W + w];
          while (m) { const int b = 64 * w + __builtin_ctzll(m); m &= m - 1; if (!seen[b]) { seen[b] = 1; nb.push_back(b); } }
        }
        std::sort(nb.begin(), nb.end(), [&](int x, int y) { return deg[x] != deg[y] ? deg[x] < deg[y] : x < y; });
        queue.insert(queue.end(), nb.begin(), nb.end());
      }
    }
    std::reverse(order.begin(), order.end());
    std::vector<int> fc2(nfc);
    for (int k = 0; k < nfc; k++) fc2[k] = free_cams[order[k]];
    free_cams.swap(fc2);
    for (int k = 0; k < nfc; k++) cam_col[free_cams[k]] = k;
  }
  const int n6 = 6 * nfc, npad = std::max(round_up(n6, NB), NB);
  const int nb_obs = std::max((nobs + BA_TPB - 1) / BA_TPB, 1), nb_cam = (ncam + BA_TPB - 1) / BA_TPB, nb_pt = std::max((npts + BA_TPB - 1) / BA_TPB, 1);
  const int nparts = std::max(nb_obs, std::max(nb_cam, nb_pt));
  // Schur block pair lists: for every point, all ordered observation pairs (i, j) with col_i <= col_j,
  // grouped by block (col_i, col_j) with a counting sort (stable: point order, then list order).
  std::vector<int4> row_meta((size_t)2 * std::max(nfc, 1), make_int4(0, 0, 0, 0)), segs;
  for (int a = 0; a < nfc; a++) { const int ca = free_cams[a]; row_meta[2 * (size_t)a + 1] = make_int4(cam_off[ca], cam_off[ca + 1] - cam_off[ca], ca, 0); }
  int* pair_i = nullptr; int* pair_j = nullptr; size_t npairs_all = 0;
  double t_count = t_lists, t_fill = t_lists;
  std::vector<int> min_partner(std::max(nfc, 1));
  for (int a = 0; a < nfc; a++) min_partner[a] = a;
  if (!opts->fix_points && nfc > 0) {
    // Per point, the free observations are first sorted by column (insertion sort, a handful of entries): the pairs with
    // col_i <= col_j are then simply the positions i <= j of the sorted run - no data-dependent branch in the pair loops
    // (the all-pairs test `cj >= ci` mispredicted every other time: 2.9 -> 1.9 ms for the C4 graph on this host).  A point
    // that a camera observes twice (degenerate inputs) keeps the literal all-pairs form, whose order within a block the
    // sorted form would change; for every other point both forms emit the same pairs in the same order.
    std::vector<int> colv(std::max(nobs, 1));
    for (int j = 0; j < nobs; j++) colv[j] = cam_col[oc[j]];
    // (round 6: the sorted runs of the counting pass are KEPT - run_c / run_i hold a point's free observations by column, run_m their number
    // or -1 for the literal all-pairs form - so the fill pass does not sort again, and what a pair stores of an observation (its place in its
    // camera's list, its place in the concatenated lists) is looked up once per observation instead of once per pair: 0.31 -> see DESIGN.md)
    std::vector<int> run_c(std::max(nobs, 1)), run_i(std::max(nobs, 1)), run_m(std::max(npts, 1));
    std::vector<int> cnt((size_t)nfc * nfc + 1, 0);
    for (int p = 0; p < npts; p++) {
      const int lo = pt_off[p], hi = pt_off[p + 1];
      int* sc = run_c.data() + lo; int* si = run_i.data() + lo;
      int m = 0; bool dup = false; const bool small = (hi - lo) <= 64;
      if (small)
        for (int i = lo; i < hi; i++) {
          const int c = colv[i];
          if (c < 0) continue;
          int k = m++;
          while (k > 0 && sc[k - 1] > c) { sc[k] = sc[k - 1]; si[k] = si[k - 1]; k--; }
          if (k > 0 && sc[k - 1] == c) dup = true;
          sc[k] = c; si[k] = i;
        }
      if (small && !dup) {
        run_m[p] = m;
        for (int i = 0; i < m; i++) { int* row = cnt.data() + (size_t)sc[i] * nfc + 1; for (int j = i; j < m; j++) row[sc[j]]++; }
      } else {
        run_m[p] = -1;
        for (int i = lo; i < hi; i++) { const int ci = colv[i]; if (ci < 0) continue; for (int j = lo; j < hi; j++) if (colv[j] >= ci) cnt[(size_t)ci * nfc + colv[j] + 1]++; }
      }
    }
    for (size_t k = 0; k < (size_t)nfc * nfc; k++) cnt[k + 1] += cnt[k];
    npairs_all = (size_t)cnt[(size_t)nfc * nfc];
    t_count = ba_now_ms();
    for (int a = 0; a < nfc; a++)                               // first column a <= b whose block (a, b) is not empty: the envelope of row b
      for (int b2 = a; b2 < nfc; b2++) { const size_t k = (size_t)a * nfc + b2; if (cnt[k + 1] > cnt[k] && min_partner[b2] > a) min_partner[b2] = a; }
    // segment list: the off-diagonal blocks of a row, in (a, b) order, cut into runs of <= SR_SEG pairs (k_ba_schur: one wave each)
    for (int a = 0; a < nfc; a++) {
      const size_t kd = (size_t)a * nfc + a;
      const int s_lo = (int)segs.size();
      for (int b2 = a + 1; b2 < nfc; b2++) {
        const size_t k = (size_t)a * nfc + b2;
        for (int e = cnt[k]; e < cnt[k + 1]; e += SR_SEG) segs.push_back(make_int4(e, std::min(e + SR_SEG, cnt[k + 1]), b2, (e == cnt[k] ? 1 : 0) | (e + SR_SEG >= cnt[k + 1] ? 2 : 0) | (free_cams[b2] << 2)));
      }
      row_meta[2 * (size_t)a] = make_int4(cnt[kd], cnt[kd + 1], s_lo, (int)segs.size());
    }
    {
      typedef HostBA A;
      if (int r = H.begin_arena2(2 * A::arena_need(npairs_all + 1, 4) + 2 * A::arena_need((size_t)nfc + 1, 4) + A::arena_need(2 * (size_t)nfc + 1, 16) + A::arena_need(segs.size() + 1, 16) + A::arena_need((size_t)npad / NB + 2, 4) + 1024)) return r;
    }
    pair_i = H.arena2_host<int>(npairs_all, &rc); pair_j = H.arena2_host<int>(npairs_all, &rc);
    if (rc) return rc;
    std::vector<int> pos(cnt.begin(), cnt.end() - 1);
    // k_ba_schur keeps camera a's records in LDS by list position: pair_i = position of the observation inside its camera's list;
    // the E records are stored in camera-major order: pair_j = position of the observation in the concatenated lists
    std::vector<int> in_list(std::max(nobs, 1));
    for (int i = 0; i < nobs; i++) in_list[i] = cam_pos[i] - cam_off[oc[i]];
    for (int p = 0; p < npts; p++) {
      const int lo = pt_off[p], hi = pt_off[p + 1], m = run_m[p];
      if (m >= 0) {
        const int* sc = run_c.data() + lo; const int* si = run_i.data() + lo;
        for (int i = 0; i < m; i++) {
          int* row = pos.data() + (size_t)sc[i] * nfc;
          const int pi = in_list[si[i]];
          for (int j = i; j < m; j++) { const int e = row[sc[j]]++; pair_i[e] = pi; pair_j[e] = cam_pos[si[j]]; }
        }
      } else {
        for (int i = lo; i < hi; i++) { const int ci = colv[i]; if (ci < 0) continue;
          for (int j = lo; j < hi; j++) if (colv[j] >= ci) { const int e = pos[(size_t)ci * nfc + colv[j]]++; pair_i[e] = in_list[i]; pair_j[e] = cam_pos[j]; } }
      }
    }
    t_fill = ba_now_ms();
  } else {
    typedef HostBA A;
    if (int r = H.begin_arena2(2 * A::arena_need(1, 4) + 2 * A::arena_need((size_t)nfc + 1, 4) + A::arena_need(2 * (size_t)nfc + 1, 16) + A::arena_need(1, 16) + A::arena_need((size_t)npad / NB + 2, 4) + 1024)) return r;
    pair_i = H.arena2_host<int>(0, &rc); pair_j = H.arena2_host<int>(0, &rc);
    if (rc) return rc;
  }
  // SKYLINE of the reduced system by 32-row tiles: tile_first[i] = the first tile column that holds a structural non-zero of tile row i
  // (block (b, a) of S is non-zero only when the cameras a <= b share a point).  Without pivoting L(i, j) = 0 for every j < tile_first[i]
  // (induction over j: A(i, j) = 0 and every product L(i, k) L(j, k)^T, k < j, has a zero factor), so k_chol_wg leaves those tiles
  // alone - exact zeros skipped, the bits do not change.  Entry nb = the augmented rhs row (dense).
  int* tile_first = H.arena2_host<int>((size_t)npad / NB + 2, &rc);
  if (rc) return rc;
  for (int i = 0; i <= npad / NB; i++) {
    int f = i;
    if (i == npad / NB) f = 0;
    else for (int b2 = (NB * i) / 6; b2 <= std::min(nfc - 1, (NB * i + NB - 1) / 6); b2++) f = std::min(f, (6 * min_partner[b2]) / NB);
    tile_first[i] = f;
  }
  out->t_struct_ms = ba_now_ms() - t_start;
  if (std::getenv("ORBHIP_BA_TIMING_STRUCT"))
    fprintf(stderr, "[ba_prepare] lists %.3f ms, pair counts %.3f, pair fill + segments %.3f, skyline %.3f\n", t_lists - t_start, t_count - t_lists, t_fill - t_count, ba_now_ms() - t_fill);

  BaDev D; std::memset(&D, 0, sizeof(D));
  D.ncam = ncam; D.npts = npts; D.nobs = nobs; D.nfc = nfc; D.n6 = n6; D.npad = npad; D.nparts = nparts;
  D.fix_points = opts->fix_points ? 1 : 0; D.huber = opts->huber_delta;
  static const bool use_la = []() { const char* e = std::getenv("ORBHIP_BA_LOOKAHEAD"); return !(e && e[0] == '0'); }();
  static const int la_max = []() { const char* e = std::getenv("ORBHIP_BA_LA_MAX"); return e ? atoi(e) : 1024; }();
  // Larger systems join the look-ahead family when their SKYLINE is narrow (round 5) - an odometry-like map (GlobalBA C5: 94 block rows,
  // a band of 3).  The persistent launch then needs a ring of 2 R + 3 workgroups instead of ~n^2 / 16, its chain steps are the short ones
  // of the small systems, and a lockstep batch factors such a system in one workgroup (k_chol_wg) whatever its size.
  // A map with a LOOP CLOSURE keeps the band and adds far links: when the keyframes that see the old landmarks come last, only the
  // last block rows have wide envelopes.  The ring walks the narrow prefix, the rows from the first wide one on keep a producer and
  // up to CP_SHARES consumer workgroups each; k_chol_wg takes such a system as long as no column has more active rows than its list.
  const int nbt = npad / NB;
  int band = 0, wmax = 0, first_wide = nbt, band_prefix = 0, wg_rows = 0;
  for (int i = 0; i < nbt; i++) {
    band = std::max(band, i - std::min(tile_first[i], i));
    if (i >= 2) { const int wi = cp_row_consumers(i, tile_first[i]); wmax = std::max(wmax, wi); if (wi > 1 && first_wide == nbt) first_wide = i; }
  }
  for (int i = 0; i < first_wide; i++) band_prefix = std::max(band_prefix, i - std::min(tile_first[i], i));
  for (int c = 0; c < nbt; c++) { int n = 1; for (int i = c; i < nbt; i++) n += (i == c || tile_first[i] <= c) ? 1 : 0; wg_rows = std::max(wg_rows, n); }   // (+ the rhs row)
  static const bool ring_on = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_RING"); return !(e && e[0] == '0'); }();
  D.band = band;
  D.persist_ring = (ring_on && first_wide - 2 > 2 * (band_prefix + 1) + 3) ? band_prefix + 1 : 0;      // (a prefix shorter than the ring keeps a workgroup set per row)
  D.persist_ring_rows = D.persist_ring ? first_wide : 2;
  int pnwg = 3 + (D.persist_ring ? 2 * D.persist_ring : 0);
  for (int i = D.persist_ring_rows; i < nbt; i++) pnwg += 1 + cp_row_consumers(i, tile_first[i]);
  D.persist_nwg = wmax <= CP_SHARES ? pnwg : (1 << 20);      // (more consumer workgroups per row than k_chol_persist's flag layout holds: such a system takes the step kernels)
  D.wg_rows = wg_rows;
  static const bool la_narrow = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_LA_NARROW"); return !(e && e[0] == '0'); }();
  // larger systems join the look-ahead family when the persistent launch stays small (<= 160 workgroups: the device holds ~230 of them)
  // and k_chol_wg's list of active rows holds every column's
  const bool narrow = la_narrow && D.persist_nwg <= 160 && wg_rows <= NB + 2 && nbt <= 1024;
  D.chol_la = (use_la && (npad <= la_max || narrow)) ? 1 : 0;
  {                                                           // the landmark blocks ride on k_ba_eval<0> when no landmark has more than PT_MAXRUN observations
    static const bool pt_fuse = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_PT_FUSE"); return !(e && e[0] == '0'); }();
    int longest = 0;
    for (int p = 0; p < npts; p++) longest = std::max(longest, pt_off[p + 1] - pt_off[p]);
    D.pt_in_eval = (pt_fuse && longest <= PT_MAXRUN) ? 1 : 0;
  }
  // (arena: host images of these arrays sit in one pinned block; ONE copy below moves them all)
  D.K4 = H.arena_dev(H.arena_copy(in.K4, 4 * (size_t)ncam, &rc)); D.cam_fixed = H.arena_dev(H.arena_copy(in.cam_fixed, ncam, &rc));
  D.cam_col = H.arena_dev(H.arena_copy(cam_col.data(), ncam, &rc));
  D.poses = H.arena_dev(H.arena_copy(in.poses7, 7 * (size_t)ncam, &rc)); D.pts = H.arena_dev(H.arena_copy(in.pts3, 3 * (size_t)npts, &rc));
  D.cand_poses = H.alloc<double>(7 * (size_t)ncam, &rc); D.cand_pts = H.alloc<double>(3 * (size_t)npts, &rc);
  D.obs_cam = H.arena_dev(oc); D.obs_pt = H.arena_dev(op); D.obs_uv = H.arena_dev(ouv);
  D.obs_w = H.arena_dev(ow); D.obs_robust = H.arena_dev(orb);
  D.pt_off = H.arena_dev(pt_off); D.cam_off = H.arena_dev(cam_off);
  D.cam_obs = H.arena_dev(cam_obs); D.cam_obs_pt = H.arena_dev(cam_obs_pt);
  D.cam_pos = H.arena_dev(cam_pos); D.Hc = H.alloc<double>(3 * (size_t)std::max(nobs, 1), &rc);
  D.free_cams = H.arena2_dev(H.arena2_copy(free_cams.data(), nfc, &rc));
  D.row_meta = H.arena2_dev(H.arena2_copy(row_meta.data(), row_meta.size(), &rc));
  D.seg = H.arena2_dev(H.arena2_copy(segs.data(), segs.size(), &rc));
  D.pair_i = H.arena2_dev(pair_i); D.pair_j = H.arena2_dev(pair_j);
  D.tile_first = H.arena2_dev(tile_first);
  D.B = H.alloc<double>(21 * (size_t)std::max(nfc, 1), &rc); D.gc = H.alloc<double>(6 * (size_t)std::max(nfc, 1), &rc);
  D.C = H.alloc<double>(6 * (size_t)npts, &rc); D.gp = H.alloc<double>(3 * (size_t)npts, &rc);
  D.scale_c = H.alloc<double>(6 * (size_t)std::max(nfc, 1), &rc); D.scale_p = H.alloc<double>(3 * (size_t)npts, &rc);
  D.Cinv = H.alloc<double>(6 * (size_t)npts, &rc); D.gps = H.alloc<double>(3 * (size_t)npts, &rc); D.Ng = H.alloc<double>(9 * (size_t)npts, &rc);
  D.E = H.alloc<double>(8 * (size_t)std::max(nobs, 1), &rc);
  D.t3 = H.alloc<double>(3 * (size_t)std::max(nobs, 1), &rc);
  D.camrec = H.alloc<double>(16 * (size_t)ncam, &rc);
  D.ae_part = H.alloc<double>(4 * AE_NS, &rc); D.ae_ticket = H.alloc<unsigned int>(4, &rc);
  D.cam_local = in.cam_local ? H.arena_dev(H.arena_copy(in.cam_local, ncam, &rc)) : nullptr;
  D.erase = in.cam_local ? H.alloc<unsigned char>(std::max(nobs, 1), &rc) : nullptr;
  D.S = H.alloc<double>((size_t)(npad + 1) * npad, &rc); D.rhs = H.alloc<double>(npad, &rc);
  D.Dinv = H.alloc<double>((size_t)npad * NB, &rc);
  D.Mb = H.alloc<double>((size_t)npad * NB, &rc); { const int nbm = npad / NB, ntm = (nbm + 1) / 2; D.ncflags = std::max(std::max(256 /* CP_NFLAGS */, 2 + (2 + CP_SHARES) * (nbm + 2)), 2 + 3 * (nbm + 2) + ntm * ntm + 8); D.cflags = H.alloc<int>(D.ncflags, &rc); }
  D.part = H.alloc<double>(6 * (size_t)nparts, &rc);
  D.st = H.alloc<BaState>(1, &rc);
  if (rc) return rc;
  out->h_st = nullptr;                                        // (the LM state, rhs and partial sums are initialised by k_ba_init for the whole batch)
  if (int r = H.flush_arena(s)) return r;
  if (int r = H.flush_arena2(s)) return r;
  out->D = D; out->nb_obs = nb_obs; out->nb_cam = nb_cam; out->nb_pt = nb_pt; out->npairs = npairs_all;
  out->perm.swap(perm); out->h_rob = orb;
  return 0;
}

// ---- helper threads of ONE calling thread: the structure passes of a lockstep batch's problems, side by side -----------------
// ba_prepare is ~1.2 ms of host work per C4-size problem (CSR by point and by camera, Schur pair and segment lists straight into
// pinned arenas): 80 ms for a 64-problem batch on the calling thread alone, against ~35 ms of GPU work.  A calling thread therefore
// owns ORBHIP_BA_PREP_THREADS - 1 helpers (default 4 threads in all; 1 = none; batches of >= 8 problems use them): helper w prepares
// the problems p = w, w + W, ... in order, every time - so each problem meets the same workspace slots of the same thread again and
// the device pointers stay what the cached graphs captured.  Helpers use their OWN thread-local workspace (it outlives the call:
// the resident batch of LocalBA's second pass points into it), make no stream call (the uploads are handed back), and belong to
// one caller only - two callers sharing helpers would overwrite each other's resident batches.
// Cost, stated (ADVICE r4): every host thread that ever solves a batch of >= 8 problems keeps W - 1 helper threads, each with its own
// device + pinned workspace, until that thread exits (twelve batch callers: 48 threads); ORBHIP_BA_PREP_THREADS=1 = none.  The
// process-wide total of helpers is capped (BA_PREP_MAX_HELPERS): callers beyond the cap prepare their batches alone.
// (Round 6, a 256-core host: one caller of 64-problem batches 480 / 1 000 / 1 290 / 1 480 solves/s with 1 / 4 / 8 / 16 threads - a problem whose
// data is cold takes 1.3 - 1.5 ms of structure pass -, twelve callers 4 870 with 4 and 4 740 with 8: the default stays 4, the cap is 128.)
static std::atomic<int> g_prep_helpers{0};
#define BA_PREP_MAX_HELPERS 128
struct BaPrepPool {
  int W = 1; bool initialised = false;
  std::vector<std::thread> th;
  std::mutex mu; std::condition_variable cv, cv_done;
  unsigned long gen = 0; int pending = 0; bool quit = false;
  const BaInputs* in = nullptr; const ba_options* opts = nullptr; BaPrepared* out = nullptr; int nprob = 0, device = 0;
  std::vector<int> rc; std::vector<std::string> err; std::vector<std::vector<HostBA::Pending>> copies;
  void share(int w, HostBA& H) {                               // problems w, w + W, ... with workspace walk H
    H.defer = &copies[w];
    try {
      for (int p = w; p < nprob; p += W) {
        const int r = ba_prepare(H, nullptr, in[p], opts, &out[p]);
        if (r) { rc[w] = r; err[w] = orbhip_last_error(); break; }
      }
    } catch (const std::bad_alloc&) {                           // (a helper thread must hand the error back, not terminate the process)
      rc[w] = ORBHIP_ENOMEM; err[w] = "out of host memory in the structure pass of a batch";
    } catch (...) {
      rc[w] = ORBHIP_EINVAL; err[w] = "exception in the structure pass of a batch";
    }
    H.defer = nullptr;
  }
  void worker(int w) {
    unsigned long seen = 0;
    int seen_device = -1;
    for (;;) {
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return quit || gen != seen; }); if (quit) return; seen = gen; }
      (void)hipSetDevice(device);
      if (device != seen_device) { g_ws.slots.clear(); g_ws.hslots.clear(); seen_device = device; }   // (as thread_stream(): buffers of the previous device are leaked on purpose)
      { HostBA H; share(w, H); }
      { std::lock_guard<std::mutex> lk(mu); if (--pending == 0) cv_done.notify_all(); }
    }
  }
  int threads() {
    if (!initialised) {
      initialised = true;                                       // (the environment is read once per calling thread, whatever it says)
      const char* e = std::getenv("ORBHIP_BA_PREP_THREADS");
      const int want = std::max(1, std::min(e ? atoi(e) : 4, 16));
      try {
        for (int w = 1; w < want; w++) {
          if (g_prep_helpers.fetch_add(1) >= BA_PREP_MAX_HELPERS) { g_prep_helpers.fetch_sub(1); break; }
          try { th.emplace_back([this, w] { worker(w); }); } catch (...) { g_prep_helpers.fetch_sub(1); throw; }
        }
      } catch (...) {                                           // (no more threads to be had: work with those that started)
      }
      W = (int)th.size() + 1;
    }
    return W;
  }
  // prepares all problems (H = the caller's own walk, share 0) and issues the deferred uploads on s; 0 or the first error
  int run(HostBA& H, hipStream_t s, const BaInputs* in_, int nprob_, const ba_options* opts_, BaPrepared* out_) {
    in = in_; opts = opts_; out = out_; nprob = nprob_; device = g_default_device.load();
    rc.assign(W, 0); err.assign(W, std::string()); copies.assign(W, {});
    { std::lock_guard<std::mutex> lk(mu); pending = W - 1; gen++; }
    cv.notify_all();
    share(0, H);
    { std::unique_lock<std::mutex> lk(mu); cv_done.wait(lk, [&] { return pending == 0; }); }
    for (int w = 0; w < W; w++) if (rc[w]) { set_error("%s", err[w].c_str()); return rc[w]; }
    for (int w = 0; w < W; w++)
      for (const HostBA::Pending& c : copies[w])
        if (hipMemcpyAsync(c.d, c.h, c.bytes, hipMemcpyHostToDevice, s) != hipSuccess) { set_error("hipMemcpy H2D failed"); return ORBHIP_ENODEV; }
    return 0;
  }
  ~BaPrepPool() {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    for (std::thread& t : th) if (t.joinable()) { t.join(); g_prep_helpers.fetch_sub(1); }
  }
};
static thread_local BaPrepPool g_prep_pool;

// ---- a batch of independent problems solved in lockstep: every launch covers all of them (grid.y = problem) --------------
// The LM control flow of each problem lives in its own device-side BaState, so finished problems simply fall through.
// One LM iteration is a fixed sequence of ~60 launches: it is captured once into a hipGraph and replayed (one graph
// launch per iteration); instantiated graphs are cached per host thread, keyed by the full kernel-argument blocks
// (sizes and workspace pointers), so repeated solves of the same shape skip the capture too.  ORBHIP_BA_GRAPH=0 = direct.
static BaPlan ba_plan_factorisation(const BaBatch& B, int ny, int persist_mode, bool wg_on, bool classic) {
  BaPlan p; std::memset(&p, 0, sizeof(p));
  p.ny = ny; p.npad_la = B.g_npad_la; p.npad_2l = B.g_npad_2l; p.band = B.g_band; p.persist_nwg = B.g_persist_nwg; p.persist_mode = persist_mode;
  p.la_large = B.g_la_large ? 1 : 0; p.wg_ok = B.g_wg_ok ? 1 : 0;
  if (B.g_npad_la > 0) {
    // one workgroup per system (k_chol_wg): a workgroup takes ~0.3 - 1 ms per factorisation of <= 32 block rows whatever the batch, so below
    // ~32 problems the step kernels' 19 launches are shorter; a call with a larger - narrow-skyline - system takes this form whenever the
    // persistent launch is not available (the step kernels would walk its whole trailing matrix once per column: 94 times for C5).
    const bool wg = wg_on && B.g_wg_ok && (ny >= 32 || (B.g_la_large && B.g_la_persist_ok));
    p.la_form = persist_mode > 0 ? LA_PERSIST : wg ? LA_WG : LA_STEPS;
  }
  if (B.g_npad_2l > 0) p.tl_form = classic ? TL_CLASSIC : persist_mode == 2 ? TL_ONE_LAUNCH : persist_mode > 0 ? TL_PERSIST_BLK : TL_HYBRID_STEPS;
  p.bsolve_form = B.g_band <= BS_SKY_BAND ? BS_SKY : BS_SUPERBLOCKS;
  return p;
}

static int ba_solve_batch_impl(const BaInputs* in, int nprob, const ba_options* opts, ba_summary* summaries, bool reuse_structure = false,
                               uint8_t* const* erase_out = nullptr) {
  ORBHIP_REQUIRE(in && opts && nprob > 0, ORBHIP_EINVAL, "NULL argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (the HIP path has no CPU fallback)"); return ORBHIP_ENODEV; }
  if (int rcd = use_default_device()) return rcd;
  const bool timing = std::getenv("ORBHIP_BA_TIMING") != nullptr;
  const double t_start = ba_now_ms();
  hipStream_t s = thread_stream();
  int rc = 0;
  unsigned char* stop_host = nullptr; const volatile unsigned char* stop_devp = nullptr;
  if (int r = stop_mirror(&stop_host, &stop_devp)) return r;
  *stop_host = 0;                                         // (no solve of this thread is in flight: every call drains its stream)
  BaBatch& B = g_batch;
  bool reused = false;
  if (reuse_structure && g_batch_valid && (int)B.P.size() == nprob) {
    // same cameras, points and observation lists as the batch still resident in this thread's workspace (the caller
    // guarantees it; sizes are re-checked): only the loss flags and the iteration cap change, the solve starts from the
    // poses / points the previous solve left on the device.  No structure pass, no pair lists, no uploads but the flags.
    reused = true;
    for (int p = 0; p < nprob; p++)
      reused = reused && B.Dh[p].ncam == in[p].ncam && B.Dh[p].npts == in[p].npts && B.Dh[p].nobs == in[p].nobs && B.Dh[p].fix_points == (opts->fix_points ? 1 : 0);
  }
  if (reused) {
    for (int p = 0; p < nprob; p++) {
      const BaDev& D = B.Dh[p];
      BaPrepared& Pp = B.P[p];
      for (int j = 0; j < D.nobs; j++) Pp.h_rob[j] = in[p].obs_robust[Pp.perm[j]];
      if (D.nobs) ORBHIP_CHECK_HIP(hipMemcpyAsync(const_cast<unsigned char*>(D.obs_robust), Pp.h_rob, D.nobs, hipMemcpyHostToDevice, s));
      Pp.t_struct_ms = 0.0;
    }
  } else {
    HostBA H;                                             // (invalidates the resident batch)
    B.P.assign(nprob, BaPrepared()); B.Dh.assign(nprob, BaDev());
    B.g_npad_la = 0; B.g_npad_2l = 0; B.g_persist_nwg = 3; B.g_la_persist_ok = true; B.g_la_large = false; B.g_wg_ok = true; B.g_band = 0;
    B.g_obs = 1; B.g_cam = 1; B.g_pt = 1; B.g_ptc = 0; B.g_blk = 0; B.g_npad = NB; B.g_pad = 0; B.g_n6 = 0; B.g_camcount = 1; B.g_apply = 1; B.g_zero = 0;
    // the structure passes: side by side on this thread and its helpers for a batch, one after the other otherwise
    const bool pooled = nprob >= 8 && g_prep_pool.threads() > 1;
    if (pooled) { if (int r = g_prep_pool.run(H, s, in, nprob, opts, B.P.data())) return r; }
    for (int p = 0; p < nprob; p++) {
      if (!pooled) { if (int r = ba_prepare(H, s, in[p], opts, &B.P[p])) return r; }
      B.P[p].D.stop_dev = stop_devp;
      const BaDev& D = B.P[p].D;
      B.Dh[p] = D;
      B.g_obs = std::max(B.g_obs, B.P[p].nb_obs); B.g_cam = std::max(B.g_cam, B.P[p].nb_cam); B.g_pt = std::max(B.g_pt, B.P[p].nb_pt);
      if (!D.pt_in_eval && !D.fix_points) B.g_ptc = std::max(B.g_ptc, B.P[p].nb_pt);
      B.g_blk = std::max(B.g_blk, D.nfc);      /* k_ba_schur: a workgroup per block row */
      B.g_npad = std::max(B.g_npad, D.npad); B.g_pad = std::max(B.g_pad, D.npad - D.n6); B.g_n6 = std::max(B.g_n6, D.n6);
      B.g_camcount = std::max(B.g_camcount, D.ncam); B.g_apply = std::max(B.g_apply, std::max(7 * D.ncam, 3 * D.npts));
      B.g_zero = std::max(B.g_zero, (size_t)D.n6 * D.npad);
      B.g_band = std::max(B.g_band, D.band);
      if (D.chol_la) {
        B.g_npad_la = std::max(B.g_npad_la, D.npad); B.g_persist_nwg = std::max(B.g_persist_nwg, D.persist_nwg);
        if (D.npad > 1024) B.g_la_large = true;
        if (D.wg_rows > NB + 2) B.g_wg_ok = false;                        // (only ORBHIP_BA_LA_MAX can bring such a system here)
        // (a system above 1024 unknowns that ORBHIP_BA_LA_MAX pushed here with a WIDE skyline keeps the step kernels: its rows would want more than four consumer workgroups)
        if (D.persist_nwg >= (1 << 20)) B.g_la_persist_ok = false;
      } else B.g_npad_2l = std::max(B.g_npad_2l, D.npad);
    }
    // the batch's output block: one slice per problem
    B.out_off.assign(nprob, 0); B.out_bytes = 0;
    for (int p = 0; p < nprob; p++) {
      B.out_off[p] = B.out_bytes;
      B.out_bytes += align256(sizeof(BaState)) + align256(7 * (size_t)in[p].ncam * sizeof(double)) + align256(3 * (size_t)in[p].npts * sizeof(double)) + align256((size_t)std::max(in[p].nobs, 1));
    }
    B.out_d = H.alloc<unsigned char>(B.out_bytes, &rc); B.out_h = H.pinned<unsigned char>(B.out_bytes, &rc);
    if (rc) return rc;
    for (int p = 0; p < nprob; p++) { B.Dh[p].out = B.out_d + B.out_off[p]; B.P[p].D.out = B.Dh[p].out; }
    B.Dv = H.upload_staged(B.Dh.data(), nprob, &rc, s);
    if (rc) return rc;
    g_batch_valid = true;
  }
  {
    BaState st0; std::memset(&st0, 0, sizeof(st0));
    st0.radius = 1e4; st0.decrease_factor = 2.0; st0.need_eval = 1; st0.first = 1; st0.max_iters = opts->max_iterations;
    hipLaunchKernelGGL(k_ba_init, dim3(4, (unsigned)nprob), dim3(256), 0, s, B.Dv, st0);
  }
  std::vector<BaPrepared>& P = B.P;
  std::vector<BaDev>& Dh = B.Dh;
  const BaDev* Dv = B.Dv;
  const int g_obs = B.g_obs, g_cam = B.g_cam, g_pt = B.g_pt, g_ptc = B.g_ptc, g_blk = B.g_blk, g_npad = B.g_npad, g_pad = B.g_pad, g_n6 = B.g_n6, g_camcount = B.g_camcount, g_apply = B.g_apply;
  const size_t g_zero = B.g_zero;
  const double t_upload = ba_now_ms();
  const bool prof = g_ba_profiling.load() != 0;
  if (prof) {
    for (int k = 0; k < 2; k++) if (!g_prof_ev[k]) ORBHIP_CHECK_HIP(hipEventCreate(&g_prof_ev[k]));
    ORBHIP_CHECK_HIP(hipEventRecord(g_prof_ev[0], s));
  }
  const unsigned ny = (unsigned)nprob;
  if (int r = raise_dynamic_lds((const void*)k_ba_schur, g_stream_device, SR_LDS_BYTES)) return r;
  if (int r = raise_dynamic_lds((const void*)k_chol_wg, g_stream_device, CW_LDS_DOUBLES * sizeof(double))) return r;
  const int npad_all = g_npad;
  // ---- which form of the Cholesky this solve takes (0 step kernels, 1 persistent launches, 2 the one-launch two-level kernel)
  static const int persist_max = []() {
    const char* e = std::getenv("ORBHIP_BA_PERSIST");      // 0: the step kernels (the bit-identity tests), 1 (default): the persistent launches; 2 = the one-launch kernel, ORBHIP_EXPERIMENTS builds only
#ifdef ORBHIP_EXPERIMENTS
    return e && e[0] >= '0' && e[0] <= '2' ? e[0] - '0' : 1;
#else
    return e && e[0] == '0' ? 0 : 1;
#endif
  }();
  static const int OB = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_OB"); const int v = e ? atoi(e) : 128; return (v >= 64 && v <= 1024 && v % 32 == 0) ? v : 128; }();
  PersistLease lease;
  int persist_mode = 0, p2_workers = 0, persist_cus = 0;
  // (round 5: up to 16 problems per call - with the ring a narrow-skyline system needs 11 workgroups, so a small batch fits the device's
  // slots and its 0.12 - 0.6 ms persistent launch beats 19 - 94 step launches or k_chol_wg's 0.3 - 1.4 ms; the lease below decides: 8 x C4
  // 1590 -> 1970 solves/s, 16 x C4 2370 -> 2610, eight C5 sub-maps 135 -> 102 ms.  Until then: fewer than four problems)
  static const int persist_ny_max = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_PERSIST_NY"); return e ? atoi(e) : 16; }();
  if (persist_max > 0 && ny <= (unsigned)persist_ny_max && B.g_la_persist_ok) {
    static thread_local int cus = 0, occ2l = 0, occ1 = 0, cu_dev = -1;
    if (cu_dev != g_stream_device) {
      hipDeviceProp_t prop;
      cus = hipGetDeviceProperties(&prop, g_stream_device) == hipSuccess ? prop.multiProcessorCount : 0;
      (void)raise_dynamic_lds((const void*)k_chol_persist, g_stream_device, CP_LDS_DOUBLES * sizeof(double));
      (void)raise_dynamic_lds((const void*)k_chol_persist_blk, g_stream_device, CP_LDS_DOUBLES * sizeof(double));
#ifdef ORBHIP_EXPERIMENTS
      (void)raise_dynamic_lds((const void*)k_chol_persist_2l, g_stream_device, CP_LDS_DOUBLES * sizeof(double));
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ2l, k_chol_persist_2l, 256, CP_LDS_DOUBLES * sizeof(double)) != hipSuccess) occ2l = 0;
#endif
      int oa = 0, ob = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&oa, k_chol_persist, 256, CP_LDS_DOUBLES * sizeof(double)) != hipSuccess) oa = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&ob, k_chol_persist_blk, 256, CP_LDS_DOUBLES * sizeof(double)) != hipSuccess) ob = 0;
      occ1 = std::min(oa, ob);
      (void)hipGetLastError();
      cu_dev = g_stream_device;
    }
    persist_cus = cus * std::max(occ1, 1);
    const int cap = cus * std::min(occ1, 2) * 9 / 10;         // resident workgroups of the persistent kernels the device holds (registers / 76 KB LDS), with a margin
    int need = 0;
    if (B.g_npad_la > 0) need += B.g_persist_nwg * (int)ny;
    if (B.g_npad_2l > 0) need += (B.g_npad_2l / NB + 2) * (int)ny;
    // the one-launch kernel: a single large problem, outer blocks of 2 or 4 panels, the whole device
    const int nbm2 = B.g_npad_2l / NB, ntm2 = (nbm2 + 1) / 2, cap2 = occ2l * cus * 9 / 10;
    if (persist_max >= 2 && ny == 1 && B.g_npad_la == 0 && nbm2 >= 8 && (OB == 64 || OB == 128) && cap2 - nbm2 >= std::max(64, ntm2) && lease.take(g_stream_device, std::max(cap, 1), std::max(cap, 1))) {
      persist_mode = 2; p2_workers = std::min(384, cap2 - nbm2);
    } else if (need > 0 && lease.take(g_stream_device, need, cap)) persist_mode = 1;
  }
  if (g_pad > 0) hipLaunchKernelGGL(k_ba_pad, dim3(g_pad, ny), dim3(64), 0, s, Dv);
  // lockstep batches factored by k_chol_wg: the reduced systems are cleared ONCE here, an iteration clears only the tiles inside the skyline
  static const bool wg_on = []() { const char* e = std::getenv("ORBHIP_BA_WG"); return !(e && e[0] == '0'); }();      // (0: the step kernels, for the bit-identity tests)
  // one workgroup per system (k_chol_wg): a workgroup takes ~0.3 - 1 ms per factorisation of <= 32 block rows whatever the batch, so below
  // ~32 problems the step kernels' 19 launches are shorter; a batch with a larger - narrow-band - system takes this form from four
  // problems on (the step kernels would walk its whole trailing matrix 94 times).  Same bits either way.
  static const bool classic = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_2L_CLASSIC"); return e && e[0] == '1'; }();
  const BaPlan plan = ba_plan_factorisation(B, (int)ny, persist_mode, wg_on, classic);
  g_last_plan = plan;
  const bool use_wg = plan.la_form == LA_WG;
  const bool wg_env = use_wg;                               // k_chol_wg never writes outside the skyline: an iteration clears only the envelope
  if (wg_env && g_n6 > 0) hipLaunchKernelGGL(k_ba_zero_S, dim3(std::min(1024, (int)((g_zero + 255) / 256)), ny), dim3(256), 0, s, Dv, 1);
  auto enqueue_eval = [&]() {
    hipLaunchKernelGGL(k_ba_eval<0>, dim3(g_obs, ny), dim3(BA_TPB), 0, s, Dv);
    hipLaunchKernelGGL(k_ba_cam_blocks, dim3(g_camcount + g_ptc, ny), dim3(BA_TPB), 0, s, Dv, g_camcount);     // + the landmark blocks of the problems whose k_ba_eval<0> does not sum them
    hipLaunchKernelGGL(k_ba_after_eval, dim3(ny >= 8 ? 1 : AE_NS, ny), dim3(AE_TPB), 0, s, Dv);      // (a lockstep batch fills the device by itself: one workgroup walks the slices)
  };
  auto enqueue_iteration = [&]() {
    // (k_ba_iter_begin's work is the tail of the previous k_ba_after_eval since round 5)
    const int g_zs = g_n6 > 0 ? std::min(1024, (int)((g_zero + 255) / 256)) : 0;
    hipLaunchKernelGGL(k_ba_schur_prep, dim3(g_pt + g_zs, ny), dim3(BA_TPB), 0, s, Dv, g_pt, wg_env ? 1 : 0);   // + zeroing of S
    if (g_blk > 0) hipLaunchKernelGGL(k_ba_schur, dim3(g_blk, ny), dim3(SC_TPB), SR_LDS_BYTES, s, Dv);      // one workgroup per block row
    const int npad = B.g_npad_2l;                             // (0 when every problem of the batch takes the look-ahead scheme)
    auto launch_update = [&](hipStream_t st_, int kcol, int K, int r_lo, int c_lo, int c_hi, int c_hi_cap) {
      if (c_hi <= c_lo || r_lo >= npad + 1) return;
      const int tiles_r = (npad - r_lo + 63) / 64, tiles_c = (c_hi - c_lo + 63) / 64;
      const int ntiles = std::max(tiles_r, 0) * tiles_c;
      const int nrhs = (c_hi - c_lo + 255) / 256;
      hipLaunchKernelGGL(k_chol_syrk, dim3(ntiles + nrhs, ny), dim3(256), 0, st_, Dv, kcol, K, r_lo, c_lo, c_hi_cap, tiles_c, ntiles);
    };
    // one look-ahead step: panel k + the previous step's update of the columns [k + 32, c_end) (c_end = min(cap, n))
    // + (hybrid) this step's share of the previous outer block's wide update
    auto launch_la = [&](int np_, int k, int k0, int c_cap, int hybrid, CholWide w) {
      const int rows_below = np_ - k - NB;
      const int r_lo = k + NB, c_end = std::min(c_cap, np_);
      int tiles_c = 1, ntiles = 0, nrhs = 0;
      if (k > k0 && r_lo < c_end) { tiles_c = (c_end - r_lo + 63) / 64; ntiles = ((np_ - r_lo + 63) / 64) * tiles_c; nrhs = (c_end - r_lo + 255) / 256; }
      const int nC = w.nq > 0 ? (w.total - w.q + w.nq - 1) / w.nq + (w.q == 0 ? w.nrhs : 0) : 0;
      if (ny >= 4 && np_ <= 1024) { const int nA = (rows_below + 1 + 255) / 256; hipLaunchKernelGGL(k_chol_la<4>, dim3(nA + ntiles + nrhs + nC, ny), dim3(256), 0, s, Dv, k, k0, c_cap, nA, tiles_c, ntiles, ntiles + nrhs, hybrid, w); }
      else { const int nA = (rows_below + 1 + 63) / 64; hipLaunchKernelGGL(k_chol_la<1>, dim3(nA + ntiles + nrhs + nC, ny), dim3(256), 0, s, Dv, k, k0, c_cap, nA, tiles_c, ntiles, ntiles + nrhs, hybrid, w); }
    };
    const CholWide no_wide = {0, 0, 0, 1, 0, 0, 0, 0};
    // look-ahead family (reduced systems <= 1024 unknowns, larger ones with a narrow skyline): the whole factorisation as ONE persistent
    // launch when the lease granted it (<= 16 problems per call; ORBHIP_BA_PERSIST=0 disables), one workgroup per system for lockstep
    // batches, else one launch per 32-column step (panel + the previous step's update) - bit-identical, all three
    const bool use_persist = persist_mode > 0;
    if (plan.la_form == LA_PERSIST) {
      // (the chain, producer + consumers of the rows 2 .. nb - 1, the rhs row's two: counted per problem from its skyline, ba_prepare)
      hipLaunchKernelGGL(k_chol_persist, dim3(B.g_persist_nwg, ny), dim3(256), CP_LDS_DOUBLES * sizeof(double), s, Dv);
    } else if (plan.la_form == LA_WG) {                       // one workgroup per problem, the whole factorisation in one launch
      hipLaunchKernelGGL(k_chol_wg, dim3(ny), dim3(CW_TPB), CW_LDS_DOUBLES * sizeof(double), s, Dv);
    } else
    for (int k = 0, npl = B.g_npad_la; k < npl; k += NB) launch_la(npl, k, 0, INT_MAX, 0, no_wide);
    // two-level scheme (outer block = 4 panels of NB = 32) for the larger systems.
    if (plan.tl_form == TL_CLASSIC) {
      // round-1 form: panel -> thin update -> panel ... -> one wide update
      for (int k0 = 0; k0 < npad; k0 += OB) {
        const int kend = std::min(k0 + OB, npad);
        for (int k = k0; k < kend; k += NB) {
          const int rows_below = npad - k - NB;
          if (ny >= 4 && npad <= 1024) hipLaunchKernelGGL(k_chol_panel<4>, dim3((rows_below + 1 + 255) / 256, ny), dim3(256), 0, s, Dv, k);
          else hipLaunchKernelGGL(k_chol_panel<1>, dim3((rows_below + 1 + 63) / 64, ny), dim3(256), 0, s, Dv, k);   // +1: augmented rhs row
          if (k + NB < kend) launch_update(s, k, NB, k + NB, k + NB, kend, k0 + OB);      // thin update inside the outer block
        }
        if (kend < npad) launch_update(s, k0, kend - k0, kend, kend, npad, INT_MAX);      // one wide update for everything to the right
      }
#ifdef ORBHIP_EXPERIMENTS
    } else if (npad > 0 && persist_mode == 2) {
      hipLaunchKernelGGL(k_chol_persist_2l, dim3(npad / NB + p2_workers, ny), dim3(256), CP_LDS_DOUBLES * sizeof(double), s, Dv, OB / NB, p2_workers);
#endif
    } else if (npad > 0) {
      // hybrid: the steps of an outer block are look-ahead launches confined to the block (the thin updates leave the serial
      // chain); of its K = 128 update only the NEXT outer block's 128 columns are a launch of their own (the chain needs
      // them), everything further right rides along with the next block's steps (role C).  One stream: every entry still
      // receives its updates in one fixed order.
      CholWide w = no_wide;
      for (int k0 = 0; k0 < npad; k0 += OB) {
        const int kend = std::min(k0 + OB, npad);
        w.nq = w.total > 0 ? (kend - k0) / NB : 0;
        if (use_persist) {
          // one persistent launch per outer block: the chain, a workgroup per block row below, the previous block's K = 128 update
          const int nbm = npad / NB, nend_ = std::min(kend + OB, npad);
          BlkGeo geo;
          geo.jb0 = k0 / NB; geo.ns = (kend - k0) / NB; geo.blk = k0 / OB; geo.base = std::max(nbm - (geo.jb0 + 2), 0) + 2;
          geo.kend = kend / NB; geo.nend = nend_ / NB;
          geo.tcn = kend < npad ? (nend_ - kend + 63) / 64 : 0;
          geo.n_tiles_n = geo.tcn * ((npad - kend + 63) / 64);
          geo.n_rhs_n = kend < npad ? (nend_ - kend + 255) / 256 : 0;
          geo.n_tiles_c = w.total > 0 ? ((w.tiles_c + 1) / 2) * std::max(w.tiles_c - geo.tcn, 0) : 0;      // items of two vertically adjacent tiles
          // the pool behind the rows: the owners of the next block's tiles + as many workgroups as the device holds besides (they
          // all draw from the queue of the previous block's far tiles)
          const int n_items = w.total > 0 ? geo.n_tiles_c + w.nrhs : 0;
          const int n_pool = std::max(geo.n_tiles_n + geo.n_rhs_n, std::min(n_items, persist_cus - geo.base));
          hipLaunchKernelGGL(k_chol_persist_blk, dim3(geo.base + std::max(n_pool, 0), ny), dim3(256), CP_LDS_DOUBLES * sizeof(double), s, Dv, geo, w);
        } else
        for (int k = k0, q = 0; k < kend; k += NB, q++) { w.q = q; launch_la(npad, k, k0, k0 + OB, 1, w); }
        w = no_wide;
        if (kend >= npad) break;
        const int nend = std::min(kend + OB, npad);
        if (!use_persist) launch_update(s, k0, kend - k0, kend, kend, nend, kend + OB);      // (the persistent launch did it itself)
        if (nend < npad) {
          const int t = (npad - nend + 63) / 64;
          w.kcol = k0; w.K = kend - k0; w.lo = nend; w.tiles_c = t; w.total = t * t; w.nrhs = (npad - nend + 255) / 256;
        }
      }
    }
    // Backward substitution.  Systems with a narrow skyline (every problem of the call: band <= BS_SKY_BAND tiles) take ONE launch of one
    // workgroup per problem (k_chol_bsolve_sky: the update of a super-block touches two or three 64-column chunks); the others one
    // launch per super-block + one for its update over all the rows above (for a DENSE system of <= 1024 unknowns the one-launch form was
    // measured slower: 298 us per LM iteration against 287 - the update's eight workgroups side by side beat four saved launch boundaries).
    // (round 6: k_chol_bsolve_sky4, the same arithmetic on four waves with the blocks requested three steps ahead; ORBHIP_BA_BSOLVE_WAVES=0: the 1024-thread form)
    static const bool bs_waves = []() { const char* e = std::getenv("ORBHIP_BA_BSOLVE_WAVES"); return !(e && e[0] == '0'); }();
    if (plan.bsolve_form == BS_SKY && bs_waves) hipLaunchKernelGGL(k_chol_bsolve_sky4, dim3(1, ny), dim3(BW_TPB), 0, s, Dv);
    else if (plan.bsolve_form == BS_SKY) hipLaunchKernelGGL(k_chol_bsolve_sky, dim3(1, ny), dim3(1024), 0, s, Dv);
    else
    for (int kb = ((npad_all - 1) / SBLK) * SBLK; kb >= 0; kb -= SBLK) {
      hipLaunchKernelGGL(k_chol_bsolve_diag, dim3(1, ny), dim3(1024), 0, s, Dv, kb);
      if (kb > 0) hipLaunchKernelGGL(k_chol_bsolve_update, dim3((kb + 63) / 64, ny), dim3(1024), 0, s, Dv, kb);
    }
    hipLaunchKernelGGL(k_ba_cam_update, dim3(g_cam, ny), dim3(BA_TPB), 0, s, Dv);
    hipLaunchKernelGGL(k_ba_backsub, dim3(g_pt, ny), dim3(BS_TPB), 0, s, Dv, 0);
    hipLaunchKernelGGL(k_ba_eval<1>, dim3(g_obs, ny), dim3(BA_TPB), 0, s, Dv);
    hipLaunchKernelGGL(k_ba_iter_end, dim3(1, ny), dim3(BA_TPB), 0, s, Dv);
    hipLaunchKernelGGL(k_ba_apply, dim3((g_apply + BA_TPB - 1) / BA_TPB, ny), dim3(BA_TPB), 0, s, Dv);
    enqueue_eval();
  };
  const volatile uint8_t* stop = opts->stop_flag;
  if (stop && *stop) __atomic_store_n(stop_host, (unsigned char)1, __ATOMIC_RELEASE);      // (the first evaluation's tail is the beginning of iteration 1: it must see a flag that is already up)
  enqueue_eval();                                             // iteration 0
  bool user_stop = stop && *stop;                             // StopFlagCallback after iteration 0
  int launched = 0;
  hipGraphExec_t gexec = nullptr;
  static const bool use_graph = []() { const char* e = ORBHIP_EXP_ENV("ORBHIP_BA_GRAPH"); return !(e && e[0] == '0'); }();
  if (use_graph && opts->max_iterations >= 3 && !user_stop) {
    for (auto& e : g_graphs)
      if (e.exec && e.Dv == Dv && e.mode == persist_mode && e.D.size() == Dh.size() && std::memcmp(e.D.data(), Dh.data(), Dh.size() * sizeof(BaDev)) == 0) { gexec = e.exec; e.stamp = ++g_graph_clock; break; }
    if (!gexec) {
      hipGraph_t graph = nullptr;
      ORBHIP_CHECK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      enqueue_iteration();
      ORBHIP_CHECK_HIP(hipStreamEndCapture(s, &graph));
      hipError_t ge = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (ge != hipSuccess) { set_error("hipGraphInstantiate failed: %s", hipGetErrorString(ge)); return ORBHIP_ENODEV; }
      GraphCacheEntry* slot = nullptr;
      if (g_graphs.size() < 4) { g_graphs.emplace_back(); slot = &g_graphs.back(); }
      else { slot = &g_graphs[0]; for (auto& e : g_graphs) if (e.stamp < slot->stamp) slot = &e; }
      if (slot->exec) { ORBHIP_CHECK_HIP(hipStreamSynchronize(s)); (void)hipGraphExecDestroy(slot->exec); }
      slot->D = Dh; slot->Dv = Dv; slot->mode = persist_mode; slot->exec = gexec; slot->stamp = ++g_graph_clock;
    }
  }
  for (int it = 0; it < opts->max_iterations + 1 && !user_stop; it++) {
    // ("iteration cap reached" is recorded by the tail of the last iteration's k_ba_after_eval - the next iteration's beginning: the
    // pass after the last iteration has nothing to launch)
    if (it == opts->max_iterations) { }
    else if (gexec) { ORBHIP_CHECK_HIP(hipGraphLaunch(gexec, s)); launched++; }
    else { enqueue_iteration(); launched++; }
    if (stop && *stop) { __atomic_store_n(stop_host, (unsigned char)1, __ATOMIC_RELEASE); user_stop = true; }   // the device stops at its next iteration boundary
    if ((it & 7) == 7 && it + 8 < opts->max_iterations) {     // all converged early? (poll every 8 iterations of long solves)
      std::vector<BaState> cur(nprob);
      for (int p = 0; p < nprob; p++) ORBHIP_CHECK_HIP(hipMemcpyAsync(&cur[p], Dh[p].st, sizeof(BaState), hipMemcpyDeviceToHost, s));
      ORBHIP_CHECK_HIP(wait_stream_forwarding_stop(s, stop, stop_host));
      bool all = true;
      for (int p = 0; p < nprob; p++) all = all && cur[p].done;
      if (all) break;
    }
  }
  const double t_enq = ba_now_ms();
  if (user_stop) hipLaunchKernelGGL(k_ba_user_stop, dim3(1, ny), dim3(1), 0, s, Dv, launched);
  ORBHIP_CHECK_HIP(hipGetLastError());
  if (prof) ORBHIP_CHECK_HIP(hipEventRecord(g_prof_ev[1], s));
  // the iterations are all enqueued: a flag raised from now on reaches the device through the mirror (StopFlagCallback is
  // polled after EVERY iteration, include/CeresOptimizer.h:332-349), the iterations behind it fall through
  if (stop) ORBHIP_CHECK_HIP(wait_stream_forwarding_stop(s, stop, stop_host));
  std::vector<BaState> fin(nprob);
  const bool classify = erase_out != nullptr && Dh[0].erase != nullptr;
  if (classify) hipLaunchKernelGGL(k_ba_classify, dim3(g_obs, ny), dim3(BA_TPB), 0, s, Dv);
  hipLaunchKernelGGL(k_ba_collect, dim3(16, ny), dim3(256), 0, s, Dv, classify ? 1 : 0);
  ORBHIP_CHECK_HIP(hipGetLastError());
  // (the megabyte-sized blocks of a solve stay on the copy engines: by kernel - as the per-frame calls' small blocks go, common.h - a
  // 12-thread batched LocalBA lost 4 %: 2545-2608 against 2689-2726 solves/s)
  ORBHIP_CHECK_HIP(hipMemcpyAsync(B.out_h, B.out_d, B.out_bytes, hipMemcpyDeviceToHost, s));
  ORBHIP_CHECK_HIP(hipStreamSynchronize(s));
  {
    for (int p = 0; p < nprob; p++) {
      const unsigned char* o = B.out_h + B.out_off[p];
      std::memcpy(&fin[p], o, sizeof(BaState)); o += align256(sizeof(BaState));
      std::memcpy(in[p].poses7, o, 7 * (size_t)in[p].ncam * sizeof(double)); o += align256(7 * (size_t)in[p].ncam * sizeof(double));
      if (in[p].npts) std::memcpy(in[p].pts3, o, 3 * (size_t)in[p].npts * sizeof(double));
      o += align256(3 * (size_t)in[p].npts * sizeof(double));
      if (classify && in[p].nobs) std::memcpy(P[p].h_rob, o, in[p].nobs);
    }
  }
  if (prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof_ev[0], g_prof_ev[1]) == hipSuccess) g_prof_ms += ms;
    g_prof_solves += nprob;
    for (int p = 0; p < nprob; p++) g_prof_iters += fin[p].iteration;
  }
  if (timing) {
    double ts = 0; size_t pairs = 0; long nobs = 0;
    for (int p = 0; p < nprob; p++) { ts += P[p].t_struct_ms; pairs += P[p].npairs; nobs += in[p].nobs; }
    fprintf(stderr, "[ba_solve] problems=%d nobs=%ld pairs=%zu | structure %.2f ms, prepare+upload %.2f ms, enqueue %.2f ms, drain+download %.2f ms\n",
            nprob, nobs, pairs, ts, t_upload - t_start, t_enq - t_upload, ba_now_ms() - t_enq);
  }
  if (classify)
    for (int p = 0; p < nprob; p++)
      for (int j = 0; j < in[p].nobs; j++) erase_out[p][P[p].perm[j]] = P[p].h_rob[j];
  if (summaries)
    for (int p = 0; p < nprob; p++) {
      ba_summary& o = summaries[p];
      o.initial_cost = fin[p].initial_cost; o.final_cost = fin[p].x_cost; o.iterations = fin[p].iteration;
      o.successful_steps = fin[p].successful_steps; o.termination = fin[p].termination; o.final_radius = fin[p].radius;
    }
  for (int p = 0; p < nprob; p++)
    if (fin[p].termination == 7) {
      set_error("problem %d of %d: a workgroup of the persistent Cholesky waited longer than the time limit for another one "
                "(the device is oversubscribed or hung); the outputs hold the last accepted iterate", p, nprob);
      return ORBHIP_ETIMEOUT;
    }
  return 0;
}

int ba_solve_impl(const double* K4, double* poses7, const uint8_t* cam_fixed, int ncam, double* pts3, int npts,
                  const int32_t* obs_cam_in, const int32_t* obs_pt_in, const double* obs_uv_in, const double* obs_w_in,
                  const uint8_t* obs_robust_in, int nobs, const ba_options* opts, ba_summary* summary) {
  ORBHIP_REQUIRE(opts, ORBHIP_EINVAL, "NULL options");
  BaInputs in{K4, poses7, cam_fixed, ncam, pts3, npts, obs_cam_in, obs_pt_in, obs_uv_in, obs_w_in, obs_robust_in, nobs};
  return ba_solve_batch_impl(&in, 1, opts, summary);
}

}  // namespace

namespace {

int pg_solve_impl(double* lie7, const uint8_t* kf_fixed, int n, const int32_t* edge_j, const int32_t* edge_i, const double* edge_Sji, int ne,
                  int max_iterations, const volatile uint8_t* stop, ba_summary* summary) {
  ORBHIP_REQUIRE(lie7 && kf_fixed && n > 0 && ne >= 0 && max_iterations >= 0, ORBHIP_EINVAL, "NULL argument");
  ORBHIP_REQUIRE(ne == 0 || (edge_j && edge_i && edge_Sji), ORBHIP_EINVAL, "NULL edge arrays");
  for (int e = 0; e < ne; e++)
    ORBHIP_REQUIRE(edge_j[e] >= 0 && edge_j[e] < n && edge_i[e] >= 0 && edge_i[e] < n && edge_i[e] != edge_j[e], ORBHIP_EINVAL, "edge vertex out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (the HIP path has no CPU fallback)"); return ORBHIP_ENODEV; }
  if (int rcd = use_default_device()) return rcd;
  std::vector<int> col(n, -1);
  int nf = 0;
  for (int v = 0; v < n; v++) if (!kf_fixed[v]) col[v] = nf++;
  const int n7 = 7 * nf, npad = std::max(round_up(std::max(n7, 1), NB), NB);
  // The reduced system is dense: (npad + 1) * npad doubles.  Round 1 refused more than 2340 free keyframes (npad > 16384); the
  // factorisation itself has no size limit (all offsets are 64-bit), so the only bound is device memory: 4700 keyframes need
  // 8.7 GB, 10000 keyframes 39 GB of the 288 GB.  (The reference's sparse Cholesky has no limit either.)
  { size_t free_b = 0, total_b = 0;
    const size_t need = ((size_t)(npad + 1) * npad + (size_t)npad * NB) * sizeof(double);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b) {
      set_error("essential graph with %d free keyframes needs %.1f GB for the dense reduced system, %.1f GB free on the device", nf, need / 1e9, free_b / 1e9);
      return ORBHIP_ECAP;
    } }
  // incident edge lists (insertion order) and off-diagonal block lists
  std::vector<int> v_off(n + 1, 0), v_edge(2 * (size_t)ne); std::vector<signed char> v_sign(2 * (size_t)ne);
  for (int e = 0; e < ne; e++) { v_off[edge_i[e] + 1]++; v_off[edge_j[e] + 1]++; }
  for (int v = 0; v < n; v++) v_off[v + 1] += v_off[v];
  { std::vector<int> fill(v_off.begin(), v_off.end() - 1);
    for (int e = 0; e < ne; e++) { int q = fill[edge_i[e]]++; v_edge[q] = e; v_sign[q] = 1; q = fill[edge_j[e]]++; v_edge[q] = e; v_sign[q] = -1; } }
  std::vector<std::pair<long long, int>> keyed;
  for (int e = 0; e < ne; e++) {
    const int ci = col[edge_i[e]], cj = col[edge_j[e]];
    if (ci < 0 || cj < 0) continue;
    const int a = std::max(ci, cj), b = std::min(ci, cj);
    keyed.push_back({(long long)a * nf + b, e});
  }
  std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<long long, int>& x, const std::pair<long long, int>& y) { return x.first < y.first; });
  std::vector<int> blk_a, blk_b, blk_off(1, 0), blk_edge;
  for (size_t k = 0; k < keyed.size(); k++) {
    if (k == 0 || keyed[k].first != keyed[k - 1].first) {
      if (k) blk_off.push_back((int)blk_edge.size());
      blk_a.push_back((int)(keyed[k].first / nf)); blk_b.push_back((int)(keyed[k].first % nf));
    }
    blk_edge.push_back(keyed[k].second);
  }
  if (!keyed.empty()) blk_off.push_back((int)blk_edge.size());
  const int nblk = (int)blk_a.size();
  const int nb_e = std::max((ne + 127) / 128, 1), nb_v = (n + 127) / 128;
  const int nparts = std::max(std::max(nb_e, nb_v), std::max((ne + BA_TPB - 1) / BA_TPB, (n + BA_TPB - 1) / BA_TPB));

  hipStream_t s = thread_stream();
  HostBA H; int rc = 0;
  PgDev P; std::memset(&P, 0, sizeof(P));
  P.n = n; P.nf = nf; P.n7 = n7; P.npad = npad; P.ne = ne; P.nblk = nblk; P.nparts = nparts;
  P.x = H.upload(lie7, 7 * (size_t)n, &rc, s); P.cand = H.alloc<double>(7 * (size_t)n, &rc); P.col = H.upload(col.data(), n, &rc, s);
  P.ej = H.upload(edge_j, ne, &rc, s); P.ei = H.upload(edge_i, ne, &rc, s); P.Sji = H.upload(edge_Sji, 7 * (size_t)ne, &rc, s);
  P.r = H.alloc<double>(7 * (size_t)std::max(ne, 1), &rc); P.J = H.alloc<double>(49 * (size_t)std::max(ne, 1), &rc);
  P.g = H.alloc<double>(std::max(n7, 1), &rc); P.scale = H.alloc<double>(std::max(n7, 1), &rc);
  P.v_off = H.upload(v_off.data(), n + 1, &rc, s); P.v_edge = H.upload(v_edge.data(), v_edge.size(), &rc, s); P.v_sign = H.upload(v_sign.data(), v_sign.size(), &rc, s);
  P.blk_a = H.upload(blk_a.data(), nblk, &rc, s); P.blk_b = H.upload(blk_b.data(), nblk, &rc, s); P.blk_off = H.upload(blk_off.data(), blk_off.size(), &rc, s);
  P.blk_edge = H.upload(blk_edge.data(), blk_edge.size(), &rc, s);
  P.vpart = H.alloc<double>(2 * (size_t)n, &rc);
  P.S = H.alloc<double>((size_t)(npad + 1) * npad, &rc); P.rhs = H.alloc<double>(npad, &rc);
  double* Dinv = H.alloc<double>((size_t)npad * NB, &rc);
  P.part = H.alloc<double>(6 * (size_t)nparts, &rc);      // (row 5: the cameras' share of the model cost change in the BA kernels; k_ba_iter_end reads it - zero here)
  P.st = H.alloc<BaState>(1, &rc);
  if (rc) return rc;
  // the view through which the shared Cholesky / controller kernels see this problem (sizes chosen so that k_ba_iter_end
  // sums exactly the partial slots written above: candidate cost and model change per 256 edges ... see nparts)
  BaDev F; std::memset(&F, 0, sizeof(F));
  F.npad = npad; F.n6 = n7; F.nparts = nparts; F.S = P.S; F.rhs = P.rhs; F.Dinv = Dinv; F.part = P.part; F.st = P.st;
  F.nobs = nb_e * BA_TPB; F.npts = nb_e * BA_TPB; F.ncam = nb_v * BA_TPB;     // -> nb_obs = nb_pt = nb_e blocks, nb_cam = nb_v blocks
  unsigned char* stop_host = nullptr;
  if (int r = stop_mirror(&stop_host, &F.stop_dev)) return r;
  *stop_host = 0;
  const BaDev* Fv = H.upload(&F, 1, &rc, s);
  if (rc) return rc;
  BaState st0; std::memset(&st0, 0, sizeof(st0));
  st0.radius = 1e4; st0.decrease_factor = 2.0; st0.need_eval = 1; st0.first = 1; st0.max_iters = max_iterations;
  ORBHIP_CHECK_HIP(hipMemcpyAsync(P.st, &st0, sizeof(st0), hipMemcpyHostToDevice, s));
  ORBHIP_CHECK_HIP(hipMemsetAsync(P.rhs, 0, (size_t)npad * sizeof(double), s));
  ORBHIP_CHECK_HIP(hipMemsetAsync(P.part, 0, 6 * (size_t)nparts * sizeof(double), s));
  if (npad > n7) hipLaunchKernelGGL(k_pg_pad, dim3(npad - n7), dim3(64), 0, s, P);
  auto enqueue_eval = [&]() {
    hipLaunchKernelGGL(k_pg_eval, dim3(nb_e), dim3(128), 0, s, P, 0);
    hipLaunchKernelGGL(k_pg_vertex, dim3(nb_v), dim3(128), 0, s, P);
    hipLaunchKernelGGL(k_pg_after_eval, dim3(1), dim3(256), 0, s, P);
  };
  enqueue_eval();
  bool user_stop = stop && *stop;
  for (int it = 0; it < max_iterations + 1 && !user_stop && n7 > 0; it++) {
    hipLaunchKernelGGL(k_ba_iter_begin, dim3(1, 1), dim3(1), 0, s, Fv);
    if (it == max_iterations) break;                          // (only records "iteration cap reached")
    hipLaunchKernelGGL(k_ba_zero_S, dim3(std::min(1024, (int)(((size_t)n7 * npad + 255) / 256)), 1), dim3(256), 0, s, Fv, 0);
    hipLaunchKernelGGL(k_pg_build, dim3(n + nblk), dim3(64), 0, s, P);
    auto launch_update = [&](int kcol, int K, int r_lo, int c_lo, int c_hi, int c_hi_cap) {
      if (c_hi <= c_lo || r_lo >= npad + 1) return;
      const int tiles_r = (npad - r_lo + 63) / 64, tiles_c = (c_hi - c_lo + 63) / 64;
      const int ntiles = std::max(tiles_r, 0) * tiles_c;
      const int nrhs = (c_hi - c_lo + 255) / 256;
      hipLaunchKernelGGL(k_chol_syrk, dim3(ntiles + nrhs, 1), dim3(256), 0, s, Fv, kcol, K, r_lo, c_lo, c_hi_cap, tiles_c, ntiles);
    };
    const int OB = 128;
    for (int k0 = 0; k0 < npad; k0 += OB) {
      const int kend = std::min(k0 + OB, npad);
      for (int k = k0; k < kend; k += NB) {
        const int rows_below = npad - k - NB;
        hipLaunchKernelGGL(k_chol_panel<1>, dim3((rows_below + 1 + 63) / 64, 1), dim3(256), 0, s, Fv, k);
        if (k + NB < kend) launch_update(k, NB, k + NB, k + NB, kend, k0 + OB);
      }
      if (kend < npad) launch_update(k0, kend - k0, kend, kend, npad, INT_MAX);
    }
    for (int kb = ((npad - 1) / SBLK) * SBLK; kb >= 0; kb -= SBLK) {
      hipLaunchKernelGGL(k_chol_bsolve_diag, dim3(1, 1), dim3(1024), 0, s, Fv, kb);
      if (kb > 0) hipLaunchKernelGGL(k_chol_bsolve_update, dim3((kb + 63) / 64, 1), dim3(1024), 0, s, Fv, kb);
    }
    hipLaunchKernelGGL(k_pg_step, dim3(nb_v), dim3(128), 0, s, P);
    hipLaunchKernelGGL(k_pg_mcc, dim3(nb_e), dim3(128), 0, s, P);
    hipLaunchKernelGGL(k_pg_eval, dim3(nb_e), dim3(128), 0, s, P, 1);
    hipLaunchKernelGGL(k_ba_iter_end, dim3(1, 1), dim3(BA_TPB), 0, s, Fv);
    hipLaunchKernelGGL(k_pg_apply, dim3((7 * n + 255) / 256), dim3(256), 0, s, P);
    enqueue_eval();
    if (stop && *stop) { __atomic_store_n(stop_host, (unsigned char)1, __ATOMIC_RELEASE); user_stop = true; }
    if ((it & 3) == 3) {                                       // converged early? (pose graphs usually need ~10 of the 100 iterations)
      BaState cur;
      ORBHIP_CHECK_HIP(hipMemcpyAsync(&cur, P.st, sizeof(cur), hipMemcpyDeviceToHost, s));
      ORBHIP_CHECK_HIP(wait_stream_forwarding_stop(s, stop, stop_host));
      if (cur.done) break;
    }
  }
  if (user_stop) hipLaunchKernelGGL(k_ba_user_stop, dim3(1, 1), dim3(1), 0, s, Fv, INT_MAX);
  ORBHIP_CHECK_HIP(hipGetLastError());
  if (stop) ORBHIP_CHECK_HIP(wait_stream_forwarding_stop(s, stop, stop_host));
  BaState fin;
  ORBHIP_CHECK_HIP(hipMemcpyAsync(&fin, P.st, sizeof(fin), hipMemcpyDeviceToHost, s));
  ORBHIP_CHECK_HIP(hipMemcpyAsync(lie7, P.x, 7 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  ORBHIP_CHECK_HIP(hipStreamSynchronize(s));
  if (summary) {
    summary->initial_cost = fin.initial_cost; summary->final_cost = fin.x_cost; summary->iterations = fin.iteration;
    summary->successful_steps = fin.successful_steps; summary->termination = fin.termination; summary->final_radius = fin.radius;
  }
  return 0;
}

}  // namespace
