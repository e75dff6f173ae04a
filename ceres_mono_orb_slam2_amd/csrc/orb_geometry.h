// ============================================================================
// orb_geometry.h -- what the extractor's kernels and its host half share (orb_extractor.hip), and the PLAN: everything that
// depends only on (extractor parameters, image shape) - level geometry, FAST cells, octree capacities, resize tables, blur tiles,
// cone boxes, LDS sizes.  Plain integer / float arithmetic with no HIP in it: a host compiler and its sanitizers reach all of it
// (tests/cpp/test_extractor_plan.cpp).  The conditions the kernels rely on are the small predicates next to the step that
// depends on them.
// ============================================================================
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbslam_hip.h"
#include "align.h"

namespace orbhip {

static const int PATCH_SIZE = 31, HALF_PATCH = 15, EDGE_THRESHOLD = 19;
static const int MAX_LEVELS = 16;
static const int MAX_INI = 64;            // initial octree nodes per level (round(W/H))
static const int KEYCAP_MAX = 1 << 23;     // the dense candidate array of a (frame, level) is sized for its theoretical worst case (cells x
                                           // in-cell NMS density 1/4); this bound only keeps the 24-bit candidate index of the octree's
                                           // best-key word valid (a 4095 x 4095 level has at most 4.2 M).  ORBHIP_KEYCAP lowers it (test hook)
// launch shapes the plan sizes its tables for (the kernels' own comments say why these values)
#define CONE_TPB 1024     /* k_pyr_cone: a lone wave per SIMD issues one instruction per ~4.5 cycles: four waves per SIMD share the work of a cone */
#define CONE_MAXL 8        /* pyramid levels the cone kernel handles (its table registers are unrolled over the levels) */
#define CONE_SRC_PT 12      /* bytes of the level 0 box a thread loads (all requested at once) */
#define BLUR_TW 128       /* k_blur7's tile */
#define BLUR_TH 64
#define BM_TW 192                   /* k_blur7_mfma: output columns per workgroup (4 waves x 48) */
#define BM_TH 58                    /* output rows per chunk */
#define BM_RC 4                     /* chunks (of 58 rows) a wave walks down its 48 columns: the Toeplitz operands are loaded once, the next
                                       chunk's source is in flight during the products (one-chunk waves were dispatch- and latency-bound:
                                       0.425 ms per 256 frames at 26 % VALU-busy) */
#define DESC_WPB 4      // k_describe: keypoints (= waves) per workgroup (1 / 2 / 4 / 8 / 16: 0.575 / 0.548 / 0.530 / 0.551 / 0.587 ms)

struct LevelDev {
  int w, h;
  int pitch;            // bytes per row of the un-blurred level (level 0: the caller's stride)
  int bpitch;           // bytes per row of the blurred level
  long long pyr_off;    // byte offset inside one frame's pyramid block (levels >= 1)
  long long blur_off;   // byte offset inside one frame's blurred block
  int minBX, minBY, winW, winH;   // detection window origin and size (maxBorder - minBorder)
  int cell_begin, ncells;
  int quota;
  int nIni; float hX;
  int ini_x[MAX_INI + 1];
  float scale; float patch;
  int kcap; int key_off;          // dense key capacity / offset (in keys) inside one frame's key block
  int dblk_begin, dblk_count;     // k_describe: first workgroup of this level / number of workgroups (level capacity / DESC_WPB)
};

struct GeomDev {
  int nlevels, ncells_total, cell_cap, sel_cap, keys_per_frame, desc_blocks;
  int tile_w, tile_h, tile_pitch;       // FAST LDS tile (max cell incl. apron)
  int node_cap, max_cells_level;
#ifdef ORBHIP_OCT_LEVEL_EXPERIMENT
  int oct_level_mask;
#endif
  long long pyr_frame_bytes, blur_frame_bytes;
  LevelDev lv[MAX_LEVELS];
};

struct alignas(16) CellDesc { short level, x0, y0, x1, y1, offx, offy, pad; };   // 16-byte aligned: read with one scalar load
struct alignas(8) BlurTile { short level, tx, ty, pad; };

inline int cv_round(double v) { return (int)std::nearbyint(v); }

// ---------------------------------------------------------------------------- tables of the extractor parameters alone
struct ScaleTables {
  std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
  std::vector<int> quota, umax;
  float atan_p[4], factorPI;
};
inline ScaleTables scale_tables(int nfeatures, double scaleFactor, int nl) {
  ScaleTables t;
  t.scale.resize(nl); t.sigma2.resize(nl); t.inv_scale.resize(nl); t.inv_sigma2.resize(nl);
  t.scale[0] = 1.0f; t.sigma2[0] = 1.0f;
  for (int i = 1; i < nl; i++) {
    t.scale[i] = (float)(t.scale[i - 1] * scaleFactor);        // src/ORBextractor.cc:421
    t.sigma2[i] = t.scale[i] * t.scale[i];
  }
  for (int i = 0; i < nl; i++) { t.inv_scale[i] = 1.0f / t.scale[i]; t.inv_sigma2[i] = 1.0f / t.sigma2[i]; }
  t.quota.resize(nl);
  float factor = (float)(1.0f / scaleFactor);
  float nDesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
  int sum = 0;
  for (int l = 0; l < nl - 1; l++) { t.quota[l] = cv_round(nDesired); sum += t.quota[l]; nDesired *= factor; }
  t.quota[nl - 1] = std::max(nfeatures - sum, 0);
  t.umax.assign(HALF_PATCH + 1, 0);
  int v, v0, vmax = (int)std::floor(HALF_PATCH * std::sqrt(2.f) / 2 + 1);
  int vmin = (int)std::ceil(HALF_PATCH * std::sqrt(2.f) / 2);
  const double hp2 = HALF_PATCH * HALF_PATCH;
  for (v = 0; v <= vmax; ++v) t.umax[v] = cv_round(std::sqrt(hp2 - v * v));
  for (v = HALF_PATCH, v0 = 0; v >= vmin; --v) {
    while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
    t.umax[v] = v0;
    ++v0;
  }
  const float k = (float)(180.0 / 3.14159265358979323846);
  t.atan_p[0] = 0.9997878412794807f * k; t.atan_p[1] = -0.3258083974640975f * k;
  t.atan_p[2] = 0.1555786518463281f * k; t.atan_p[3] = -0.04432655554792128f * k;
  t.factorPI = (float)(3.14159265358979323846 / 180.f);
  return t;
}

// Node arrays of one (frame, level) octree workgroup.  LDS instantiation with 16-bit counters: 44 bytes per node, so that the 442
// nodes of nfeatures = 2000 take 19.3 kB and EIGHT workgroups share a CU's 160 kB - all 2048 workgroups of a 256-frame batch are
// resident at once (at 50 bytes per node plus a separate cell-prefix array only six fitted and the kernel ran in two rounds).  The
// scan arrays are 16-bit there (values <= 4 node_cap), the cell-prefix array of the gather phase lies over everything behind rect[0]
// (nothing else is live yet), the final-phase sort keys and the processing order share the childpos rows (dead until phase G),
// the best-key array the child-count rows (dead after the last sweep).
inline size_t octree_lds_bytes(int node_cap, int max_cells_level, bool wide, bool gmem) {
  const size_t scan_b = (wide || gmem) ? 4 : 2;
  const size_t per_node = 8 * 2 + (wide ? 16 : 8) + 8 + 2 * scan_b + (wide ? 4 : 2) * 2 + 2 + 2;
  const size_t nodes = (size_t)node_cap * per_node, pref = (size_t)node_cap * 8 + (size_t)(max_cells_level + 8) * 4;
  return std::max(nodes, pref) + 16;
}

// ---------------------------------------------------------------------------- the plan
struct ExtractorParams { int nlevels; const float* inv_scale; const float* scale; const int* quota; };   // (ScaleTables' arrays)

struct RmHost { size_t oW = 0, oC = 0, oC0 = 0, oRow = 0; int nchunks = 0, nblocks = 0; bool ok = false; };   // k_resize_mfma's tables of a level
struct ConePlan { size_t tab = 0; int wgs = 0, buf0 = 0, bufk = 0; size_t lds = 0; };      // k_pyr_cone: boxes in tab, grid, LDS layout (wgs == 0: not available)

struct ExtractorPlan {
  GeomDev G;
  std::vector<CellDesc> cells;
  std::vector<BlurTile> btiles, mtiles, mtiles1;      // k_blur7's 128 x 64 tiles, k_blur7_mfma's strips of BM_RC chunks (batches) / of one chunk (a lone frame: latency)
  std::vector<uint8_t> tab;                            // the byte image of the device table block; every piece starts on 16 bytes
  std::vector<size_t> tab_xofs, tab_yofs, tab_ibeta;   // byte offsets into tab per level (k_resize / k_pyr_cone)
  std::vector<RmHost> rm;                              // per level (ok = false: the level takes k_resize)
  ConePlan cone;
  bool fast_narrow = false;           // k_fast_cells<true>: all cell interiors <= 32 px wide
  size_t fast_lds = 0;
  bool octree_wide = false;           // some level can hold > 65535 candidates: 32-bit node counters (k_octree<true, .>)
  bool octree_gmem = false;           // node arrays larger than the LDS: global scratch rows (k_octree<., true>)
  size_t octree_lds = 0, octree_lds_wide = 0, octree_row = 0;
};

#define ORBHIP_PLAN_REQUIRE(cond, msg) do { if (!(cond)) { *why = msg " (" #cond ")"; return ORBHIP_EINVAL; } } while (0)

inline size_t tab_push(std::vector<uint8_t>& tab, const void* p, size_t bytes) {      // append a piece on a 16-byte boundary
  const size_t off = (tab.size() + 15) / 16 * 16;
  tab.resize(off + bytes);
  if (bytes) std::memcpy(tab.data() + off, p, bytes);
  return off;
}

// running sizes over the levels (a level's kcap uses the cell capacity of the levels up to it)
struct PlanSizes {
  long long pyr_off = 0, blur_off = 0;
  int key_off = 0, tile_w = 8, tile_h = 8, cell_cap = 1, max_cells = 1, node_cap = MAX_INI + 8, sel_cap = 8, desc_blocks = 0;
};

// ---- step 1: size, pitches, detection window and FAST cell grid of level l (src/ORBextractor.cc:773-787, :1112)
inline int plan_level_cells(const ExtractorParams& P, int l, int w, int h, int stride, ExtractorPlan& out, PlanSizes& S, const char** why) {
  LevelDev& L = out.G.lv[l];
  float s = P.inv_scale[l];
  L.w = cv_round((float)w * s); L.h = cv_round((float)h * s);
  ORBHIP_PLAN_REQUIRE(L.w >= 1 && L.h >= 1, "image too small for the requested number of pyramid levels");
  L.pitch = (l == 0) ? stride : round_up(L.w, 64);
  L.bpitch = round_up(L.w, 64);
  L.pyr_off = S.pyr_off; if (l > 0) S.pyr_off += (long long)L.pitch * L.h;
  L.blur_off = S.blur_off; S.blur_off += (long long)L.bpitch * L.h;
  L.scale = P.scale[l];
  L.patch = (float)(int)(PATCH_SIZE * P.scale[l]);                 // :837
  L.quota = P.quota[l];
  const int minBX = EDGE_THRESHOLD - 3, minBY = minBX;
  const int maxBX = L.w - EDGE_THRESHOLD + 3, maxBY = L.h - EDGE_THRESHOLD + 3;
  L.minBX = minBX; L.minBY = minBY; L.winW = maxBX - minBX; L.winH = maxBY - minBY;
  const float W = 30;
  const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
  const int nCols = (int)(width / W), nRows = (int)(height / W);
  L.cell_begin = (int)out.cells.size();
  if (nCols >= 1 && nRows >= 1) {
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    for (int i = 0; i < nRows; i++) {
      const float iniY = (float)(minBY + i * hCell);
      float maxY = iniY + hCell + 6;
      if (iniY >= maxBY - 3) continue;
      if (maxY > maxBY) maxY = (float)maxBY;
      for (int j = 0; j < nCols; j++) {
        const float iniX = (float)(minBX + j * wCell);
        float maxX = iniX + wCell + 6;
        if (iniX >= maxBX - 6) continue;
        if (maxX > maxBX) maxX = (float)maxBX;
        CellDesc cd;
        cd.level = (short)l; cd.x0 = (short)iniX; cd.y0 = (short)iniY; cd.x1 = (short)maxX; cd.y1 = (short)maxY;
        cd.offx = (short)(j * wCell); cd.offy = (short)(i * hCell); cd.pad = 0;
        out.cells.push_back(cd);
        int tw = cd.x1 - cd.x0, th = cd.y1 - cd.y0;
        S.tile_w = std::max(S.tile_w, tw); S.tile_h = std::max(S.tile_h, th);
        int iw = std::max(tw - 6, 0), ih = std::max(th - 6, 0);
        S.cell_cap = std::max(S.cell_cap, ((iw + 1) / 2) * ((ih + 1) / 2));
      }
    }
  }
  L.ncells = (int)out.cells.size() - L.cell_begin;
  S.max_cells = std::max(S.max_cells, L.ncells);
  return 0;
}

// ---- step 2: octree initial nodes (:543-563) and the capacities that follow from the quota and the cells of level l
inline int plan_level_octree(LevelDev& L, int keycap_max, PlanSizes& S, const char** why) {
  // (levels too small to hold a cell produce no candidates; the reference divides by zero there)
  int nIni = (L.ncells > 0) ? (int)std::round(static_cast<float>(L.winW) / L.winH) : 1;
  if (nIni < 1) nIni = 1;
  ORBHIP_PLAN_REQUIRE(nIni <= MAX_INI, "aspect ratio too extreme (more than 64 initial octree nodes)");
  L.nIni = nIni;
  L.hX = (L.ncells > 0) ? static_cast<float>(L.winW) / nIni : 1.0f;
  for (int i = 0; i <= nIni; i++) L.ini_x[i] = (int)(L.hX * static_cast<float>(i));
  S.node_cap = std::max(S.node_cap, std::max(L.quota + 8, 4 * nIni + 8));
  S.sel_cap = std::max(S.sel_cap, std::max(L.quota + 4, 4 * nIni + 4));   // the first octree sweep can return 4 * nIni > N nodes
  L.dblk_begin = S.desc_blocks; L.dblk_count = (std::max(L.quota + 4, 4 * nIni + 4) + 2 * DESC_WPB - 1) / (2 * DESC_WPB); S.desc_blocks += L.dblk_count;
  const long long theo = (long long)L.ncells * S.cell_cap;
  L.kcap = (int)std::min<long long>(std::max<long long>(theo, 64), keycap_max);
  L.key_off = S.key_off; S.key_off += round_up(L.kcap, 4);
  return 0;
}

// ---- step 3: cv::resize INTER_LINEAR tables of one level from the level below: source index and the two fixed-point
// weights (0 .. 2048) per output column / row
struct ResizeTables { std::vector<int> xofs, yofs; std::vector<short> ia, ib; };
inline ResizeTables linear_resize_tables(int sw, int sh, int dw, int dh) {
  ResizeTables T;
  const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
  const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
  T.xofs.resize(dw); T.yofs.resize(dh); T.ia.resize(2 * (size_t)dw); T.ib.resize(2 * (size_t)dh);
  auto sat = [](int v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); };
  for (int dx = 0; dx < dw; dx++) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = (int)std::floor(fx);
    fx -= sx;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    T.xofs[dx] = sx;
    T.ia[2 * dx] = sat(cv_round((1.f - fx) * 2048)); T.ia[2 * dx + 1] = sat(cv_round(fx * 2048));
  }
  for (int dy = 0; dy < dh; dy++) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = (int)std::floor(fy);
    fy -= sy;
    T.yofs[dy] = sy;
    T.ib[2 * dy] = sat(cv_round((1.f - fy) * 2048)); T.ib[2 * dy + 1] = sat(cv_round(fy * 2048));
  }
  return T;
}
// k_resize / k_pyr_cone read them as xtab[dx] = {sx | a0 << 16, a0 | a1 << 16}, yofs[dy], ibeta[2 dy .. 2 dy + 1]
inline void push_linear_tables(const ResizeTables& T, int l, ExtractorPlan& out) {
  const int dw = (int)T.xofs.size();
  const int dw4 = round_up(dw, 4);                      // padded with copies of the last column: a thread reads its 4 entries as two 16-byte loads
  std::vector<uint32_t> xt(2 * (size_t)dw4);
  for (int dx4 = 0; dx4 < dw4; dx4++) {
    const int dx = std::min(dx4, dw - 1);
    xt[2 * dx4] = (uint32_t)(T.xofs[dx] & 0xFFFF) | ((uint32_t)(uint16_t)T.ia[2 * dx] << 16);
    xt[2 * dx4 + 1] = (uint32_t)(uint16_t)T.ia[2 * dx] | ((uint32_t)(uint16_t)T.ia[2 * dx + 1] << 16);   // both weights, v_dot2 operand order
  }
  out.tab_xofs[l] = tab_push(out.tab, xt.data(), xt.size() * 4);
  out.tab_yofs[l] = tab_push(out.tab, T.yofs.data(), T.yofs.size() * 4);
  out.tab_ibeta[l] = tab_push(out.tab, T.ib.data(), T.ib.size() * 2);
}

// ---- step 4: k_resize_mfma's tables (see the kernel): per 48-column chunk the weight digits as MFMA A operands + the accumulator
// start values, per source row the output row it is sy0 of.  A level takes the kernel when the three conditions below hold.
// the origin of every 48-column chunk: its first source column, rounded down to a multiple of 4
inline std::vector<int> rm_chunk_origins(const ResizeTables& T) {
  std::vector<int> c0((T.xofs.size() + 47) / 48);
  for (size_t t = 0; t < c0.size(); t++) c0[t] = T.xofs[48 * t] & ~3;
  return c0;
}
// a chunk's source columns, counted from its origin, are the K index 0 .. 63 of one MFMA (true for scale factors up to ~1.3)
inline bool rm_chunks_fit(const ResizeTables& T, int sw, const std::vector<int>& c0) {
  const int dw = (int)T.xofs.size();
  for (size_t t = 0; t < c0.size(); t++) {
    const int hi = std::min(T.xofs[std::min((int)(48 * t + 47), dw - 1)] + 1, sw - 1);
    if (hi - c0[t] > 63) return false;
  }
  return true;
}
// a source row is sy0 of at most one output row, and the row table is indexed by it (true for every downscale)
inline bool rm_rows_ascend(const std::vector<int>& yofs) {
  for (size_t dy = 0; dy < yofs.size(); dy++) if (yofs[dy] < 0 || (dy > 0 && yofs[dy] <= yofs[dy - 1])) return false;
  return true;
}
// a weight is two int8 digits, 32 ah + al
inline bool rm_weights_fit(const std::vector<short>& wgt) {
  for (short v : wgt) if (v < 0 || v > 2048) return false;
  return true;
}
inline RmHost plan_resize_mfma(const ResizeTables& T, int sw, std::vector<uint8_t>& tab) {
  RmHost M;
  const int dw = (int)T.xofs.size(), dh = (int)T.yofs.size();
  const int nchunks = (dw + 47) / 48;
  const std::vector<int> c0 = rm_chunk_origins(T);
  if (!(rm_chunks_fit(T, sw, c0) && rm_rows_ascend(T.yofs) && rm_weights_fit(T.ia) && rm_weights_fit(T.ib))) return M;
  std::vector<int8_t> W((size_t)nchunks * 6 * 64 * 16, 0);
  std::vector<int32_t> Cc((size_t)nchunks * 3 * 16, 0);
  for (int t = 0; t < nchunks; t++)
    for (int cb = 0; cb < 3; cb++)
      for (int m = 0; m < 16; m++) {
        const int dx = 48 * t + 12 * (m >> 2) + 4 * cb + (m & 3);
        if (dx >= dw) continue;
        const int s0 = T.xofs[dx], s1 = std::min(T.xofs[dx] + 1, sw - 1);
        const int wgt[2] = {T.ia[2 * dx], T.ia[2 * dx + 1]}, col[2] = {s0, s1};
        Cc[((size_t)t * 3 + cb) * 16 + m] = 128 * (wgt[0] + wgt[1]);
        for (int e = 0; e < 2; e++) {
          const int k = col[e] - c0[t];                       // (0 .. 63: rm_chunks_fit)
          const size_t lane = (size_t)m + 16 * (k >> 4), byte = (size_t)(k & 15);
          int8_t* wh = &W[(((size_t)t * 6 + 2 * cb) * 64 + lane) * 16 + byte];
          int8_t* wl = &W[(((size_t)t * 6 + 2 * cb + 1) * 64 + lane) * 16 + byte];
          // (s1 == s0 at the right border: the two weights meet in one column and add up - a1 is 0 there)
          const int tot = 32 * (int)*wh + (int)*wl + wgt[e];
          *wh = (int8_t)(tot >> 5); *wl = (int8_t)(tot & 31);
        }
      }
  const int smax = T.yofs[dh - 1], nblocks = (smax + 1 + 14) / 15;
  std::vector<uint32_t> rowtab(2 * ((size_t)15 * nblocks + 1), 0);
  for (size_t s2 = 0; s2 < rowtab.size() / 2; s2++) rowtab[2 * s2] = 0xFFFFFFFFu;        // dy = -1
  for (int dy = 0; dy < dh; dy++) {
    rowtab[2 * (size_t)T.yofs[dy]] = (uint32_t)dy;
    rowtab[2 * (size_t)T.yofs[dy] + 1] = (uint32_t)(uint16_t)T.ib[2 * dy] | ((uint32_t)(uint16_t)T.ib[2 * dy + 1] << 16);
  }
  M.oW = tab_push(tab, W.data(), W.size()); M.oC = tab_push(tab, Cc.data(), Cc.size() * 4);
  M.oC0 = tab_push(tab, c0.data(), c0.size() * 4); M.oRow = tab_push(tab, rowtab.data(), rowtab.size() * 4);
  M.nchunks = nchunks; M.nblocks = nblocks; M.ok = true;
  return M;
}

// ---- step 5: blur tiles of level l for the three launch shapes
inline void plan_blur_tiles(int l, const LevelDev& L, ExtractorPlan& out) {
  for (int ty = 0; ty < (L.h + BLUR_TH - 1) / BLUR_TH; ty++)
    for (int tx = 0; tx < (L.w + BLUR_TW - 1) / BLUR_TW; tx++) {
      BlurTile bt; bt.level = (short)l; bt.tx = (short)tx; bt.ty = (short)ty; bt.pad = 0;
      out.btiles.push_back(bt);
    }
  for (int ty = 0, nty = (L.h + BM_TH - 1) / BM_TH; ty < nty; ty += BM_RC)       // k_blur7_mfma: ty = first 58-row chunk, pad = chunks of the workgroup
    for (int tx = 0; tx < (L.w + BM_TW - 1) / BM_TW; tx++) {
      BlurTile bt; bt.level = (short)l; bt.tx = (short)tx; bt.ty = (short)ty; bt.pad = (short)std::min(BM_RC, nty - ty);
      out.mtiles.push_back(bt);
      for (int q = 0; q < bt.pad; q++) { BlurTile b1 = bt; b1.ty = (short)(ty + q); b1.pad = 1; out.mtiles1.push_back(b1); }
    }
}

// ---- step 6: k_pyr_cone - per 32 x 8 tile of the top level, the box it computes on every level (see the kernel)
// a thread loads one table entry per level above 0 (<= 256 columns and rows; CONE_TPB covers them) and CONE_SRC_PT bytes of level 0
inline bool cone_box_fits(int k, int bw, int bh) { return k >= 1 ? (bw <= 256 && bh <= 256) : (bw * bh <= CONE_TPB * CONE_SRC_PT); }
static const size_t CONE_LDS_MAX = 96 * 1024;
// the box [x0, x1) x [y0, y1) of level k that the box U = {ux0, uy0, ux1, uy1} of level k + 1 reads through its tables
inline void cone_source_box(const ResizeTables& T, const short* U, int Wu, int Wk, int Hk, int* x0, int* y0, int* x1, int* y1) {
  const std::vector<int>& xo = T.xofs; const std::vector<int>& yo = T.yofs;
  const int ux0 = U[0], ux1 = std::min<int>(U[2], Wu), uy0 = U[1], uy1 = U[3];
  auto cy = [&](int v) { return std::min(std::max(v, 0), Hk - 1); };
  int nx0 = xo[ux0], nx1 = std::min(xo[ux1 - 1] + 1, Wk - 1) + 1, ny0 = cy(yo[uy0]), ny1 = cy(yo[uy1 - 1] + 1) + 1;
  for (int y = uy0; y < uy1; y++) { ny0 = std::min(ny0, cy(yo[y])); ny1 = std::max(ny1, cy(yo[y] + 1) + 1); }
  for (int x = ux0; x < ux1; x++) { nx0 = std::min(nx0, xo[x]); nx1 = std::max(nx1, std::min(xo[x] + 1, Wk - 1) + 1); }
  *x0 = nx0; *x1 = nx1; *y0 = ny0; *y1 = ny1;
}
inline void plan_cone(const std::vector<ResizeTables>& T, ExtractorPlan& out) {
  const GeomDev& G = out.G;
  const int nl = G.nlevels;
  out.cone = ConePlan();
  if (!(nl >= 3 && nl <= CONE_MAXL)) return;
  const int top = nl - 1, TW = 32, TH = 8;
  const int ntx = (G.lv[top].w + TW - 1) / TW, nty = (G.lv[top].h + TH - 1) / TH;
  std::vector<short> boxes((size_t)ntx * nty * nl * 4);
  int buf0 = 0, bufk = 0; size_t tabmax = 0; bool ok = G.lv[0].w < 32000 && G.lv[0].h < 32000;
  for (int j = 0; j < nty && ok; j++)
    for (int i = 0; i < ntx && ok; i++) {
      short* Bx = &boxes[((size_t)j * ntx + i) * nl * 4];
      int bx0 = i * TW, by0 = j * TH, bx1 = std::min((i + 1) * TW, G.lv[top].w), by1 = std::min((j + 1) * TH, G.lv[top].h);
      size_t tb = 0;
      for (int k = top; k >= 0; k--) {
        const int Wk = G.lv[k].w, Hk = G.lv[k].h;
        if (k < top) {
          cone_source_box(T[k + 1], &Bx[4 * (k + 1)], G.lv[k + 1].w, Wk, Hk, &bx0, &by0, &bx1, &by1);      // what the box of level k + 1 reads from level k ...
          if (k >= 1) {                                       // ... and this workgroup's share of level k itself
            bx0 = std::min(bx0, (int)((long long)i * Wk / ntx)); bx1 = std::max(bx1, (int)((long long)(i + 1) * Wk / ntx));
            by0 = std::min(by0, (int)((long long)j * Hk / nty)); by1 = std::max(by1, (int)((long long)(j + 1) * Hk / nty));
          }
        }
        if (k >= 1) { bx0 &= ~3; bx1 = std::min(round_up(bx1, 4), round_up(Wk, 4)); }      // whole dwords, as k_resize stores them
        Bx[4 * k] = (short)bx0; Bx[4 * k + 1] = (short)by0; Bx[4 * k + 2] = (short)bx1; Bx[4 * k + 3] = (short)by1;
        const int bytes = (bx1 - bx0) * (by1 - by0);
        if (!cone_box_fits(k, bx1 - bx0, by1 - by0)) ok = false;
        if (k == 0) buf0 = std::max(buf0, bytes); else { bufk = std::max(bufk, bytes); tb += 8 * (size_t)(bx1 - bx0) + 16 * (size_t)(by1 - by0); }
      }
      tabmax = std::max(tabmax, tb);
    }
  buf0 = round_up(buf0, 16); bufk = round_up(bufk, 16);
  const size_t lds = (size_t)buf0 + 2 * (size_t)bufk + tabmax + 64;
  if (!(ok && lds <= CONE_LDS_MAX)) return;
  out.cone.tab = tab_push(out.tab, boxes.data(), boxes.size() * 2);
  out.cone.wgs = ntx * nty; out.cone.buf0 = buf0; out.cone.bufk = bufk; out.cone.lds = lds;
}

// ---- step 7: totals and the LDS sizes of k_fast_cells and k_octree
inline void plan_totals(const PlanSizes& S, ExtractorPlan& out) {
  GeomDev& G = out.G;
  G.ncells_total = (int)out.cells.size();
  G.cell_cap = S.cell_cap; G.sel_cap = S.sel_cap; G.keys_per_frame = S.key_off; G.desc_blocks = S.desc_blocks;
  G.tile_w = S.tile_w; G.tile_h = S.tile_h; G.tile_pitch = round_up(S.tile_w, 4) + 4;
  G.node_cap = round_up(S.node_cap, 8); G.max_cells_level = round_up(S.max_cells, 8);
  G.pyr_frame_bytes = (S.pyr_off + 255) / 256 * 256;
  G.blur_frame_bytes = (S.blur_off + 255) / 256 * 256;
  out.fast_narrow = S.tile_w - 6 <= 32;                      // every cell interior <= 32 px wide: k_fast_cells<true> (32-bit row masks)
  out.fast_lds = (size_t)round_up((int)((size_t)2 * round_up(G.tile_h * G.tile_pitch, 16) + 2 * 64 * (out.fast_narrow ? 4 : 8) + 16 + (size_t)2 * std::max(S.tile_w - 6, 1) * std::max(S.tile_h - 6, 1) + 16), 16);   // tile + score (u8) + row masks + queue counter + queue (u16)
  out.octree_wide = false;
  for (int l = 0; l < G.nlevels; l++) out.octree_wide = out.octree_wide || G.lv[l].kcap > 65535;
  out.octree_lds = octree_lds_bytes(G.node_cap, G.max_cells_level, false, false);
  out.octree_lds_wide = octree_lds_bytes(G.node_cap, G.max_cells_level, true, false);
  // node arrays beyond the LDS: both instantiations keep them in a global scratch row per (frame, level) instead (k_octree<.., true>)
  out.octree_gmem = (out.octree_wide ? out.octree_lds_wide : out.octree_lds) > 160 * 1024;
  out.octree_row = (size_t)round_up((int)octree_lds_bytes(G.node_cap, G.max_cells_level, true, true), 256);
}

// Everything the extractor needs for images of w x h with row stride `stride`.  keycap_max: KEYCAP_MAX, or the ORBHIP_KEYCAP test
// hook's lower bound.  0, or an ORBHIP_E* code with *why = a static message; *out is unspecified after an error.
inline int plan_extractor(const ExtractorParams& P, int w, int h, int stride, int keycap_max, ExtractorPlan* out, const char** why) {
  ORBHIP_PLAN_REQUIRE(w >= 2 * EDGE_THRESHOLD + 8 && h >= 2 * EDGE_THRESHOLD + 8, "image too small");
  ORBHIP_PLAN_REQUIRE(w <= 4095 && h <= 4095, "image larger than 4095 px per side");
  const int nl = P.nlevels;
  *out = ExtractorPlan();
  GeomDev& G = out->G;
  std::memset(&G, 0, sizeof(G));
  G.nlevels = nl;
  out->tab_xofs.assign(nl, 0); out->tab_yofs.assign(nl, 0); out->tab_ibeta.assign(nl, 0); out->rm.assign(nl, RmHost());
  PlanSizes S;
  std::vector<ResizeTables> T(nl);                 // (kept for the cone boxes)
  for (int l = 0; l < nl; l++) {
    LevelDev& L = G.lv[l];
    if (int rc = plan_level_cells(P, l, w, h, stride, *out, S, why)) return rc;
    if (int rc = plan_level_octree(L, keycap_max, S, why)) return rc;
    if (l > 0) {
      T[l] = linear_resize_tables(G.lv[l - 1].w, G.lv[l - 1].h, L.w, L.h);
      push_linear_tables(T[l], l, *out);
      out->rm[l] = plan_resize_mfma(T[l], G.lv[l - 1].w, out->tab);
    }
    plan_blur_tiles(l, L, *out);
  }
  const int tile_w = S.tile_w, tile_h = S.tile_h;      // (named so: the message quotes the condition, and its text is part of the error)
  ORBHIP_PLAN_REQUIRE(tile_w <= 64 && tile_h <= 64, "FAST cell larger than 64 px (unsupported image geometry)");
  plan_totals(S, *out);
  ORBHIP_PLAN_REQUIRE(G.node_cap <= 32760, "nfeatures too large: more than 32752 keypoints in one level (16-bit node indices)");
  plan_cone(T, *out);
  return 0;
}
#undef ORBHIP_PLAN_REQUIRE

}  // namespace orbhip
