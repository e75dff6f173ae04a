// Host check of the extractor's plan (csrc/orb_geometry.h): plans every shape the GPU tests and the bench use and a sweep around
// them, and asserts on each plan what the kernels of orb_extractor.hip take for granted.  No GPU, no HIP; built with
// -fsanitize=address,undefined by tests/test_extractor_plan.py, so an out-of-range index in the plan's own arithmetic stops it too.
#include "orb_geometry.h"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace orbhip;

static std::string g_case;
#define CHECK(cond)                                                                               \
  do {                                                                                            \
    if (!(cond)) { std::fprintf(stderr, "FAILED %s\n  %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

template <typename T> static const T* piece(const ExtractorPlan& P, size_t off) { return (const T*)(P.tab.data() + off); }

// ---- every piece of tab starts on a 16-byte boundary, ends inside tab, and no two overlap (they were appended in this order)
static void check_tab_layout(const ExtractorPlan& P) {
  const GeomDev& G = P.G;
  size_t end = 0;
  auto take = [&](size_t off, size_t bytes) { CHECK(off % 16 == 0); CHECK(off >= end); CHECK(off + bytes <= P.tab.size()); end = off + bytes; };
  for (int l = 1; l < G.nlevels; l++) {
    const int dw = G.lv[l].w, dh = G.lv[l].h;
    take(P.tab_xofs[l], 8 * (size_t)round_up(dw, 4)); take(P.tab_yofs[l], 4 * (size_t)dh); take(P.tab_ibeta[l], 4 * (size_t)dh);
    const RmHost& M = P.rm[l];
    if (!M.ok) continue;
    take(M.oW, (size_t)M.nchunks * 6 * 64 * 16); take(M.oC, (size_t)M.nchunks * 3 * 16 * 4); take(M.oC0, (size_t)M.nchunks * 4);
    take(M.oRow, 8 * ((size_t)15 * M.nblocks + 1));
  }
  if (P.cone.wgs > 0) take(P.cone.tab, (size_t)P.cone.wgs * G.nlevels * 4 * 2);
}

// ---- cells, capacities and offsets
static void check_levels(const ExtractorPlan& P, const ExtractorParams& prm, int w, int h, int stride, int keycap_max) {
  const GeomDev& G = P.G;
  CHECK(G.nlevels == prm.nlevels && G.ncells_total == (int)P.cells.size());
  CHECK(G.tile_w <= 64 && G.tile_h <= 64 && G.tile_pitch % 4 == 0 && G.tile_pitch >= G.tile_w + 3);
  CHECK(G.pyr_frame_bytes % 256 == 0 && G.blur_frame_bytes % 256 == 0);
  CHECK(G.node_cap % 8 == 0 && G.node_cap <= 32760 && G.max_cells_level % 8 == 0);
  CHECK(G.lv[0].w == w && G.lv[0].h == h && G.lv[0].pitch == stride);
  int cells_seen = 0, key_end = 0, dblk_end = 0; long long pyr_end = 0, blur_end = 0; bool wide = false;
  for (int l = 0; l < G.nlevels; l++) {
    const LevelDev& L = G.lv[l];
    CHECK(L.w >= 1 && L.h >= 1 && L.w <= 4095 && L.h <= 4095 && L.pitch >= L.w && L.bpitch >= L.w && L.quota == prm.quota[l]);
    if (l > 0) { CHECK(L.pyr_off >= pyr_end && L.pitch % 4 == 0); pyr_end = L.pyr_off + (long long)L.pitch * L.h; }
    CHECK(L.blur_off >= blur_end); blur_end = L.blur_off + (long long)L.bpitch * L.h;
    CHECK(L.cell_begin == cells_seen && L.ncells >= 0 && L.ncells <= G.max_cells_level);
    long long worst = 0;                                         // candidates the level's cells can hold after their 3 x 3 NMS
    for (int i = L.cell_begin; i < L.cell_begin + L.ncells; i++) {
      const CellDesc& c = P.cells[i];
      CHECK(c.level == l && 0 <= c.x0 && c.x0 < c.x1 && c.x1 <= L.w && 0 <= c.y0 && c.y0 < c.y1 && c.y1 <= L.h);
      CHECK(c.x0 == L.minBX + c.offx && c.y0 == L.minBY + c.offy && c.x1 <= L.minBX + L.winW && c.y1 <= L.minBY + L.winH);
      CHECK(c.x1 - c.x0 <= G.tile_w && c.y1 - c.y0 <= G.tile_h);
      const int iw = std::max(c.x1 - c.x0 - 6, 0), ih = std::max(c.y1 - c.y0 - 6, 0), cap = ((iw + 1) / 2) * ((ih + 1) / 2);
      CHECK(cap <= G.cell_cap);
      worst += cap;
    }
    cells_seen += L.ncells;
    CHECK(L.kcap >= 64 && L.kcap <= keycap_max && L.kcap >= std::min<long long>(worst, keycap_max));
    CHECK(L.key_off % 4 == 0 && L.key_off >= key_end); key_end = L.key_off + L.kcap;
    wide = wide || L.kcap > 65535;
    CHECK(L.nIni >= 1 && L.nIni <= MAX_INI && L.ini_x[0] == 0 && L.ini_x[L.nIni] <= std::max(L.winW, 1));
    for (int i = 0; i < L.nIni; i++) CHECK(L.ini_x[i] <= L.ini_x[i + 1]);
    const int out_cap = std::max(L.quota + 4, 4 * L.nIni + 4);   // what the octree can select on this level
    CHECK(G.sel_cap >= out_cap && G.node_cap >= out_cap + 4);
    CHECK(L.dblk_begin == dblk_end && L.dblk_count * 2 * DESC_WPB >= out_cap); dblk_end += L.dblk_count;
  }
  CHECK(cells_seen == G.ncells_total && key_end <= G.keys_per_frame && dblk_end == G.desc_blocks);
  CHECK(pyr_end <= G.pyr_frame_bytes && blur_end <= G.blur_frame_bytes);
  CHECK(P.octree_wide == wide && P.fast_narrow == (G.tile_w - 6 <= 32) && P.fast_lds % 16 == 0 && P.fast_lds <= 64 * 1024);
  CHECK(P.octree_lds >= octree_lds_bytes(G.node_cap, G.max_cells_level, false, false) && P.octree_lds_wide >= P.octree_lds);
  CHECK(P.octree_gmem == ((wide ? P.octree_lds_wide : P.octree_lds) > 160 * 1024));
  CHECK(P.octree_row % 256 == 0 && P.octree_row >= octree_lds_bytes(G.node_cap, G.max_cells_level, true, true));
}

static void check_blur_tiles(const ExtractorPlan& P) {
  const GeomDev& G = P.G;
  size_t nb = 0, nm1 = 0;
  for (int l = 0; l < G.nlevels; l++) {
    nb += (size_t)((G.lv[l].w + BLUR_TW - 1) / BLUR_TW) * ((G.lv[l].h + BLUR_TH - 1) / BLUR_TH);
    nm1 += (size_t)((G.lv[l].w + BM_TW - 1) / BM_TW) * ((G.lv[l].h + BM_TH - 1) / BM_TH);
  }
  CHECK(P.btiles.size() == nb && P.mtiles1.size() == nm1);
  for (const BlurTile& t : P.btiles) CHECK(t.level >= 0 && t.level < G.nlevels && t.tx * BLUR_TW < G.lv[t.level].w && t.ty * BLUR_TH < G.lv[t.level].h);
  size_t chunks = 0;
  for (const BlurTile& t : P.mtiles) {
    CHECK(t.level >= 0 && t.level < G.nlevels && t.pad >= 1 && t.pad <= BM_RC && t.ty % BM_RC == 0);
    CHECK(t.tx * BM_TW < G.lv[t.level].w && (t.ty + t.pad - 1) * BM_TH < G.lv[t.level].h);
    chunks += t.pad;
  }
  CHECK(chunks == nm1);
  for (const BlurTile& t : P.mtiles1) CHECK(t.pad == 1 && t.tx * BM_TW < G.lv[t.level].w && t.ty * BM_TH < G.lv[t.level].h);
}

// ---- the linear tables of level l as the kernels read them; returns xofs / yofs for the checks below
struct Linear { std::vector<int> xofs, yofs, a0, a1, b0, b1; };
static Linear check_linear(const ExtractorPlan& P, int l) {
  const LevelDev& S = P.G.lv[l - 1]; const LevelDev& D = P.G.lv[l];
  const uint32_t* xt = piece<uint32_t>(P, P.tab_xofs[l]); const int* yo = piece<int>(P, P.tab_yofs[l]); const short* ib = piece<short>(P, P.tab_ibeta[l]);
  Linear T;
  for (int dx4 = 0; dx4 < round_up(D.w, 4); dx4++) {
    const int sx = (int)(xt[2 * dx4] & 0xFFFF), a0 = (int)(xt[2 * dx4 + 1] & 0xFFFF), a1 = (int)(xt[2 * dx4 + 1] >> 16);
    CHECK(sx >= 0 && sx <= S.w - 1 && (int)(xt[2 * dx4] >> 16) == a0);
    CHECK(sx < S.w - 1 || a1 == 0);                              // (the clamped second column never matters)
    if (dx4 < D.w) { T.xofs.push_back(sx); T.a0.push_back((short)a0); T.a1.push_back((short)a1); }
    else CHECK(sx == T.xofs.back());                             // padding: copies of the last column
  }
  for (int dy = 0; dy < D.h; dy++) { T.yofs.push_back(yo[dy]); T.b0.push_back(ib[2 * dy]); T.b1.push_back(ib[2 * dy + 1]); CHECK(yo[dy] >= -1 && yo[dy] <= S.h - 1); }
  return T;
}

// ---- a level that takes k_resize_mfma
static void check_resize_mfma(const ExtractorPlan& P, int l, const Linear& T) {
  const RmHost& M = P.rm[l];
  const int sw = P.G.lv[l - 1].w, dw = P.G.lv[l].w, dh = P.G.lv[l].h;
  CHECK(M.nchunks == (dw + 47) / 48);
  const int8_t* W = piece<int8_t>(P, M.oW); const int32_t* Cc = piece<int32_t>(P, M.oC); const int* c0 = piece<int>(P, M.oC0); const uint32_t* row = piece<uint32_t>(P, M.oRow);
  size_t placed = 0;                                             // non-zero digits where the weights belong
  for (int dx = 0; dx < dw; dx++) {
    CHECK(T.a0[dx] >= 0 && T.a0[dx] <= 2048 && T.a1[dx] >= 0 && T.a1[dx] <= 2048);
    const int t = dx / 48, r = dx % 48, m = 4 * (r / 12) + (r & 3), cb = (r % 12) / 4;      // dx = 48 t + 12 (m >> 2) + 4 cb + (m & 3)
    const int s0 = T.xofs[dx], s1 = std::min(s0 + 1, sw - 1);
    CHECK(c0[t] % 4 == 0 && c0[t] >= 0 && s0 - c0[t] >= 0 && s1 - c0[t] <= 63);
    CHECK(Cc[(t * 3 + cb) * 16 + m] == 128 * (T.a0[dx] + T.a1[dx]));
    auto digit = [&](int k, int lo) { return (int)W[(((size_t)t * 6 + 2 * cb + lo) * 64 + (size_t)m + 16 * (k >> 4)) * 16 + (k & 15)]; };
    auto weight = [&](int k) { CHECK(digit(k, 0) >= 0 && digit(k, 1) >= 0 && digit(k, 1) < 32); return 32 * digit(k, 0) + digit(k, 1); };
    if (s1 == s0) CHECK(weight(s0 - c0[t]) == T.a0[dx] + T.a1[dx]);
    else CHECK(weight(s0 - c0[t]) == T.a0[dx] && weight(s1 - c0[t]) == T.a1[dx]);
    placed += (digit(s0 - c0[t], 0) != 0) + (digit(s0 - c0[t], 1) != 0);
    if (s1 != s0) placed += (digit(s1 - c0[t], 0) != 0) + (digit(s1 - c0[t], 1) != 0);
  }
  size_t nonzero = 0;                                            // every digit anywhere else in the operand tables is zero
  for (size_t i = 0; i < (size_t)M.nchunks * 6 * 64 * 16; i++) nonzero += W[i] != 0;
  CHECK(nonzero == placed);
  CHECK(15 * M.nblocks > T.yofs[dh - 1]);
  std::vector<int> back(15 * (size_t)M.nblocks + 1, -1);
  for (int dy = 0; dy < dh; dy++) {
    CHECK(T.yofs[dy] >= 0 && (dy == 0 || T.yofs[dy] > T.yofs[dy - 1]));
    CHECK(T.b0[dy] >= 0 && T.b0[dy] <= 2048 && T.b1[dy] >= 0 && T.b1[dy] <= 2048);
    back[T.yofs[dy]] = dy;
    CHECK(row[2 * T.yofs[dy] + 1] == ((uint32_t)(uint16_t)T.b0[dy] | ((uint32_t)(uint16_t)T.b1[dy] << 16)));
  }
  for (size_t s = 0; s < back.size(); s++) CHECK((int)row[2 * s] == back[s]);
}

// ---- k_pyr_cone: box sizes, LDS layout, and every box holds what the box above it reads and its own share of the level
static void check_cone(const ExtractorPlan& P, const std::vector<Linear>& T) {
  const GeomDev& G = P.G; const ConePlan& C = P.cone;
  const int nl = G.nlevels, top = nl - 1, ntx = (G.lv[top].w + 31) / 32, nty = (G.lv[top].h + 7) / 8;
  CHECK(nl >= 3 && nl <= CONE_MAXL && C.wgs == ntx * nty && C.buf0 % 16 == 0 && C.bufk % 16 == 0 && C.lds <= 96 * 1024);
  const short* boxes = piece<short>(P, C.tab);
  for (int j = 0; j < nty; j++)
    for (int i = 0; i < ntx; i++) {
      const short* B = boxes + ((size_t)j * ntx + i) * nl * 4;
      size_t tb = 0;
      for (int k = 0; k < nl; k++) {
        const int x0 = B[4 * k], y0 = B[4 * k + 1], x1 = B[4 * k + 2], y1 = B[4 * k + 3], Wk = G.lv[k].w, Hk = G.lv[k].h;
        CHECK(0 <= x0 && x0 < x1 && 0 <= y0 && y0 < y1 && y1 <= Hk && x1 <= (k ? round_up(Wk, 4) : Wk));
        if (k == 0) { CHECK((x1 - x0) * (y1 - y0) <= CONE_TPB * CONE_SRC_PT && (x1 - x0) * (y1 - y0) <= C.buf0); }
        else {
          CHECK(x1 - x0 <= 256 && y1 - y0 <= 256 && x0 % 4 == 0 && (x1 - x0) % 4 == 0 && (x1 - x0) * (y1 - y0) <= C.bufk);
          CHECK(x1 <= G.lv[k].pitch);                            // whole dwords are stored
          tb += 8 * (size_t)(x1 - x0) + 16 * (size_t)(y1 - y0);
        }
        // its share of the level (the top level: its 32 x 8 tile): the shares of all workgroups tile the level, so every pixel is written
        if (k == top) { CHECK(x0 <= 32 * i && std::min(x1, Wk) >= std::min(32 * (i + 1), Wk) && y0 <= 8 * j && y1 >= std::min(8 * (j + 1), Hk)); continue; }
        if (k >= 1) {
          CHECK(x0 <= (int)((long long)i * Wk / ntx) && std::min(x1, Wk) >= (int)((long long)(i + 1) * Wk / ntx));
          CHECK(y0 <= (int)((long long)j * Hk / nty) && y1 >= (int)((long long)(j + 1) * Hk / nty));
        }
        // what the box of level k + 1 reads from level k, with the kernel's clamping
        const short* U = B + 4 * (k + 1); const Linear& L = T[k + 1];
        for (int x = U[0]; x < std::min<int>(U[2], G.lv[k + 1].w); x++) CHECK(L.xofs[x] >= x0 && std::min(L.xofs[x] + 1, Wk - 1) < x1);
        for (int y = U[1]; y < U[3]; y++) {
          const int sy0 = std::min(std::max(L.yofs[y], 0), Hk - 1), sy1 = std::min(std::max(L.yofs[y] + 1, 0), Hk - 1);
          CHECK(sy0 >= y0 && sy0 < y1 && sy1 >= y0 && sy1 < y1);
        }
      }
      CHECK((size_t)C.buf0 + 2 * (size_t)C.bufk + tb <= C.lds);
    }
}

struct Tally { int plans = 0, rejected = 0, mfma = 0, valu = 0, cones = 0, wide = 0, gmem = 0; };

// plan one configuration; every accepted plan goes through all checks
static int plan_and_check(int w, int h, int stride, int nl, double sf, int nfeatures, int keycap_max, Tally* tally, std::string* why_out = nullptr) {
  char name[160]; std::snprintf(name, sizeof(name), "%dx%d stride %d, %d levels, scale %.2f, %d features, keycap %d", w, h, stride, nl, sf, nfeatures, keycap_max);
  g_case = name;
  const ScaleTables S = scale_tables(nfeatures, sf, nl);
  const ExtractorParams prm = {nl, S.inv_scale.data(), S.scale.data(), S.quota.data()};
  ExtractorPlan P; const char* why = nullptr;
  const int rc = plan_extractor(prm, w, h, stride, keycap_max, &P, &why);
  if (rc) { CHECK(rc == ORBHIP_EINVAL && why && why[0]); if (why_out) *why_out = why; if (tally) tally->rejected++; return rc; }
  check_tab_layout(P);
  check_levels(P, prm, w, h, stride, keycap_max);
  check_blur_tiles(P);
  std::vector<Linear> T(nl);
  for (int l = 1; l < nl; l++) {
    T[l] = check_linear(P, l);
    if (P.rm[l].ok) check_resize_mfma(P, l, T[l]);
    if (tally) (P.rm[l].ok ? tally->mfma : tally->valu)++;
  }
  if (P.cone.wgs > 0) check_cone(P, T);
  if (tally) { tally->plans++; tally->cones += P.cone.wgs > 0; tally->wide += P.octree_wide; tally->gmem += P.octree_gmem; }
  return 0;
}

static void expect_error(int w, int h, int nl, double sf, int nfeatures, const char* text) {
  std::string why;
  const int rc = plan_and_check(w, h, w, nl, sf, nfeatures, KEYCAP_MAX, nullptr, &why);
  CHECK(rc == ORBHIP_EINVAL && why.find(text) != std::string::npos);
}

int main() {
  const int SMALL = 2 * EDGE_THRESHOLD + 8;
  const int sizes[][3] = {{640, 480, 640}, {752, 480, 752}, {1241, 376, 1241}, {1241, 376, 1280}, {1920, 1080, 1920}, {1000, 1000, 1000},
                          {1200, 1200, 1200}, {1500, 700, 1500}, {700, 500, 700}, {480, 640, 480}, {SMALL, 480, SMALL}, {640, SMALL, 640}, {SMALL, SMALL, 64}};
  const int levels[] = {1, 3, 4, 8, 16};
  const double factors[] = {1.2, 1.1, 1.5, 2.0};
  const int features[] = {500, 1000, 2000, 3000, 8000, 15000, 30000};
  const int NS = sizeof(sizes) / sizeof(sizes[0]), NL = sizeof(levels) / sizeof(int), NF = sizeof(factors) / sizeof(double), NN = sizeof(features) / sizeof(int);
  Tally t;
  for (int i = 0; i < NS * NL * NF * NN; i++) {                  // mixed radix over the four lists: every combination
    const int* s = sizes[i % NS];
    plan_and_check(s[0], s[1], s[2], levels[i / NS % NL], factors[i / (NS * NL) % NF], features[i / (NS * NL * NF)], KEYCAP_MAX, &t);
  }
  // the ORBHIP_KEYCAP test hook's range
  for (int keycap : {64, 1000, 65535, 65536}) plan_and_check(640, 480, 640, 8, 1.2, 1000, keycap, &t);
  g_case = "sweep totals";
  CHECK(t.plans > 3 * t.rejected && t.mfma > 0 && t.valu > 0 && t.cones > 0 && t.wide > 0 && t.gmem > 0);      // the sweep reached every path
  // the benchmarked configuration: every level on k_resize_mfma, a cone for the lone frame
  {
    const ScaleTables S = scale_tables(2000, 1.2, 8);
    const ExtractorParams prm = {8, S.inv_scale.data(), S.scale.data(), S.quota.data()};
    ExtractorPlan P; const char* why = nullptr;
    g_case = "1241x376, 8 levels, scale 1.2, 2000 features";
    CHECK(plan_extractor(prm, 1241, 376, 1241, KEYCAP_MAX, &P, &why) == 0 && P.cone.wgs > 0 && !P.octree_gmem);
    for (int l = 1; l < 8; l++) CHECK(P.rm[l].ok);
  }
  // the four argument errors come back as errors
  expect_error(SMALL - 1, 480, 8, 1.2, 1000, "image too small");
  expect_error(640, SMALL - 1, 8, 1.2, 1000, "image too small");
  expect_error(4096, 480, 8, 1.2, 1000, "image larger than 4095 px per side");
  expect_error(640, 4096, 8, 1.2, 1000, "image larger than 4095 px per side");
  expect_error(SMALL, SMALL, 16, 2.0, 1000, "image too small for the requested number of pyramid levels");
  expect_error(4095, 62, 1, 1.2, 1000, "aspect ratio too extreme");
  std::printf("extractor plan: %d plans checked (%d rejected), %d levels on k_resize_mfma, %d on k_resize, %d cones, %d wide, %d gmem\n",
              t.plans, t.rejected, t.mfma, t.valu, t.cones, t.wide, t.gmem);
  return 0;
}
