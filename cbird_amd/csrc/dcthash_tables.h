// dcthash_tables.h -- the host half of the image hash that needs no device: the INTER_AREA tables and what dcthash.hip
// derives from them (the y table seen from a source row, the column strips of wide images, k_band_area's strips and band
// matrices, k_dcthash_256_band's B operand), and the sizing rules of the k_blur_area_regs strips.  Plain C++17, no HIP
// header: tests/cpp/hash_tables.cpp compiles it alone with the host compiler.  The entry types that kernel signatures
// mention keep the namespaces they had in dcthash.hip / dcthash_common.h, the anonymous one included.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace cbh {

struct AreaTab {
  int si, di;
  float alpha;
};
// the y table of make_area_tab seen from a SOURCE row (k_blur_area_regs<.., FUSE>): a row contributes to one or two
// consecutive output rows (scale >= 1).  info: bits 0..7 di of the first entry, bit 8 = that entry opens its cell,
// bit 9 = it closes it, bit 10 = a second entry exists (cell di + 1), bit 11 / 12 = opens / closes for that one
// k0 = 0.f when the first entry opens its cell, 1.f when it continues one: sum = fma(sum, k0, a0 * v) is `t0` or `sum + t0`
// (one rounding either way) without a select (k_band_area)
struct YRow {
  float a0, a1;
  int info;
  float k0;
};

namespace {

struct BandTables {
  unsigned int w[1][64][4];  // the B operand (i8 x 16 per lane) of an interior column tile: the only one (see "borders")
};

struct BaStrip {
  int xs;       // first source column of the strip's first cell
  int T;        // 16-column tiles (<= 15)
  int cell0;    // first output cell
  int ncell;    // cells (<= 16)
  int amax;     // longest cell walk
  int amin;     // shortest: entries 1 .. amin - 2 of EVERY cell weigh its wmid (checked on the host)
  int tp;       // dwords between the images' planes of sT: chosen on the host so that the cells' walks (lane = image, cell
                // reads column si0[cell] + k of its image's plane) meet in as few LDS banks as possible
  int rotm;     // integer ratios with 16 or 32 columns per cell (512, 1024 px): cell width - 1, else 0 -- see rot
  int si0[16];             // first source column of cell c, relative to xs
  // the block-sum walk of cell c starts at its column rot[c] and wraps (a sum has no order): cells a multiple of 16 columns
  // apart would otherwise read the same LDS bank in every step of the walk, 8 lanes a bank at 512 px
  int rot[16];
  // weights of cell c in table order: wfirst, then wmid for entries 1 .. amin - 2, then wtail[j] for entry amin - 1 + j
  // (+0.0f past the cell's end; amax - amin + 1 <= 4 of them)
  float wfirst[16], wmid[16], wtail[16][4];
  unsigned band[3][64][4]; // B operands: the plain band, the strip's first tile, its last tile
};

// Row bands: a small batch has too few (group, strip) pairs to fill the machine (256 frames of 1920 x 1080: 512 waves for 2560
// slots, each walking 270 steps), so the 32 output ROWS are dealt to up to 8 waves per (group, strip) as well: band b makes
// the output rows [c0, c1) and walks the source rows [ra, rb] that feed them (+ two warm-up steps for the blur's seven-row
// window; a source row that straddles two bands' cells is walked by both).
struct BaBands {
  int n;
  int ra[8], rb[8], c0[8], c1[8];
};

}  // namespace

// computeResizeAreaTab (OpenCV 2.4 imgwarp.cpp, as recalled): see oracle/cbird_oracle.c for the prose
// cv::resize: inv_scale = (double)dsize/ssize; scale = 1./inv_scale (two roundings -- it is not ssize/dsize), and the
// integer "area fast" path only when |scale - round(scale)| < DBL_EPSILON on both axes: for ssize = 32*m with
// m = 49, 93, 98, 99, 103 ... the double rounding misses m by an ulp and the weighted tables are used instead.
inline double cv_resize_scale(int ssize, int dsize) {
  const double inv_scale = (double)dsize / ssize;
  return 1. / inv_scale;
}
// cv::resize takes its integer-ratio INTER_AREA path for this geometry
inline bool area_fast(int w, int h) {
  const double sx = cv_resize_scale(w, 32), sy = cv_resize_scale(h, 32);
  return std::fabs(sx - std::nearbyint(sx)) < DBL_EPSILON && std::fabs(sy - std::nearbyint(sy)) < DBL_EPSILON;
}

inline std::vector<AreaTab> make_area_tab(int ssize, int dsize, std::vector<int>* first) {
  std::vector<AreaTab> tab;
  const double scale = cv_resize_scale(ssize, dsize);
  first->assign((size_t)dsize + 1, 0);
  for (int dx = 0; dx < dsize; dx++) {
    (*first)[(size_t)dx] = (int)tab.size();
    const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
    const double cellWidth = std::min(scale, ssize - fsx1);
    int sx1 = (int)__builtin_ceil(fsx1), sx2 = (int)__builtin_floor(fsx2);
    sx2 = std::min(sx2, ssize - 1);
    sx1 = std::min(sx1, sx2);
    if (sx1 - fsx1 > 1e-3) tab.push_back(AreaTab{sx1 - 1, dx, (float)((sx1 - fsx1) / cellWidth)});
    for (int sx = sx1; sx < sx2; sx++) tab.push_back(AreaTab{sx, dx, (float)(1.0 / cellWidth)});
    if (fsx2 - sx2 > 1e-3)
      tab.push_back(AreaTab{sx2, dx, (float)(std::min(std::min(fsx2 - sx2, 1.), cellWidth) / cellWidth)});
  }
  (*first)[(size_t)dsize] = (int)tab.size();
  return tab;
}

inline int reflect101_host(int p, int len) {
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
  return p;
}

constexpr int kYRowPad = 8;

// The YRow rows of the y table (yt, yf) = make_area_tab(h, 32): h entries with kYRowPad neutral entries before and behind
// them (k_band_area reads the four rows of a step without clamping their indices); empty when some source row has more
// than two entries (never for h >= 32).
inline std::vector<YRow> make_yrows(int h, const std::vector<AreaTab>& yt, const std::vector<int>& yf) {
  std::vector<YRow> yr_all((size_t)h + 2 * kYRowPad, YRow{0.f, 0.f, 0, 1.f});
  YRow* const yr = yr_all.data() + kYRowPad;
  std::vector<int> cnt((size_t)h, 0);
  bool ok = true;
  for (size_t j = 0; j < yt.size() && ok; ++j) {
    const AreaTab& en = yt[j];
    if (en.si < 0 || en.si >= h || en.di < 0 || en.di > 31) {
      ok = false;
      break;
    }
    const bool opens = (int)j == yf[(size_t)en.di], closes = (int)j + 1 == yf[(size_t)en.di + 1];
    YRow& r = yr[(size_t)en.si];
    if (cnt[(size_t)en.si] == 0) {
      r.a0 = en.alpha;
      r.info = en.di | (opens ? 0x100 : 0) | (closes ? 0x200 : 0);
      r.k0 = opens ? 0.f : 1.f;
    } else if (cnt[(size_t)en.si] == 1 && en.di == (r.info & 0xff) + 1) {
      r.a1 = en.alpha;
      r.info |= 0x400 | (opens ? 0x800 : 0) | (closes ? 0x1000 : 0);
    } else {
      ok = false;
    }
    cnt[(size_t)en.si]++;
  }
  for (int y = 0; y < h && ok; ++y) ok = cnt[(size_t)y] >= 1;
  if (!ok) yr_all.clear();
  return yr_all;
}

// Column strips of an image wider than 2048 pixels (k_blur_area_regs spans a row with one workgroup of <= 256 lanes x 8
// columns): strip s of ncol makes the output cells [s * 32 / ncol, (s + 1) * 32 / ncol); it covers the source columns of
// exactly those cells (the blur's 3-pixel border comes from the parent through the view mechanism).
struct StripGeom {
  int x0 = 0, ws = 0;
  std::vector<AreaTab> x;   // fractional ratios: the cells' table entries, si relative to x0
  std::vector<int> xfirst;  // 33 entries
};
// integer: the image takes resizeAreaFast_ (both ratios integral, area_fast()): cells are whole pixel runs, no tables
inline StripGeom make_strip_geom(int w, bool integer, int ncol, int s) {
  const int cpw = 32 / ncol, c_lo = s * cpw, c_hi = c_lo + cpw;
  StripGeom d;
  if (integer) {
    d.x0 = c_lo * (w / 32);
    d.ws = cpw * (w / 32);
  } else {
    std::vector<int> xf;
    const std::vector<AreaTab> xt = make_area_tab(w, 32, &xf);
    const int e0 = xf[(size_t)c_lo], e1 = xf[(size_t)c_hi];
    d.x0 = xt[(size_t)e0].si;
    d.ws = xt[(size_t)e1 - 1].si + 1 - d.x0;
    d.x.assign(xt.begin() + e0, xt.begin() + e1);
    for (AreaTab& e : d.x) e.si -= d.x0, e.di -= c_lo;
    d.xfirst.resize(33);
    for (int c = 0; c <= 32; ++c) d.xfirst[(size_t)c] = xf[(size_t)std::min(c_lo + c, c_hi)] - e0;
  }
  return d;
}

namespace {

// Strips and band matrices of k_band_area for images of width w: n_strips >= 2 strips of cps = ceil(32 / n_strips) <= 16
// cells, each at most 240 source columns wide with cells of at most 32 table entries.  strips is empty when the geometry
// does not fit (the caller takes k_blur_area_regs).
struct BaStripList {
  std::vector<BaStrip> strips;
  int n_strips = 0, T = 0, amax = 0, RS = 4;
};

inline BaStripList make_ba_strips(int w) {
  BaStripList d;
  std::vector<int> xf;
  const std::vector<AreaTab> xt = make_area_tab(w, 32, &xf);
  std::vector<BaStrip>& host = d.strips;
  auto band_of = [&](int xs0, int c, bool plain, unsigned (*dst)[4]) {
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 16; ++j) {
        const int k = 16 * (l >> 4) + j, kk = k & 31;
        const int col = xs0 + 16 * c - 8 + kk, xo = xs0 + 16 * c + (l & 15);
        int wgt = 0;
        if (plain) {
          wgt = std::abs(col - xo) <= 3 ? 1 : 0;
        } else if (col >= 0 && col < w && xo < w) {
          for (int dd = -3; dd <= 3; ++dd) wgt += reflect101_host(xo + dd, w) == col;
        }
        if (k >= 32) wgt = -wgt;
        dst[l][j >> 2] |= (unsigned)(wgt & 0xff) << (8 * (j & 3));
      }
  };
  // cells per strip, in order of preference: 16 or 11 (a lane carries the four rows of a step: RS 4), 8 (two rows: RS 2),
  // 4 (one row: RS 1; w <= 1920).  Two cells per strip (w <= 3840) leave half the walk's lanes idle: measured 1.45 TB/s at
  // 3840 x 2160 against k_blur_area_regs' 2.6 -- not offered.
  // (fewer cells per strip than the geometry allows -- shorter rings, 15 instead of 10 waves per CU -- lose more to the
  // strips' halos than the occupancy returns: 400 x 300 2.92 -> 2.72 TB/s with 8 cells, 160 x 120 2.03 -> 1.42;
  // profiles/r06_band_area_cells_per_strip.txt)
  const int cps_try[4] = {16, 11, 8, 4};
  for (int ci = 0; ci < 4 && host.empty(); ++ci) {
    const int cps = cps_try[ci];
    bool ok = true;
    // one tile count for every strip: the widest strip's
    int Tc = 0;
    for (int c0 = 0; c0 < 32 && ok; c0 += cps) {
      const int c1 = std::min(32, c0 + cps);
      Tc = std::max(Tc, (xt[(size_t)xf[(size_t)c1] - 1].si + 1 - xt[(size_t)xf[(size_t)c0]].si + 15) / 16);
    }
    ok = ok && Tc >= 2 && Tc <= 15 && 16 * Tc + 8 <= w;
    if (!ok) continue;
    d.RS = cps > 8 ? 4 : cps == 8 ? 2 : 1;
    std::vector<BaStrip> cand;
    for (int c0 = 0; c0 < 32 && ok; c0 += cps) {
      const int c1 = std::min(32, c0 + cps);
      BaStrip b;
      memset(&b, 0, sizeof b);
      const int xs_cells = xt[(size_t)xf[(size_t)c0]].si;
      // the strip's tiles start at its first cell -- or further left, so that the LAST strip's tiles end exactly at
      // column w - 1 (then only its last tile sees the right edge) and no strip reaches past it
      b.xs = c0 == 0 ? 0 : std::min(xs_cells, w - 16 * Tc);
      b.T = Tc;
      b.cell0 = c0;
      b.ncell = c1 - c0;
      ok = b.xs == 0 || b.xs >= 8;
      if (c1 == 32) ok = ok && b.xs == w - 16 * Tc;
      for (int c = c0; c < c1 && ok; ++c) {
        const int e0 = xf[(size_t)c], e1 = xf[(size_t)c + 1];
        ok = e1 - e0 >= 2;
        b.amax = std::max(b.amax, e1 - e0);
        b.amin = c == c0 ? e1 - e0 : std::min(b.amin, e1 - e0);
        b.si0[c - c0] = xt[(size_t)e0].si - b.xs;
        ok = ok && b.si0[c - c0] >= 0 && b.si0[c - c0] + (e1 - e0) <= 16 * Tc;
        for (int e = e0; e < e1 && ok; ++e) {
          ok = xt[(size_t)e].si == xt[(size_t)e0].si + (e - e0) && xt[(size_t)e].di == c;  // consecutive columns, in order
        }
      }
      ok = ok && b.amax - b.amin + 1 <= 4;
      for (int c = c0; c < c1 && ok; ++c) {  // the walk's weights: first, mid (entries 1 .. amin - 2), tail
        const int e0 = xf[(size_t)c], nn = xf[(size_t)c + 1] - e0;
        b.wfirst[c - c0] = xt[(size_t)e0].alpha;
        b.wmid[c - c0] = xt[(size_t)e0 + 1].alpha;
        for (int k = 1; k <= b.amin - 2 && ok; ++k) ok = xt[(size_t)(e0 + k)].alpha == b.wmid[c - c0];
        for (int j = 0; j < 4; ++j) b.wtail[c - c0][j] = b.amin - 1 + j < nn ? xt[(size_t)(e0 + b.amin - 1 + j)].alpha : 0.f;
      }
      if (b.amin == b.amax && (b.amin == 16 || b.amin == 32)) {
        b.rotm = b.amin - 1;
        for (int c = 0; c < b.ncell; ++c) b.rot[c] = c * std::max(1, b.amin / b.ncell) & b.rotm;
      }
      {  // plane stride: the fewest lanes per LDS bank over the walk (every lane advances by one column per read)
        int best = 1 << 30;
        for (int cand_tp = 16 * Tc + 8; cand_tp <= 16 * Tc + 8 + 39; ++cand_tp) {
          int cnt[32] = {0};
          for (int im = 0; im < 4; ++im)
            for (int c = 0; c < b.ncell; ++c) cnt[(b.si0[c] + b.rot[c] + im * cand_tp) & 31]++;
          int worst = 0;
          for (int k = 0; k < 32; ++k) worst = std::max(worst, cnt[k]);
          // (ties: prefer strides that also keep the blur's stores -- 16 consecutive columns per image -- apart)
          const int score = worst * 64 + ((cand_tp & 31) == 16 ? 0 : (cand_tp & 15) == 8 ? 1 : 2);
          if (score < best) best = score, b.tp = cand_tp;
        }
      }
      band_of(b.xs, 0, true, b.band[0]);
      band_of(b.xs, 0, false, b.band[1]);
      band_of(b.xs, Tc - 1, false, b.band[2]);
      // every tile between must be the plain band: no image edge within three columns of it
      for (int c = 1; c + 1 < Tc && ok; ++c) {
        unsigned m[64][4];
        memset(m, 0, sizeof m);
        band_of(b.xs, c, false, m);
        ok = memcmp(m, b.band[0], sizeof m) == 0;
      }
      cand.push_back(b);
    }
    if (ok) host.swap(cand);
  }
  if (!host.empty()) {
    for (BaStrip& b : host) d.amax = std::max(d.amax, b.amax);
    d.n_strips = (int)host.size();
    d.T = host[0].T;
  }
  return d;
}

// The B operand of k_dcthash_256_band: lane l = (column n = l & 15 of the tile, chunk q = l >> 4), byte j <-> k = 16 q + j.
// k < 32: source column 16 c - 8 + k of the row, weight 1 on the 7 taps of output column 16 c + n (an interior tile: the
// kernel mirrors the image's edge columns into the ring); k >= 32: the same columns of the row seven above, weights negated.
inline void make_band_tables(BandTables* bt) {
  memset(bt, 0, sizeof(*bt));
  for (int l = 0; l < 64; ++l)
    for (int j = 0; j < 16; ++j) {
      const int k = 16 * (l >> 4) + j, kk = k & 31;
      int wgt = std::abs((kk - 8) - (l & 15)) <= 3 ? 1 : 0;
      if (k >= 32) wgt = -wgt;
      bt->w[0][l][j >> 2] |= (unsigned)(wgt & 0xff) << (8 * (j & 3));
    }
}

// rows per step for a workgroup of T threads making ncell cells per row: a turn of the area phase has 2 T / ncell row
// slots, and 14 rows fill a turn of 12 (T = 192), 24, 32, 48 or 64 slots badly -- 21 where that fills the turns better
inline int pick_rows_per_step(int K, unsigned T, int ncell, size_t lds_per_row, size_t lds_fixed) {
  if (K != 7) return 15;
  auto fits = [&](int ks) { return lds_fixed + (size_t)ks * lds_per_row <= (size_t)64 * 1024; };
  const int cap = (int)(2 * T) / ncell;
  int best = 14;
  double best_u = 0.0;
  for (int ks : {14, 21}) {  // (28 measured too: slower than 21 everywhere, 15-30 % slower than 14 on one-wave workgroups)
    if (!fits(ks)) break;
    const int turns = (ks + cap - 1) / cap;
    const double u = (double)ks / ((double)turns * cap);
    if (u > best_u + 0.05) best = ks, best_u = u;  // (more rows per step only for a real gain: they cost LDS)
  }
  return best;
}
// steps per strip of k_blur_area_regs: every strip re-reads the 6 rows of blur halo and its last step may be partly
// empty, so the rows PROCESSED depend on how h divides: 960 rows in strips of 8 x 14 = 106 output rows are 10 strips =
// 1120 rows, in strips of 9 x 14 = 120 they are 8 = 1008.  Around the target (which the batch size sets: enough
// workgroups), the count that processes the fewest rows; ties go to the longer strip.  hash_stream (the knob's value) >= 2
// forces its value.
inline int pick_steps_per_strip(int h, int ks, int target, int halo, int hash_stream) {
  const int all = (h + halo + ks - 1) / ks;  // one strip spanning the image
  if (hash_stream >= 2 || target >= all) return std::max(1, std::min(target, all));
  int best = target;
  long long best_rows = -1;
  for (int st = std::max(2, target - 1); st <= std::min(all, target + 3); ++st) {
    const int out = st * ks - halo;
    if (out <= 0) continue;
    const long long rows = (long long)((h + out - 1) / out) * st * ks;
    if (best_rows < 0 || rows <= best_rows) best = st, best_rows = rows;
  }
  return best;
}
// integer ratios, cells of nd = isx / 4 dwords: the 32 lanes of a row group read dword u of their cells together, gcd(nd, 32)
// to a bank -- one pad dword behind every cell of a blurred LDS row where that would be 4 ways or more (512, 1024, 1536 px ...)
inline int cell_pad_for(bool integer, int isx) {
  if (!integer || (isx & 7)) return 0;  // (nd even: a blur lane's two dwords stay in one cell)
  int g = 1;
  while (g < 32 && ((isx >> 2) % (2 * g)) == 0) g *= 2;
  return g >= 4 ? 1 : 0;
}

}  // namespace
}  // namespace cbh
