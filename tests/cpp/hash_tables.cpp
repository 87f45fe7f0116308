// The host-only tables and sizing rules of cbird_amd/csrc/dcthash_tables.h, printed for tests/test_hash_tables.py.  Host code
// only: includes nothing else of the library and links nothing.  Floats are printed as their bit patterns (hex).
// In (stdin), one command per line; out, one line per command (strips: one more line per strip):
//   area S            -> n | si di alpha ...                        make_area_tab(S, 32)
//   fast W H          -> 0 / 1                                      area_fast
//   yrow H            -> n (0: none) | a0 a1 info k0 ...            make_yrows, the kYRowPad pads included
//   strips W          -> n_strips T amax RS, then per strip: xs T cell0 ncell amax amin tp rotm | si0[ncell]
//   bands W           -> per strip one line: the 3 x 64 x 4 words of band[]
//   cols W INT NCOL S -> x0 ws n | si di alpha ... | xfirst[33]     make_strip_geom
//   steps H KS TARGET HALO STREAM -> pick_steps_per_strip
//   rows K T NCELL PER_ROW FIXED  -> pick_rows_per_step
//   sweep LO HI       -> builds every table for every size in [LO, HI] (the sanitizer run); prints counts
#include <cstdio>
#include <cstring>

#include "dcthash_tables.h"

using namespace cbh;

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

static void print_tab(const std::vector<AreaTab>& t) {
  for (const AreaTab& e : t) printf(" %d %d %08x", e.si, e.di, bits(e.alpha));
}

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "area")) {
      int s;
      if (scanf("%d", &s) != 1) return 2;
      std::vector<int> first;
      const std::vector<AreaTab> t = make_area_tab(s, 32, &first);
      printf("%zu |", t.size());
      print_tab(t);
      printf("\n");
    } else if (!strcmp(cmd, "fast")) {
      int w, h;
      if (scanf("%d %d", &w, &h) != 2) return 2;
      printf("%d\n", area_fast(w, h) ? 1 : 0);
    } else if (!strcmp(cmd, "yrow")) {
      int h;
      if (scanf("%d", &h) != 1) return 2;
      std::vector<int> yf;
      const std::vector<AreaTab> yt = make_area_tab(h, 32, &yf);
      const std::vector<YRow> yr = make_yrows(h, yt, yf);
      printf("%zu |", yr.size());
      for (const YRow& r : yr) printf(" %08x %08x %d %08x", bits(r.a0), bits(r.a1), r.info, bits(r.k0));
      printf("\n");
    } else if (!strcmp(cmd, "strips") || !strcmp(cmd, "bands")) {
      int w;
      if (scanf("%d", &w) != 1) return 2;
      const BaStripList l = make_ba_strips(w);
      if ((size_t)l.n_strips != l.strips.size()) return 3;
      if (!strcmp(cmd, "strips")) printf("%d %d %d %d\n", l.n_strips, l.T, l.amax, l.RS);
      for (const BaStrip& b : l.strips) {
        if (!strcmp(cmd, "strips")) {
          printf("%d %d %d %d %d %d %d %d |", b.xs, b.T, b.cell0, b.ncell, b.amax, b.amin, b.tp, b.rotm);
          for (int c = 0; c < b.ncell; ++c) printf(" %d", b.si0[c]);
        } else {
          for (int t = 0; t < 3; ++t)
            for (int l64 = 0; l64 < 64; ++l64)
              for (int q = 0; q < 4; ++q) printf(" %08x", b.band[t][l64][q]);
        }
        printf("\n");
      }
    } else if (!strcmp(cmd, "cols")) {
      int w, integer, ncol, s;
      if (scanf("%d %d %d %d", &w, &integer, &ncol, &s) != 4) return 2;
      const StripGeom g = make_strip_geom(w, integer != 0, ncol, s);
      printf("%d %d %zu |", g.x0, g.ws, g.x.size());
      print_tab(g.x);
      printf(" |");
      for (int v : g.xfirst) printf(" %d", v);
      printf("\n");
    } else if (!strcmp(cmd, "steps")) {
      int h, ks, target, halo, stream;
      if (scanf("%d %d %d %d %d", &h, &ks, &target, &halo, &stream) != 5) return 2;
      printf("%d\n", pick_steps_per_strip(h, ks, target, halo, stream));
    } else if (!strcmp(cmd, "rows")) {
      int K, T, ncell;
      unsigned long long per_row, fixed;
      if (scanf("%d %d %d %llu %llu", &K, &T, &ncell, &per_row, &fixed) != 5) return 2;
      printf("%d\n", pick_rows_per_step(K, (unsigned)T, ncell, (size_t)per_row, (size_t)fixed));
    } else if (!strcmp(cmd, "sweep")) {
      int lo, hi;
      if (scanf("%d %d", &lo, &hi) != 2) return 2;
      unsigned long long entries = 0, rows = 0, strips = 0, cols = 0;
      for (int s = lo; s <= hi; ++s) {
        std::vector<int> first;
        const std::vector<AreaTab> t = make_area_tab(s, 32, &first);
        entries += t.size();
        rows += make_yrows(s, t, first).size();
        strips += make_ba_strips(s).strips.size();
        for (int ncol = 2; ncol <= 8; ncol *= 2)
          for (int k = 0; k < ncol; ++k) {
            cols += (unsigned long long)make_strip_geom(s, false, ncol, k).ws;
            if (s % 32 == 0) cols += (unsigned long long)make_strip_geom(s, true, ncol, k).ws;
          }
        cols += (unsigned long long)cell_pad_for(s % 32 == 0, s / 32);
      }
      BandTables bt;
      make_band_tables(&bt);
      printf("%llu %llu %llu %llu %08x\n", entries, rows, strips, cols, bt.w[0][0][0]);
    } else {
      return 2;
    }
  }
  return 0;
}
