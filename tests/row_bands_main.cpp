// Stand-alone CPU driver of csrc/ian_row_bands.h (tests/test_row_bands_host.py builds it under AddressSanitizer + UBSan).
//   row_bands_main bands <gran> <min_rows> <H> <wgs> <n> [<n> ...]   prints row_bands(n, wgs, H, gran, min_rows) for every n
//   row_bands_main sweep    every (n, wgs, H, gran, min_rows) of a grid: the result is the loop each call site used to carry, it is
//                           1, 2, 4 or 8, it divides H (whole row pairs when gran = 2), and no doubling was taken without need;
//                           prints "ok <cases> <cases with 1 band> <2> <4> <8>"
//   row_bands_main walk     walks the rows of every band the way deconv_small_kernel and head6_kernel (kernels_head.hip) do, for 1, 2, 4
//                           and 8 bands: every owned output row gets each of its input rows exactly once and leaves exactly once, and
//                           no two open rows share a ring slot.  Prints per kernel and band count the row span of an inner and of an
//                           edge band and how many bands take the even / --r_begin / ++r_end path
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ian_row_bands.h"

using namespace ian;

#define CHECK(cond, ...)                                               \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                                    \
      fprintf(stderr, "\n");                                           \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

// the three loops as they stood at their call sites before the rule had a function of its own
static int old_head(int n, int wgs, int H, int halo) {
  int bands = 1;
  while (n * bands < wgs && bands < 8 && (H % (bands * 2)) == 0 && H / (bands * 2) >= 2 * halo) bands *= 2;
  return bands;
}
static int old_dec_out(int n, int wgs, int in_h) {
  int bands = 1;
  while (n * bands < wgs && bands < 8 && (in_h % (4 * bands)) == 0) bands *= 2;
  return bands;
}

static int run_sweep() {
  long long cases = 0, hist[9] = {0};
  for (int H : {4, 8, 16, 24, 32, 36, 48, 64, 96, 128})
    for (int wgs : {1, 2, 3, 6, 8, 12, 16, 32, 100, 256, 1024})
      for (int n = 1; n <= 300; ++n) {
        for (int halo = 0; halo <= 4; ++halo) {
          const int b = row_bands(n, wgs, H, 1, 2 * halo);
          CHECK(b == old_head(n, wgs, H, halo), "head: n %d wgs %d H %d halo %d: %d", n, wgs, H, halo, b);
          CHECK((b == 1 || b == 2 || b == 4 || b == 8) && H % b == 0, "head: %d bands of %d rows", b, H);
          CHECK(b == 1 || H / b >= 2 * halo, "head: a band of %d rows with a halo of %d", H / b, halo);
          CHECK(b == 1 || n * (b / 2) < wgs, "head: %d bands although %d x %d workgroups reach %d", b, n, b / 2, wgs);
          ++cases; ++hist[b];
        }
        const int b = row_bands(n, wgs, H, 2, 0);
        CHECK(b == old_dec_out(n, wgs, H), "dec_out: n %d wgs %d H %d: %d", n, wgs, H, b);
        CHECK((b == 1 || b == 2 || b == 4 || b == 8) && H % b == 0 && H % (2 * b) == 0, "dec_out: %d bands of %d rows are not whole row pairs", b, H);
        CHECK(b == 1 || n * (b / 2) < wgs, "dec_out: %d bands although %d x %d workgroups reach %d", b, n, b / 2, wgs);
        ++cases; ++hist[b];
      }
  printf("ok %lld %lld %lld %lld %lld\n", cases, hist[1], hist[2], hist[4], hist[8]);
  return 0;
}

struct WalkStats { int inner_span = -1, edge_span = -1, even = 0, dec_begin = 0, inc_end = 0; };

// deconv_small_kernel: input rows H, output rows 2H; output row oy collects input rows (oy - 2) / 2 .. (oy + 2) / 2 (ky = oy + 2 - 2 q in 0..4)
static WalkStats walk_dec_out(int H, int bands) {
  const int RING = 8;
  WalkStats st;
  std::vector<int> written(2 * H, 0);
  for (int band = 0; band < bands; ++band) {
    const int rows_per_band = H / bands, q0 = band * rows_per_band, q1 = q0 + rows_per_band, oy_lo = 2 * q0, oy_hi = 2 * q1;
    int r_begin = std::max(0, q0 - 1), r_end = std::min(H, q1 + 1);
    const int span = r_end - r_begin;
    const bool edge = bands > 1 && (band == 0 || band == bands - 1);
    int& slot = edge ? st.edge_span : st.inner_span;
    CHECK(slot < 0 || slot == span, "bands of one kind with spans %d and %d", slot, span);
    slot = span;
    if (span & 1) {
      if (r_begin > 0) { --r_begin; ++st.dec_begin; }
      else { ++r_end; ++st.inc_end; }
    } else ++st.even;
    CHECK(r_begin >= 0 && r_end <= H && ((r_end - r_begin) & 1) == 0, "band %d of %d walks rows [%d, %d) of %d", band, bands, r_begin, r_end, H);
    std::vector<int> ring_row(RING, -1);                  // which output row a ring slot holds
    std::vector<std::vector<int>> got(2 * H);             // input rows added to an output row, in order
    for (int r = r_begin; r < r_end; r += 2) {
      for (int d = 0; d < 7; ++d) {
        const int oy = 2 * r - 2 + d;
        if (oy < oy_lo || oy >= oy_hi) continue;
        int& held = ring_row[oy & (RING - 1)];
        CHECK(held == -1 || held == oy, "ring slot of row %d still holds row %d", oy, held);
        held = oy;
        for (int ql = 0; ql < 2; ++ql) {                  // s7[2 ql + ky]
          const int ky = d - 2 * ql;
          if (ky >= 0 && ky < 5) got[oy].push_back(r + ql);
        }
      }
      const int f_lo = std::max(oy_lo, 2 * r - 2), f_hi = std::min(oy_hi - 1, (r + 2 >= H) ? 2 * r + 3 : 2 * r + 1);
      for (int oy = f_lo; oy <= f_hi; ++oy) {
        std::vector<int> want;
        for (int q = 0; q < H; ++q)
          if (oy + 2 - 2 * q >= 0 && oy + 2 - 2 * q < 5) want.push_back(q);
        CHECK(got[oy] == want, "output row %d (band %d of %d) leaves with %zu of its %zu input rows", oy, band, bands, got[oy].size(), want.size());
        ++written[oy];
        ring_row[oy & (RING - 1)] = -1;
      }
    }
  }
  for (int oy = 0; oy < 2 * H; ++oy) CHECK(written[oy] == 1, "output row %d written %d times with %d bands", oy, written[oy], bands);
  return st;
}

// head6_kernel: H rows in, H rows out; output row y collects the input rows y - halo .. y + halo
static WalkStats walk_head(int H, int bands, int halo) {
  const int RING = 16;
  WalkStats st;
  std::vector<int> written(H, 0);
  for (int band = 0; band < bands; ++band) {
    const int rows_per_band = H / bands, y0 = band * rows_per_band, y1 = y0 + rows_per_band;
    const int r_begin = std::max(0, y0 - halo), r_end = std::min(H, y1 + halo);
    const bool edge = bands > 1 && (band == 0 || band == bands - 1);
    int& slot = edge ? st.edge_span : st.inner_span;
    CHECK(slot < 0 || slot == r_end - r_begin, "bands of one kind with spans %d and %d", slot, r_end - r_begin);
    slot = r_end - r_begin;
    ++st.even;
    std::vector<int> ring_row(RING, -1);
    std::vector<std::vector<int>> got(H);
    for (int r = r_begin; r < r_end; ++r) {
      for (int g = 0; g < 9; ++g) {
        const int dy = (g == 0) ? 0 : (g <= 4 ? g - 5 : g - 4);
        if (std::abs(dy) > halo) continue;                // no tap with this dy: the kernel adds a zero
        const int y = r - dy;
        if (y < y0 || y >= y1) continue;
        int& held = ring_row[y & (RING - 1)];
        CHECK(held == -1 || held == y, "ring slot of row %d still holds row %d", y, held);
        held = y;
        got[y].push_back(r);
      }
      const int lo = std::max(y0, r - halo), hi = std::min(y1 - 1, (r == H - 1) ? y1 - 1 : r - halo);
      for (int yf = lo; yf <= hi; ++yf) {
        std::vector<int> have = got[yf], want;
        std::sort(have.begin(), have.end());
        for (int q = std::max(0, yf - halo); q <= std::min(H - 1, yf + halo); ++q) want.push_back(q);
        CHECK(have == want, "output row %d (band %d of %d) leaves with %zu of its %zu input rows", yf, band, bands, have.size(), want.size());
        ++written[yf];
        ring_row[yf & (RING - 1)] = -1;
      }
    }
  }
  for (int y = 0; y < H; ++y) CHECK(written[y] == 1, "output row %d written %d times with %d bands", y, written[y], bands);
  return st;
}

static int run_walk() {
  for (int bands : {1, 2, 4, 8}) {
    const WalkStats s = walk_dec_out(32, bands);
    printf("dec_out 32 %d %d %d %d %d %d\n", bands, s.inner_span, s.edge_span, s.even, s.dec_begin, s.inc_end);
  }
  for (int H : {64, 32})
    for (int bands : {1, 2, 4, 8}) {
      if (H / bands < 2 * 4) continue;                    // row_bands never goes there with a halo of 4
      const WalkStats s = walk_head(H, bands, 4);
      printf("head %d %d %d %d %d %d %d\n", H, bands, s.inner_span, s.edge_span, s.even, s.dec_begin, s.inc_end);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
  if (argc == 2 && !strcmp(argv[1], "walk")) return run_walk();
  if (argc >= 7 && !strcmp(argv[1], "bands")) {
    const int gran = atoi(argv[2]), min_rows = atoi(argv[3]), H = atoi(argv[4]), wgs = atoi(argv[5]);
    for (int i = 6; i < argc; ++i) printf("%d%c", row_bands(atoi(argv[i]), wgs, H, gran, min_rows), i + 1 < argc ? ' ' : '\n');
    return 0;
  }
  return 2;
}
