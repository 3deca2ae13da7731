// Stand-alone driver of tip_shape_slot (csrc/ian_tip_check.h) for tests/test_sessions_soft_brush_host.py, built under AddressSanitizer
// and UBSan: the weights are a heap block of exactly th * tw floats and the slot one of exactly 64 * 64 doubles, so a read or a write
// past either ends the program.  Every size 1..64 x 1..64 on a coarse grid and the extremes: the slot holds the float64 quotient
// wn / max wn at row stride 64, 1.0 at the maximum, zeros in the rest of the slot, and all zeros for an all-zero tip.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ian_tip_check.h"

static int check(int tw, int th, unsigned seed, bool zero) {
  using namespace ian;
  float* w = new float[(size_t)tw * th];
  double* slot = new double[(size_t)TIP_SLOT];
  for (int i = 0; i < TIP_SLOT; ++i) slot[i] = -1.0;   // every element must be written
  unsigned s = seed;
  float mx = 0.0f;
  for (int i = 0; i < tw * th; ++i) {
    s = s * 1664525u + 1013904223u;
    w[i] = zero ? 0.0f : (float)(s >> 8) / (float)(1u << 24) * 0.01f;
    mx = w[i] > mx ? w[i] : mx;
  }
  tip_shape_slot(w, tw, th, slot);
  int bad = 0, ones = 0;
  for (int r = 0; r < TIP_MAX_SIDE; ++r)
    for (int c = 0; c < TIP_MAX_SIDE; ++c) {
      const double got = slot[r * TIP_MAX_SIDE + c];
      const bool inside = r < th && c < tw;
      const double want = (inside && mx > 0.0f) ? (double)w[r * tw + c] / (double)mx : 0.0;
      if (got != want || got < 0.0 || got > 1.0) ++bad;
      if (got == 1.0) ++ones;
    }
  if (!zero && mx > 0.0f && ones < 1) ++bad;
  if ((zero || !(mx > 0.0f)) && ones != 0) ++bad;
  delete[] w;
  delete[] slot;
  if (bad) printf("tip_shape_slot %d x %d seed %u zero %d: %d wrong\n", tw, th, seed, (int)zero, bad);
  return bad;
}

int main() {
  int bad = 0;
  const int sides[] = {1, 2, 3, 5, 9, 21, 63, 64};
  for (int tw : sides)
    for (int th : sides) {
      bad += check(tw, th, 17u * tw + th, false);
      bad += check(tw, th, 1u, true);
    }
  if (bad) return 1;
  printf("soft brush checks passed\n");
  return 0;
}
