// Stand-alone driver of csrc/ian_tip_check.h for tests/test_sessions_tip_host.py, built under AddressSanitizer and UBSan: the buffers
// are heap blocks of exactly the size the checks may read, so a read past a tip's th * tw weights or past the (tw, th) table ends the
// program.  One operation per run:
//   size tw th                          -> the refusal code of tip_check_size
//   weights tw th what at               -> code and index of tip_check_weights on th * tw ones with element `at` replaced by `what`
//                                          (neg, nan, inf, ninf, zero, none)
//   event tip c1 r1 c2 r2 tw0 th0 ...   -> the refusal code of tip_check_event against the tips (tw0, th0), ... (0 0: never set)
//   slot tw th                          -> "ok" when tip_to_slot / tip_from_slot give the weights back and zero the rest of the slot
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ian_tip_check.h"

int main(int argc, char** argv) {
  using namespace ian;
  if (argc < 2) return 2;
  const char* op = argv[1];
  auto arg = [&](int i) { return atoi(argv[i]); };
  if (!strcmp(op, "size") && argc == 4) {
    printf("%d\n", (int)tip_check_size(arg(2), arg(3)));
    return 0;
  }
  if (!strcmp(op, "weights") && argc == 6) {
    const int tw = arg(2), th = arg(3), at = arg(5);
    if (tip_check_size(tw, th) != TIP_OK) return 2;
    float* w = new float[(size_t)tw * th];
    for (int i = 0; i < tw * th; ++i) w[i] = 1.0f;
    const char* what = argv[4];
    if (strcmp(what, "none")) {
      if (at < 0 || at >= tw * th) return 2;
      w[at] = !strcmp(what, "neg") ? -1e-30f
            : !strcmp(what, "nan") ? std::numeric_limits<float>::quiet_NaN()
            : !strcmp(what, "inf") ? std::numeric_limits<float>::infinity()
            : !strcmp(what, "ninf") ? -std::numeric_limits<float>::infinity() : 0.0f;
    }
    int where = -1;
    const TipRefusal r = tip_check_weights(w, tw, th, &where);
    printf("%d %d\n", (int)r, where);
    delete[] w;
    return 0;
  }
  if (!strcmp(op, "event") && argc >= 7 && (argc - 7) % 2 == 0) {
    const int count = (argc - 7) / 2;
    int32_t* wh = new int32_t[(size_t)2 * count + (count ? 0 : 1)];
    for (int i = 0; i < 2 * count; ++i) wh[i] = arg(7 + i);
    printf("%d\n", (int)tip_check_event(arg(2), count, wh, arg(3), arg(4), arg(5), arg(6)));
    delete[] wh;
    return 0;
  }
  if (!strcmp(op, "slot") && argc == 4) {
    const int tw = arg(2), th = arg(3);
    if (tip_check_size(tw, th) != TIP_OK) return 2;
    std::vector<float> w((size_t)tw * th), back((size_t)tw * th, -1.0f);
    for (int i = 0; i < tw * th; ++i) w[i] = 1.0f + (float)i;
    float* slot = new float[TIP_SLOT];
    tip_to_slot(w.data(), tw, th, slot);
    tip_from_slot(slot, tw, th, back.data());
    bool ok = w == back;
    for (int r = 0; r < TIP_MAX_SIDE; ++r)
      for (int c = 0; c < TIP_MAX_SIDE; ++c)
        if ((r >= th || c >= tw) && slot[r * TIP_MAX_SIDE + c] != 0.0f) ok = false;
    delete[] slot;
    printf("%s\n", ok ? "ok" : "bad");
    return 0;
  }
  return 2;
}
