// The Adam step of ian_session_fit (csrc/ian_fit_step.h) on the CPU, for tests/test_sessions_fit_host.py: the very body the device
// kernel compiles.  stdin: one case per line, "z g m v lr t" -- the five floats as the hexadecimal bit patterns of their float32
// values, t decimal.  stdout: per case "z_new m_new v_new" as bit patterns.  The bias corrections are formed from t exactly as the
// library's host code forms them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ian_fit_step.h"

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}
static uint32_t to_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  unsigned z, g, m, v, lr;
  int t;
  while (scanf("%x %x %x %x %x %d", &z, &g, &m, &v, &lr, &t) == 6) {
    if (t < 1 || t > 512) return 2;
    const float c1 = (float)(1.0 / (1.0 - std::pow(0.9, (double)t)));
    const float c2 = (float)(1.0 / (1.0 - std::pow(0.999, (double)t)));
    float mf = from_bits(m), vf = from_bits(v);
    const float zn = ian_fit_adam_step(from_bits(z), from_bits(g), &mf, &vf, c1, c2, from_bits(lr));
    printf("%08x %08x %08x\n", (unsigned)to_bits(zn), (unsigned)to_bits(mf), (unsigned)to_bits(vf));
  }
  return 0;
}
