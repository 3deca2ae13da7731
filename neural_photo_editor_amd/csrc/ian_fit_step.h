// One Adam step of ian_session_fit on one latent component (include/ian.h; npe_ops.fit_adam_step is the same lines in numpy float32).
// Plain float32, every operation rounded on its own, in exactly this order; division and square root correctly rounded (the library
// is built without any flag that relaxes them).  Contraction is switched off for this function alone, as latent_step does
// (kernels_brush.hip), so that the device kernel, the host and tests/session_fit_main.cpp compile the very same body to the same bits.
// No dependency but <math.h>: the CPU test compiles this header with a plain C++ compiler.
#ifndef IAN_FIT_STEP_H_
#define IAN_FIT_STEP_H_

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IAN_FIT_HD __host__ __device__
#else
#define IAN_FIT_HD
#endif

// c1 = float32(1 / (1 - 0.9^t)), c2 = float32(1 / (1 - 0.999^t)) of step t, computed in double by the caller.  *m and *v are the
// moments, updated in place; -> the new latent component.  g == 0 with zero moments returns z: 0 / 1e-8f == 0.
IAN_FIT_HD inline float ian_fit_adam_step(float z, float g, float* m, float* v, float c1, float c2, float lr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float m0 = 0.9f * *m;
  const float m1 = 0.1f * g;
  const float mn = m0 + m1;
  const float v0 = 0.999f * *v;
  float v1 = 0.001f * g;
  v1 = v1 * g;
  const float vn = v0 + v1;
  *m = mn;
  *v = vn;
  const float mh = mn * c1;
  const float vh = vn * c2;
  const float num = lr * mh;
  const float den = sqrtf(vh) + 1e-8f;
  const float step = num / den;
  return z - step;
}

#endif  // IAN_FIT_STEP_H_
