// npe_blend.h -- device code of NPE.paint's photo blend shared by kernels_npe.hip (ian_photo_blend, ian_brush_step_batch) and
// kernels_session.hip (ian_session_brush / ian_session_set_latent): the byte casts and photo_blend_image.  kernels_window.hip
// includes it for the pragma alone.
// Everything BELOW the include of this header is compiled with floating-point contraction off (see the pragma).
#pragma once
#include "ian_internal.h"

// numpy and scipy round every operation, while hipcc's default -ffp-contract=fast fuses a*b+c into ONE rounding
// (measured on MI355X: 1-ulp differences from scipy in 31 % of the mask values).  HIP's __dadd_rn / __dmul_rn / __fadd_rn
// do not help: on AMD targets they are inline plain operators defined under the default mode, and fuse after inlining.
// So: plain operators, with contraction switched off for everything below this line (checked in the ISA: separate
// v_mul_f64 / v_add_f64; the only fmas left are inside the correctly rounded division expansions).
#pragma clang fp contract(off)

namespace ian {

__device__ __forceinline__ unsigned char np_uint8(double v) {  // numpy float64 -> uint8 on x86-64: cvttsd2si, low byte
  const int i = (int)v;   // truncation toward zero; |v| stays far below 2^31 here
  return (unsigned char)(i & 0xFF);
}
__device__ __forceinline__ unsigned char np_uint8f(float v) {
  const int i = (int)v;
  return (unsigned char)(i & 0xFF);
}
__device__ __forceinline__ int reflect_idx(int i, int n) {  // d c b a | a b c d | d c b a
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - 1 - i;
  return i;
}

constexpr int PB_T = 1024;
// one 64x64 image per workgroup of PB_T threads; m0 / m1 are the workgroup's two 64x64 float64 LDS planes.
// LOCAL (session_blend_local_kernel only; npe_ops.photo_blend_local): in the last pass the thread that owns a pixel reads its UMASK
// value once, max-es it with the brush footprint (two loads from the 64-entry falloff table, one product: npe_ops.local_footprint),
// writes it back once and multiplies MASK by it; dampen replaces D where to_tanh(float32(RECON)) + D passes the threshold.  Every
// branch on l is uniform over the workgroup.  The instantiation without LOCAL is the code it always was.
template <bool LOCAL = false>
__device__ __forceinline__ void photo_blend_image(const PhotoBlendArgs& a, double* m0, double* m1, const PhotoLocalArgs* l = nullptr) {
  constexpr int H = 64, W = 64, HW = H * W;
  const int tid = threadIdx.x;
  // ---- min(mean_c |DELTA|, 1): float32 until np.min promotes to float64
  for (int p = tid; p < HW; p += PB_T) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r = (float)a.recon[c * HW + p];
      const float tt = (2.0f * (r / 255.0f)) - 1.0f;      // to_tanh(np.float32(RECON))
      const float d = fabsf(a.xhat[c * HW + p] - tt);
      s = (c == 0) ? d : s + d;                                           // add.reduce over axis 0
    }
    const float mean = s / 3.0f;
    const double v = (double)mean;
    m0[p] = v < 1.0 ? v : 1.0;
  }
  __syncthreads();
  // ---- separable Gaussian, axis 0 (rows) then axis 1 (columns)
  const int R = a.radius;
  for (int p = tid; p < HW; p += PB_T) {
    const int y = p / W, x = p % W;
    double t = m0[p] * a.w[0];
    for (int j = R; j >= 1; --j)
      t = t + (m0[reflect_idx(y - j, H) * W + x] + m0[reflect_idx(y + j, H) * W + x]) * a.w[j];
    m1[p] = t;
  }
  __syncthreads();
  for (int p = tid; p < HW; p += PB_T) {
    const int y = p / W, x = p % W;
    double t = m1[p] * a.w[0];
    for (int j = R; j >= 1; --j)
      t = t + (m1[y * W + reflect_idx(x - j, W)] + m1[y * W + reflect_idx(x + j, W)]) * a.w[j];
    m0[p] = t;   // every thread rewrites only the pixels it read in the FIRST pass and nobody reads m0 in this pass
  }
  __syncthreads();
  // ---- IM = uint8(from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR)), float64
  for (int p = tid; p < HW; p += PB_T) {
    double mask = m0[p];
    if (a.mask) a.mask[p] = mask;
    if constexpr (LOCAL) {
      if (l->umask) {
        double u = l->umask[p];
        if (l->falloff && l->c2 > l->c1 && l->r2 > l->r1) {   // umask_paint: np.maximum(U, t[dy] * t[dx]); the table has no NaN
          const int y = p / W, x = p % W;
          const int dx = x < l->c1 ? l->c1 - x : (x >= l->c2 ? x - l->c2 + 1 : 0);   // 0..63 for 0 <= c1 < c2 <= 64 (the launcher checks)
          const int dy = y < l->r1 ? l->r1 - y : (y >= l->r2 ? y - l->r2 + 1 : 0);
          const double f = l->falloff[dy] * l->falloff[dx];
          u = u < f ? f : u;
          l->umask[p] = u;
        }
        mask = mask * u;   // MASK_L
      }
    }
    const double om = 1.0 - mask;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned char rb = a.recon[c * HW + p];
      const float r = (float)rb;
      const float tt = (2.0f * (r / 255.0f)) - 1.0f;
      const float delta = a.xhat[c * HW + p] - tt;
      double D = mask * (double)delta + om * (double)a.error[c * HW + p];
      bool damp = false;
      if constexpr (LOCAL) {
        if (l->dampen) {   // NPE.py:184-189 as np.where(float64(t32) + D > thresh, thresh - float64(t32), D)
          damp = true;
          const double s = (double)tt + D;
          if (s > l->thresh) D = l->thresh - (double)tt;
        }
      }
      const double t64 = 2.0 * ((double)rb / 255.0) - 1.0;   // to_tanh(RECON): uint8 -> float64
      const double v = 255.0 * ((t64 + D) + 1.0) / 2.0;
      a.im[c * HW + p] = np_uint8(v);
      if (a.field)   // npe_ops.edit_field; dampened: float32(D - float64(ERROR))
        a.field[c * HW + p] = damp ? (float)(D - (double)a.error[c * HW + p]) : (float)(mask * ((double)delta - (double)a.error[c * HW + p]));
    }
  }
}

}  // namespace ian
