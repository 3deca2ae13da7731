// The 64x64 steps right after the decoder in every NPE edit, on the device:
//   photo_blend_kernel  NPE.paint's photo-mode blend, NPE.py:218-231
//       DELTA = X_hat - to_tanh(float32(RECON));  MASK = gaussian_filter(min(mean_c|DELTA|, 1), 0.7)
//       IM    = uint8(from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR))
//   to_uint8_kernel     uint8(from_tanh(X_hat)), NPE.py:110,261 (update_photo / RECON)
// so that an edit needs ONE 12 KB device->host copy instead of a 48 KB float image plus host numpy/scipy passes.
//
// Byte work is held to bit-exactness against the reference expression (oracle: npe_ops.photo_blend_host): every operation
// is performed in the precision numpy uses for it (float32 for DELTA and its channel mean, float64 from the np.min(...)
// on), in numpy's order, with explicitly rounded intrinsics so that hipcc cannot contract a*b+c into an fma, and the
// Gaussian follows scipy.ndimage's separable 'reflect' correlate1d summation order for a symmetric kernel
// (t = x[l]*w0; t += (x[l-j] + x[l+j])*w[j] for j = R..1; axis 0 first), with the weights computed by the host exactly
// as scipy computes them.  The bare np.uint8 cast (no clipping, NPE.py:231) is truncation toward zero modulo 256.
#include "ian_internal.h"
#include "npe_blend.h"   // contraction off from here on; np_uint8, reflect_idx, photo_blend_image

namespace ian {

__global__ __launch_bounds__(PB_T) void photo_blend_kernel(PhotoBlendArgs a) {
  __shared__ double m0[64 * 64];
  __shared__ double m1[64 * 64];
  photo_blend_image(a, m0, m1);
}
hipError_t launch_photo_blend(const PhotoBlendArgs& a, hipStream_t s) {
  if (a.radius < 0 || a.radius > 7) return hipErrorInvalidValue;
  hipLaunchKernelGGL(photo_blend_kernel, dim3(1), dim3(PB_T), 0, s, a);
  return hipGetLastError();
}
// several editors (ian_brush_step_batch): blockIdx.y = item, every image / mask at that item's offset, the same arithmetic per element
__global__ __launch_bounds__(PB_T) void photo_blend_batch_kernel(PhotoBlendArgs a) {
  __shared__ double m0[64 * 64];
  __shared__ double m1[64 * 64];
  constexpr size_t IMG = 3 * 64 * 64, PLANE = 64 * 64;
  const size_t i = blockIdx.y;
  PhotoBlendArgs b = a;
  b.xhat = a.xhat + i * IMG;
  b.recon = a.recon + i * IMG;
  b.error = a.error + i * IMG;
  b.im = a.im + i * IMG;
  b.mask = a.mask ? a.mask + i * PLANE : nullptr;
  photo_blend_image(b, m0, m1);
}
hipError_t launch_photo_blend_batch(const PhotoBlendArgs& a, int n, hipStream_t s) {
  if (a.radius < 0 || a.radius > 7 || n < 1 || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(photo_blend_batch_kernel, dim3(1, n), dim3(PB_T), 0, s, a);
  return hipGetLastError();
}

// uint8(from_tanh(x)) on float32: 255.0*(x+1)/2.0 (NPE.py:40-41), truncation modulo 256
__global__ __launch_bounds__(256) void to_uint8_kernel(const float* __restrict__ x, unsigned char* __restrict__ y, long long n) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    uchar4 o;
    o.x = np_uint8f(255.0f * (v.x + 1.0f) / 2.0f);
    o.y = np_uint8f(255.0f * (v.y + 1.0f) / 2.0f);
    o.z = np_uint8f(255.0f * (v.z + 1.0f) / 2.0f);
    o.w = np_uint8f(255.0f * (v.w + 1.0f) / 2.0f);
    *reinterpret_cast<uchar4*>(y + i) = o;
  } else {
    for (long long k = i; k < n; ++k) y[k] = np_uint8f(255.0f * (x[k] + 1.0f) / 2.0f);
  }
}
hipError_t launch_to_uint8(const float* x, unsigned char* y, long long n, hipStream_t s) {
  hipLaunchKernelGGL(to_uint8_kernel, dim3((unsigned)((n / 4 + 255) / 256 + 1)), dim3(256), 0, s, x, y, n);
  return hipGetLastError();
}


// ---- keep-warm (option edit_keep_warm_us, an EXPERIMENT, off by default) ---------------------------------------------------------
// One wave that keeps the interactive stream's queue busy between two brush events: it polls a flag in the mapped pinned block
// (the next event sets it just before its graph is launched) and gives up after max_ticks of the 100 MHz wall clock (s_memrealtime).  What it is for:
// the first kernel of every graph replay costs ~20 us whatever it does (profiles/r05_batch1_chains.md) -- is that the wake-up of
// an idle queue?  The bench line's edit_step.keep_warm compares the event latency with and without it.
__global__ __launch_bounds__(64) void keep_warm_kernel(const volatile int* flag, long long max_ticks) {
  if (threadIdx.x != 0) return;
  const long long t0 = (long long)wall_clock64();
  while (*flag == 0 && (long long)wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(8);
}
hipError_t launch_keep_warm(const int* flag, long long max_ticks, hipStream_t s) {
  hipLaunchKernelGGL(keep_warm_kernel, dim3(1), dim3(64), 0, s, flag, max_ticks);
  return hipGetLastError();
}

}  // namespace ian
