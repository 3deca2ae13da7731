// The latent brush's backward kernels (ian_grad_*, ian_brush_step, their batched forms, ian_session_brush): the loss seeds of
// API.py:59,64, the backward-data of the image-producing transposed conv, the latent's backward GEMV and the brush update
// Z += coef * (dZ * gscale) of NPE.py:205-209.  Latency work at batch 1, bandwidth work for several editors; never MFMA.
// Everything here is compiled under the default floating-point contraction mode (1 - y*y of m_dact is one fma); only
// latent_step switches it off, for itself.
#include <algorithm>

#include "ian_internal.h"
#include "ian_dact.h"   // m_dact

namespace ian {

// ---- loss seeds ------------------------------------------------------------------------------------------------------------------
// d loss / d x_hat for the two brush losses over the rectangle rows r1..r2, columns c1..c2 of an image x_hat [3,H,W]:
//  mode 0 (API.py:59): loss = mean(x_hat[:, r1:r2, c1:c2])                  -> g = 1/N           N = 3*(r2-r1)*(c2-c1)
//  mode 1 (API.py:64): loss = mean((target - x_hat)^2 over the rectangle)   -> g = 2*(x_hat-target)/N
// and zero outside the rectangle (everywhere, when the rectangle is empty).  Where the rectangle, the loss kind and the target of
// item blockIdx.y come from is BrushSeedSrc (ian_internal.h); a kernel is compiled per kind of source:
enum { SEED_IMM = 0,      // the rectangle and loss kind are launch arguments, the target an image (the eager single call)
       SEED_RGB = 1,      // row blockIdx.y of the ian_brush_item table, the target an image rgb [n,3,H,W]
       SEED_COLOUR = 2,   // the same table, the target a constant colour [n][3] (ian_session_brush, NPE.py:205 myRGB)
       SEED_PHOTO = 3,    // the same table, the target the item's own photo: tab[GIM byte] of session ids[item] (ian_session_fit)
       SEED_CLONE = 4,    // the same table, the target another picture of the pool, shifted: tab[F byte at o + shift] of session
                          // clone[3 item], F = its GIM, IM or RECON row (ian_session_clone)
       SEED_TIP = 5,      // SEED_COLOUR with a weight per pixel in the place of the flat 1/N: tips[tipsel[item]][r - r1][c - c1], a
                          // brush tip of ian_sessions_set_tip (ian_session_brush_tip); an item with tipsel -1 keeps 1/N
       SEED_CLONE_TIP = 6 };   // SEED_CLONE with SEED_TIP's weight (ian_session_stamp_soft): the target from the pool, the factor from the tip
constexpr bool seed_clones(int kind) { return kind == SEED_CLONE || kind == SEED_CLONE_TIP; }   // the target is SEED_CLONE's
constexpr bool seed_tipped(int kind) { return kind == SEED_TIP || kind == SEED_CLONE_TIP; }     // the factor is SEED_TIP's
struct SeedRect { int c1, r1, c2, r2, mode, id, field, shift, tip; };   // id: SEED_PHOTO the item's session, the clones its source;
                                                                        // field, shift: the clones only; tip: the tipped kinds only
constexpr int SEED_PHOTO_IMG = 3 * 64 * 64;          // a GIM / IM / RECON row of the session pool
constexpr int SEED_TIP_ROW = 64, SEED_TIP_IMG = 64 * 64;   // a tip's row stride and its slot in BrushSeedSrc::tips
template <int KIND> struct SeedLds {                 // ints / floats of LDS a kernel hands to seed_fetch
  static constexpr int SP = KIND == SEED_CLONE_TIP ? 9 : (KIND == SEED_CLONE ? 8 : ((KIND == SEED_PHOTO || KIND == SEED_TIP) ? 6 : 5));
  static constexpr int SC = (KIND == SEED_PHOTO || seed_clones(KIND)) ? 256 : 4;
};

// The table may live in mapped host memory (zero-copy graphs): ONE lane per word fetches it and hands it on through LDS -- a scalar
// load per wave over PCIe made the fused kernel the longest of the brush event (19.0 us, profiles/r05_batch1_chains.md).  Ends in a
// barrier: every thread of the workgroup calls it.  sp: SeedLds::SP ints, sc: SeedLds::SC floats of LDS (sc receives the item's
// colour, or for SEED_PHOTO the 256-entry tanh table).
// SEED_PHOTO stages the 1 KB table in LDS instead of reading it through the cache: with the whole-picture rectangle of a fit every
// thread of the fused kernel looks up all 75 (tap, channel) targets of its pixel, each a byte load followed by a dependent table
// load, and the second hop from LDS is a fraction of an L1 hit; the 32 lanes that share a pixel read the same entry (a broadcast,
// no bank conflict).  Staging costs one load per thread under the barrier the rectangle needs anyway (the workgroups are 256
// threads, one per entry), as session_open_in_kernel stages it.  The unfused kernel looks up once per thread: there staging neither
// wins nor loses, and it keeps the one seed_value body.
// SEED_CLONE is SEED_PHOTO with the row chosen per item: its three words (source id, field selector, shift) travel like SEED_PHOTO's
// id, one lane per word, and the table is staged for the same reason (ian_session_clone takes the whole picture as a rectangle too).
// SEED_TIP is SEED_COLOUR with one more word, the item's tip index, which travels like SEED_PHOTO's id.  The tip's weights are NOT
// staged: a tip is up to 16 KB, a workgroup of the fused kernel covers 8 pixels and reads at most 8 x 25 of its weights, so staging
// would load far more than is used; they are read through the cache where they are needed (seed_weight).
// SEED_CLONE_TIP is both: SEED_CLONE's three words and staged table, and the tip index as a ninth word by a ninth lane.
template <int KIND>
__device__ __forceinline__ SeedRect seed_fetch(const BrushSeedSrc& src, int item, int* sp, float* sc) {
  if (KIND == SEED_IMM) return {src.c1, src.r1, src.c2, src.r2, src.mode, 0, 0, 0, -1};
  if (threadIdx.x < 5) sp[threadIdx.x] = src.table[item * 7 + threadIdx.x];
  if ((KIND == SEED_COLOUR || KIND == SEED_TIP) && threadIdx.x >= 8 && threadIdx.x < 11) sc[threadIdx.x - 8] = src.colour[item * 3 + (threadIdx.x - 8)];
  if (KIND == SEED_PHOTO) {
    if (threadIdx.x == 5) sp[5] = src.ids[item];
    sc[threadIdx.x] = src.tanh_tab[threadIdx.x];
  }
  if (seed_clones(KIND)) {
    if (threadIdx.x >= 5 && threadIdx.x < 8) sp[threadIdx.x] = src.clone[item * 3 + (threadIdx.x - 5)];
    sc[threadIdx.x] = src.tanh_tab[threadIdx.x];
  }
  if (KIND == SEED_TIP && threadIdx.x == 5) sp[5] = src.tipsel[item];
  if (KIND == SEED_CLONE_TIP && threadIdx.x == 8) sp[8] = src.tipsel[item];
  __syncthreads();
  // the same five words in every lane: kept in scalar registers, as the launch arguments of SEED_IMM are
  return {__builtin_amdgcn_readfirstlane(sp[0]), __builtin_amdgcn_readfirstlane(sp[1]), __builtin_amdgcn_readfirstlane(sp[2]),
          __builtin_amdgcn_readfirstlane(sp[3]), __builtin_amdgcn_readfirstlane(sp[4]),
          (KIND == SEED_PHOTO || seed_clones(KIND)) ? __builtin_amdgcn_readfirstlane(sp[5]) : 0,
          seed_clones(KIND) ? __builtin_amdgcn_readfirstlane(sp[6]) : 0, seed_clones(KIND) ? __builtin_amdgcn_readfirstlane(sp[7]) : 0,
          seed_tipped(KIND) ? __builtin_amdgcn_readfirstlane(sp[KIND == SEED_TIP ? 5 : 8]) : -1};
}
// the u8 row a seed's targets are looked up in: SEED_PHOTO the GIM row of the item's session, the clones the row of their source that
// the field selector names (0 GIM, 1 IM, 2 RECON: the same for every lane of the workgroup); the other kinds have none
template <int KIND>
__device__ __forceinline__ const unsigned char* seed_row(const BrushSeedSrc& src, const SeedRect& R) {
  if (KIND == SEED_PHOTO) return src.gim + (size_t)R.id * SEED_PHOTO_IMG;
  if (seed_clones(KIND)) return (R.field == 0 ? src.gim : (R.field == 1 ? src.im : src.recon)) + (size_t)R.id * SEED_PHOTO_IMG;
  return nullptr;
}
// 1/N, or 0 for an empty rectangle
__device__ __forceinline__ float seed_inv(const SeedRect& R) {
  const int cnt = 3 * (R.r2 - R.r1) * (R.c2 - R.c1);
  return cnt > 0 ? 1.f / (float)cnt : 0.f;
}
// The factor of the loss at pixel (r, c) INSIDE the rectangle: the flat inv, or for the tipped kinds the tip's weight there (all three
// channels share it).  The tip index is the same in every lane (a scalar register), so an item without a tip takes the inv path on a
// workgroup-uniform branch.  ian_session_brush_tip / ian_session_stamp_soft refused every item whose rectangle is not exactly its tip's tw x th <= 64 x 64 and
// every tip outside the reservation: (r - r1) * 64 + (c - c1) stays inside the tip's 64 x 64 slot.  A weight of 0 is not skipped: the
// seed 2 * (xh - t) * 0 is +-0 and adds nothing to an accumulator, so skipping would change no bit, and the branch would serve only
// the corners of a round tip.
template <int KIND>
__device__ __forceinline__ float seed_weight(const BrushSeedSrc& src, const SeedRect& R, float inv, int r, int c) {
  if (seed_tipped(KIND) && R.tip >= 0) return src.tips[(size_t)R.tip * SEED_TIP_IMG + (r - R.r1) * SEED_TIP_ROW + (c - R.c1)];
  return inv;
}
// the seed of element o (channel co, value xh) of the item's image, for an element INSIDE a non-empty rectangle; rgb_i = the item's
// target image, sc = its colour in LDS (SEED_PHOTO / SEED_CLONE: the tanh table, gim_i = the row of seed_row): whichever KIND names
// is read, and only in mode 1.  inv: the pixel's seed_weight; SEED_TIP is SEED_COLOUR, SEED_CLONE_TIP is SEED_CLONE from here on
template <int KIND>
__device__ __forceinline__ float seed_value(int mode, float inv, float xh, const float* rgb_i, const float* sc,
                                            const unsigned char* gim_i, int o, int co, int shift) {
  if (seed_clones(KIND)) {
    // o lies inside the item's rectangle, and ian_session_clone refused every rectangle whose copy shifted by (dr, dc) leaves the
    // 64x64 image: o + shift = (co * 64 + r + dr) * 64 + c + dc stays inside channel plane co of the source row
    return (mode == 0) ? inv : 2.f * (xh - sc[gim_i[o + shift]]) * inv;
  }
  return (mode == 0) ? inv : 2.f * (xh - ((KIND == SEED_COLOUR || KIND == SEED_TIP) ? sc[co] : (KIND == SEED_PHOTO ? sc[gim_i[o]] : rgb_i[o]))) * inv;
}

// seed only: g NCHW [n,3,H,W]; element i of an image belongs to channel i / (H*W).  Grid (3*H*W / 256, n).
template <int KIND>
__global__ __launch_bounds__(256) void brush_seed_kernel(BrushSeedSrc src, const float* __restrict__ xhat, float* __restrict__ g, int H,
                                                         int W) {
  __shared__ int sp[SeedLds<KIND>::SP];
  __shared__ float sc[SeedLds<KIND>::SC];
  const int item = blockIdx.y;
  const SeedRect R = seed_fetch<KIND>(src, item, sp, sc);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * H * W) return;
  const size_t img = (size_t)item * 3 * H * W;   // this item's image and target image
  const float* xh_i = xhat + img;
  const float* rgb_i = (KIND != SEED_COLOUR && KIND != SEED_TIP && KIND != SEED_PHOTO && !seed_clones(KIND) && R.mode) ? src.rgb + img : nullptr;
  const unsigned char* gim_i = seed_row<KIND>(src, R);
  const int xx = i % W, yy = (i / W) % H;
  float v = 0.f;
  if (yy >= R.r1 && yy < R.r2 && xx >= R.c1 && xx < R.c2) {
    const float inv = seed_inv(R);
    if (inv > 0.f) v = seed_value<KIND>(R.mode, seed_weight<KIND>(src, R, inv, yy, xx), xh_i[i], rgb_i, sc, gim_i, i, i / (H * W), R.shift);
  }
  (g + img)[i] = v;
}

// The brush's first backward step in ONE launch when the image comes out of a transposed conv (IAN_simple dec_out): the seed, the
// output activation's derivative and the conv's backward-data.
//   gout[co,oy,ox] = seed(co,oy,ox) * out_act'(xhat) * oscale[co]
//   dx[iy,ix,ci]   = ( sum_{ky,kx,co} gout[co,2iy-2+ky,2ix-2+kx] * w[ky*5+kx][co][ci] ) * act'(yfwd[iy,ix,ci]) * scale[ci]
// xhat NCHW [n,Cout,2H,2W]; dx, yfwd NHWC [n,H,W,Cin]; w packed [25][4][Cin].  The seed is non-zero only inside the rectangle, so a
// thread visits only the taps whose output pixel lies in it (a brush event: most threads none; the whole-picture rectangle of
// ian_session_fit: every thread all of its taps, see seed_fetch for what that means for SEED_PHOTO's table).  A thread owns four consecutive channels of a
// pixel (float4 filter loads and stores); grid (H*W*Cin/4 / 256, n).  One event is n = 1 with a one-row table.
template <int KIND>
__global__ __launch_bounds__(256) void brush_seed_dec_out_kernel(BrushSeedSrc src, const float* __restrict__ xhat, int out_act,
                                                                 const float* __restrict__ oscale, const float* __restrict__ w,
                                                                 float* __restrict__ dx, const float* __restrict__ yfwd,
                                                                 const float* __restrict__ scale, int H, int W, int Cin, int Cout, int act) {
  __shared__ int sp[SeedLds<KIND>::SP];
  __shared__ float sc[SeedLds<KIND>::SC];
  const int item = blockIdx.y;
  const SeedRect R = seed_fetch<KIND>(src, item, sp, sc);
  const int c4n = Cin >> 2;
  const int idx4 = blockIdx.x * 256 + threadIdx.x;
  if (idx4 >= H * W * c4n) return;
  const int ci = (idx4 % c4n) * 4, pix = idx4 / c4n;
  const int ix = pix % W, iy = pix / W;
  const int OH = 2 * H, OW = 2 * W;
  const size_t img = (size_t)item * Cout * OH * OW;   // this item's image and target image
  const float* xh_i = xhat + img;
  const float* rgb_i = (KIND != SEED_COLOUR && KIND != SEED_TIP && KIND != SEED_PHOTO && !seed_clones(KIND) && R.mode) ? src.rgb + img : nullptr;
  const unsigned char* gim_i = seed_row<KIND>(src, R);
  const float inv = seed_inv(R);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (inv > 0.f) {
    const int ky0 = max(0, R.r1 - (2 * iy - 2)), ky1 = min(5, R.r2 - (2 * iy - 2));
    const int kx0 = max(0, R.c1 - (2 * ix - 2)), kx1 = min(5, R.c2 - (2 * ix - 2));
    for (int ky = ky0; ky < ky1; ++ky) {
      const int oy = 2 * iy - 2 + ky;
      if ((unsigned)oy >= (unsigned)OH) continue;
      for (int kx = kx0; kx < kx1; ++kx) {
        const int ox = 2 * ix - 2 + kx;
        if ((unsigned)ox >= (unsigned)OW) continue;
        const float wt = seed_weight<KIND>(src, R, inv, oy, ox);   // once per tap: the three channels share it
        for (int co = 0; co < Cout; ++co) {
          const int o = (co * OH + oy) * OW + ox;
          const float xh = xh_i[o];
          float gv = seed_value<KIND>(R.mode, wt, xh, rgb_i, sc, gim_i, o, co, R.shift);
          gv = gv * m_dact(xh, out_act) * (oscale ? oscale[co] : 1.f);
          const float4 wv = *reinterpret_cast<const float4*>(w + ((size_t)(ky * 5 + kx) * 4 + co) * Cin + ci);
          acc[0] = fmaf(gv, wv.x, acc[0]);
          acc[1] = fmaf(gv, wv.y, acc[1]);
          acc[2] = fmaf(gv, wv.z, acc[2]);
          acc[3] = fmaf(gv, wv.w, acc[3]);
        }
      }
    }
  }
  const size_t o4 = ((size_t)item * H * W + pix) * Cin + ci;
  float4 out;
  float* op = &out.x;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float d = yfwd ? m_dact(yfwd[o4 + e], act) : 1.f;
    op[e] = acc[e] * d * (scale ? scale[ci + e] : 1.f);
  }
  *reinterpret_cast<float4*>(dx + o4) = out;
}

static int seed_kind(const BrushSeedSrc& src) {
  return !src.table ? SEED_IMM : (src.clone ? (src.tipsel ? SEED_CLONE_TIP : SEED_CLONE) : (src.gim ? SEED_PHOTO : (src.tipsel ? SEED_TIP : (src.colour ? SEED_COLOUR : SEED_RGB))));
}
// a tip weights a colour brush: the colours, the tips' array, and the 64x64 image a tip's slot is made for
static bool seed_tip_ok(const BrushSeedSrc& src, int C, int H, int W) { return src.colour && src.tips && C == 3 && H <= 64 && W <= 64; }
// a photo target is a GIM row of the pool: 3 x 64 x 64 bytes, with the id list and the table to go with it
static bool seed_photo_ok(const BrushSeedSrc& src, int C, int H, int W) { return src.ids && src.tanh_tab && C * H * W == SEED_PHOTO_IMG; }
// a cloned target is a GIM, IM or RECON row of the pool: all three bases, the table, and the 3 x 64 x 64 image the shift is made for
static bool seed_clone_ok(const BrushSeedSrc& src, int C, int H, int W) {
  return src.gim && src.im && src.recon && src.tanh_tab && C == 3 && H == 64 && W == 64;
}

// a weighted clone: a clone's sources and the tips' array
static bool seed_clone_tip_ok(const BrushSeedSrc& src, int C, int H, int W) { return seed_clone_ok(src, C, H, W) && src.tips; }

hipError_t launch_brush_seed(const BrushSeedSrc& src, int n, const float* xhat, float* g, int H, int W, hipStream_t s) {
  const int kind = seed_kind(src);
  if (n < 1 || n > 65535 || (kind == SEED_IMM && n != 1) || (kind == SEED_PHOTO && !seed_photo_ok(src, 3, H, W))) return hipErrorInvalidValue;
  if (kind == SEED_CLONE && !seed_clone_ok(src, 3, H, W)) return hipErrorInvalidValue;
  if (kind == SEED_TIP && !seed_tip_ok(src, 3, H, W)) return hipErrorInvalidValue;
  if (kind == SEED_CLONE_TIP && !seed_clone_tip_ok(src, 3, H, W)) return hipErrorInvalidValue;
  const dim3 grid((3 * H * W + 255) / 256, n);
  if (kind == SEED_IMM) hipLaunchKernelGGL(brush_seed_kernel<SEED_IMM>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  else if (kind == SEED_RGB) hipLaunchKernelGGL(brush_seed_kernel<SEED_RGB>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  else if (kind == SEED_PHOTO) hipLaunchKernelGGL(brush_seed_kernel<SEED_PHOTO>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  else if (kind == SEED_CLONE) hipLaunchKernelGGL(brush_seed_kernel<SEED_CLONE>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  else if (kind == SEED_TIP) hipLaunchKernelGGL(brush_seed_kernel<SEED_TIP>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  else if (kind == SEED_CLONE_TIP) hipLaunchKernelGGL(brush_seed_kernel<SEED_CLONE_TIP>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  else hipLaunchKernelGGL(brush_seed_kernel<SEED_COLOUR>, grid, dim3(256), 0, s, src, xhat, g, H, W);
  return hipGetLastError();
}
hipError_t launch_brush_seed_dec_out(const BrushSeedSrc& src, int n, const float* xhat, int out_act, const float* oscale, const float* w,
                                     float* dx, const float* yfwd, const float* scale, int H, int W, int Cin, int Cout, int act,
                                     hipStream_t s) {
  const int kind = seed_kind(src);   // a colour has three channels; the fused form always reads a table
  if ((Cin & 3) || n < 1 || n > 65535 || kind == SEED_IMM || (kind == SEED_COLOUR && Cout > 3)) return hipErrorInvalidValue;
  if (kind == SEED_PHOTO && !seed_photo_ok(src, Cout, 2 * H, 2 * W)) return hipErrorInvalidValue;
  if (kind == SEED_CLONE && !seed_clone_ok(src, Cout, 2 * H, 2 * W)) return hipErrorInvalidValue;
  if (kind == SEED_TIP && !seed_tip_ok(src, Cout, 2 * H, 2 * W)) return hipErrorInvalidValue;
  if (kind == SEED_CLONE_TIP && !seed_clone_tip_ok(src, Cout, 2 * H, 2 * W)) return hipErrorInvalidValue;
  const dim3 grid((H * W * (Cin >> 2) + 255) / 256, n);
  if (kind == SEED_CLONE_TIP)
    hipLaunchKernelGGL(brush_seed_dec_out_kernel<SEED_CLONE_TIP>, grid, dim3(256), 0, s, src, xhat, out_act, oscale, w, dx, yfwd, scale, H,
                       W, Cin, Cout, act);
  else if (kind == SEED_TIP)
    hipLaunchKernelGGL(brush_seed_dec_out_kernel<SEED_TIP>, grid, dim3(256), 0, s, src, xhat, out_act, oscale, w, dx, yfwd, scale, H, W,
                       Cin, Cout, act);
  else if (kind == SEED_CLONE)
    hipLaunchKernelGGL(brush_seed_dec_out_kernel<SEED_CLONE>, grid, dim3(256), 0, s, src, xhat, out_act, oscale, w, dx, yfwd, scale, H, W,
                       Cin, Cout, act);
  else if (kind == SEED_PHOTO)
    hipLaunchKernelGGL(brush_seed_dec_out_kernel<SEED_PHOTO>, grid, dim3(256), 0, s, src, xhat, out_act, oscale, w, dx, yfwd, scale, H, W,
                       Cin, Cout, act);
  else if (kind == SEED_RGB)
    hipLaunchKernelGGL(brush_seed_dec_out_kernel<SEED_RGB>, grid, dim3(256), 0, s, src, xhat, out_act, oscale, w, dx, yfwd, scale, H, W, Cin,
                       Cout, act);
  else
    hipLaunchKernelGGL(brush_seed_dec_out_kernel<SEED_COLOUR>, grid, dim3(256), 0, s, src, xhat, out_act, oscale, w, dx, yfwd, scale, H, W,
                       Cin, Cout, act);
  return hipGetLastError();
}

// ---- the unfused backward of the image-producing transposed conv (the eager single call) -------------------------------------------
// elementwise: g = g * act'(y) * scale  (NCHW small tensors, c channels of hw pixels)
__global__ __launch_bounds__(256) void dact_nchw_kernel(float* __restrict__ g, const float* __restrict__ y,
                                                        const float* __restrict__ scale, int n, int c, int hw,
                                                        int act) {
  const long long total = (long long)n * c * hw;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)((i / hw) % c);
  g[i] = g[i] * m_dact(y[i], act) * (scale ? scale[ch] : 1.f);
}
hipError_t launch_dact_nchw(float* g, const float* y, const float* scale, int n, int c, int hw, int act,
                            hipStream_t s) {
  const long long total = (long long)n * c * hw;
  hipLaunchKernelGGL(dact_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, y, scale, n, c, hw,
                     act);
  return hipGetLastError();
}

// backward-data of dec_out for the latent brush (API.py:59,64):
//   dacc[n,iy,ix,ci] = ( sum_{ky,kx,co} g[n,co,2iy-2+ky,2ix-2+kx] * w[ky*5+kx][co][ci] ) * act'(yfwd) * scale[ci]
// g is the (patch-sparse) NCHW gradient wrt the pre-activation of dec_out; one thread per (pixel, ci).
__global__ __launch_bounds__(256) void deconv_out_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                             float* __restrict__ dx, const float* __restrict__ yfwd,
                                                             const float* __restrict__ scale, int n, int H, int W,
                                                             int Cin, int Cout, int act) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)n * H * W * Cin;
  if (idx >= total) return;
  const int ci = idx % Cin;
  const size_t pix = idx / Cin;
  const int ix = pix % W, iy = (pix / W) % H, b = pix / ((size_t)W * H);
  const int OH = 2 * H, OW = 2 * W;
  float acc = 0.f;
  for (int ky = 0; ky < 5; ++ky) {
    const int oy = 2 * iy - 2 + ky;
    if ((unsigned)oy >= (unsigned)OH) continue;
    for (int kx = 0; kx < 5; ++kx) {
      const int ox = 2 * ix - 2 + kx;
      if ((unsigned)ox >= (unsigned)OW) continue;
      for (int co = 0; co < Cout; ++co) {
        const float gv = g[((size_t)(b * Cout + co) * OH + oy) * OW + ox];
        acc = fmaf(gv, w[((size_t)(ky * 5 + kx) * 4 + co) * Cin + ci], acc);
      }
    }
  }
  const float d = yfwd ? m_dact(yfwd[idx], act) : 1.f;
  dx[idx] = acc * d * (scale ? scale[ci] : 1.f);
}
hipError_t launch_deconv_out_bwd(const float* g, const float* w, float* dx, const float* yfwd, const float* scale,
                                 int n, int H, int W, int Cin, int Cout, int act, hipStream_t s) {
  const size_t total = (size_t)n * H * W * Cin;
  hipLaunchKernelGGL(deconv_out_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, s, g, w, dx, yfwd, scale, n, H,
                     W, Cin, Cout, act);
  return hipGetLastError();
}

// ---- the latent's backward GEMV and the brush update -------------------------------------------------------------------------------
// Batch-1 backward-data of the dense layer that consumes the latent (l_dec_fc2, IAN_simple.py:112-121; the last step of
// API.py:59,64's T.grad): dz[j] = sum_k g[k] * Wb[j][k].  One workgroup per latent row j streams its 32 KB weight row with
// every load in flight at once -- one launch instead of a split-K tap GEMM, its reduce pass and a row copy.
// upd (ian_brush_step, NPE.py:205-209 / 313-314): the workgroup that owns latent row j also applies the brush update
// Z[j] += coef * (dZ[j] * gscale) -- float32, every product rounded on its own, in the reference's order: bit-identical to the numpy
// expression and to latent_update_kernel below, the separate launch this replaces in the captured brush event.  No
// other workgroup of this launch reads Z[j], and the next kernel of the chain (the decoder's first layer) reads the new row.
struct LatentUpd {
  float* z;          // the latent row, updated in place (nullptr: no update)
  const float* cg;   // (coef, gscale), device-readable
  float* z_mirror;   // or nullptr: the new latent ...
  float* g_mirror;   // ... and the gradient also go there (the pinned host block, zero-copy)
};
__device__ __forceinline__ float latent_step(float z, float g, float coef, float gscale) {
#pragma clang fp contract(off)
  float t = g * gscale;
  t = coef * t;
  return z + t;
}
__global__ __launch_bounds__(256) void dense_bwd_gemv_kernel(const float* __restrict__ g, const float* __restrict__ wb, int K,
                                                             const float* __restrict__ res, float* __restrict__ dz, LatentUpd upd) {
  __shared__ float part[4];
  const int row = blockIdx.x;
  const float* wr = wb + (size_t)row * K;
  // (coef, gscale) may live in mapped host memory: requested first, so that the PCIe round trip runs under the weight stream
  float cg0 = 0.f, cg1 = 0.f, zrow = 0.f;
  if (threadIdx.x == 0 && upd.z) { cg0 = upd.cg[0]; cg1 = upd.cg[1]; zrow = upd.z[row]; }
  float acc = 0.f;
#pragma unroll 8
  for (int k = threadIdx.x * 4; k < K; k += 1024) {
    const float4 a = *reinterpret_cast<const float4*>(g + k);
    const float4 w = *reinterpret_cast<const float4*>(wr + k);
    acc = fmaf(a.x, w.x, acc);
    acc = fmaf(a.y, w.y, acc);
    acc = fmaf(a.z, w.z, acc);
    acc = fmaf(a.w, w.w, acc);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = (part[0] + part[1]) + (part[2] + part[3]);
    if (res) v += res[row];
    dz[row] = v;
    if (upd.z) {
      const float zn = latent_step(zrow, v, cg0, cg1);
      upd.z[row] = zn;
      if (upd.z_mirror) upd.z_mirror[row] = zn;
      if (upd.g_mirror) upd.g_mirror[row] = v;
    }
  }
}
hipError_t launch_dense_bwd_gemv(const float* g, const float* wb, int rows, int K, const float* res, float* dz, float* upd_z,
                                 const float* upd_cg, float* z_mirror, float* g_mirror, hipStream_t s) {
  if (K & 3) return hipErrorInvalidValue;
  const LatentUpd u{upd_z, upd_cg, z_mirror, g_mirror};
  hipLaunchKernelGGL(dense_bwd_gemv_kernel, dim3(rows), dim3(256), 0, s, g, wb, K, res, dz, u);
  return hipGetLastError();
}

// The latent's backward GEMV for n brush events at once (ian_grad_batch / ian_brush_step_batch): dz[i][j] = sum_k g[i][k] * Wb[j][k].
// A workgroup owns GB_RB (1 or 4) weight rows x GB_NB items and streams each of its weight rows ONCE for the whole item block (the batch-1
// kernel above reads the 6.5 MB slab once per latent row and per event); a lane keeps GB_RB x GB_NB accumulators.  Lane k-split,
// fma order, wave reduction and the final combination per (row, item) are the batch-1 kernel's: bitwise its dz for the same g.
// items != nullptr: the owner of (j, i) also applies z[i][j] = latent_step(z[i][j], dz[i][j], coef[i], gscale[i]) (ian_brush_item
// fields 5, 6).  Rows / items past the end are clamped for the loads and never stored.
constexpr int GB_NB = 8;
template <int GB_RB>
__global__ __launch_bounds__(256) void dense_bwd_gemv_batch_kernel(const float* __restrict__ g, int gs, const float* __restrict__ wb,
                                                                   int rows, int K, int n, const float* __restrict__ res,
                                                                   float* __restrict__ dz, int ds, float* __restrict__ z,
                                                                   const int* __restrict__ items) {
  __shared__ float part[4][GB_RB * GB_NB];
  const int r0 = blockIdx.x * GB_RB, i0 = blockIdx.y * GB_NB;
  const float* wr[GB_RB];
  const float* gr[GB_NB];
#pragma unroll
  for (int r = 0; r < GB_RB; ++r) wr[r] = wb + (size_t)min(r0 + r, rows - 1) * K;
#pragma unroll
  for (int i = 0; i < GB_NB; ++i) gr[i] = g + (size_t)min(i0 + i, n - 1) * gs;
  float acc[GB_RB][GB_NB];
#pragma unroll
  for (int r = 0; r < GB_RB; ++r)
#pragma unroll
    for (int i = 0; i < GB_NB; ++i) acc[r][i] = 0.f;
#pragma unroll 2
  for (int k = threadIdx.x * 4; k < K; k += 1024) {
    float4 w[GB_RB];
#pragma unroll
    for (int r = 0; r < GB_RB; ++r) w[r] = *reinterpret_cast<const float4*>(wr[r] + k);
#pragma unroll
    for (int i = 0; i < GB_NB; ++i) {
      const float4 a = *reinterpret_cast<const float4*>(gr[i] + k);
#pragma unroll
      for (int r = 0; r < GB_RB; ++r) {
        acc[r][i] = fmaf(a.x, w[r].x, acc[r][i]);
        acc[r][i] = fmaf(a.y, w[r].y, acc[r][i]);
        acc[r][i] = fmaf(a.z, w[r].z, acc[r][i]);
        acc[r][i] = fmaf(a.w, w[r].w, acc[r][i]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < GB_RB; ++r)
#pragma unroll
    for (int i = 0; i < GB_NB; ++i) {
      float v = acc[r][i];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][r * GB_NB + i] = v;
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= GB_RB * GB_NB) return;
  const int row = r0 + t / GB_NB, item = i0 + t % GB_NB;
  if (row >= rows || item >= n) return;
  float v = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
  const size_t o = (size_t)item * ds + row;
  if (res) v += res[o];
  dz[o] = v;
  if (z) z[o] = latent_step(z[o], v, __int_as_float(items[item * 7 + 5]), __int_as_float(items[item * 7 + 6]));
}
hipError_t launch_dense_bwd_gemv_batch(const float* g, int gs, const float* wb, int rows, int K, int n, const float* res, float* dz, int ds,
                                       float* upd_z, const int* items, hipStream_t s) {
  if ((K & 3) || (gs & 3) || n < 1 || (upd_z && !items)) return hipErrorInvalidValue;
  // 4-row blocks once they fill the 256 CUs; below that one row per workgroup (IAN_simple at n <= 8: 100 workgroups instead of 25).
  // The arithmetic per (row, item) does not depend on the block shape.
  const int iblocks = (n + GB_NB - 1) / GB_NB;
  if ((long long)((rows + 3) / 4) * iblocks >= 256)
    hipLaunchKernelGGL(dense_bwd_gemv_batch_kernel<4>, dim3((rows + 3) / 4, iblocks), dim3(256), 0, s, g, gs, wb, rows, K, n, res, dz, ds,
                       upd_z, items);
  else
    hipLaunchKernelGGL(dense_bwd_gemv_batch_kernel<1>, dim3(rows, iblocks), dim3(256), 0, s, g, gs, wb, rows, K, n, res, dz, ds, upd_z,
                       items);
  return hipGetLastError();
}

// The brush update on its own, when the latent's backward did not take the GEMV form (or fuse_latent_update is off).
// One event: cg = {coef, gscale} in device-readable memory so that a captured graph can be replayed with other values;
// z_mirror / g_mirror (or nullptr): the new latent and the gradient are also written there -- the pinned host block of the
// interactive loop (zero-copy), which spares the captured graph two device -> host copy nodes; cg may live there as well.
__global__ __launch_bounds__(128) void latent_update_kernel(float* __restrict__ z, const float* __restrict__ g,
                                                            const float* __restrict__ cg, int n, float* __restrict__ z_mirror,
                                                            float* __restrict__ g_mirror) {
  const int i = threadIdx.x;
  if (i < n) {
    const float gi = g[i];
    const float zn = latent_step(z[i], gi, cg[0], cg[1]);
    z[i] = zn;
    if (z_mirror) z_mirror[i] = zn;
    if (g_mirror) g_mirror[i] = gi;
  }
}
hipError_t launch_latent_update(float* z, const float* g, const float* cg, int n, float* z_mirror, float* g_mirror, hipStream_t s) {
  if (n > 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(latent_update_kernel, dim3(1), dim3(128), 0, s, z, g, cg, n, z_mirror, g_mirror);
  return hipGetLastError();
}
// n rows, (coef, gscale) per item from the ian_brush_item table: one workgroup per item
__global__ __launch_bounds__(128) void latent_update_batch_kernel(float* __restrict__ z, const float* __restrict__ g, int stride,
                                                                  const int* __restrict__ items, int zl) {
  const int item = blockIdx.x;
  const float coef = __int_as_float(items[item * 7 + 5]), gscale = __int_as_float(items[item * 7 + 6]);
  for (int j = threadIdx.x; j < zl; j += 128) {
    const size_t o = (size_t)item * stride + j;
    z[o] = latent_step(z[o], g[o], coef, gscale);
  }
}
hipError_t launch_latent_update_batch(float* z, const float* g, int stride, const int* items, int n, int zl, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(latent_update_batch_kernel, dim3(n), dim3(128), 0, s, z, g, stride, items, zl);
  return hipGetLastError();
}

}  // namespace ian
