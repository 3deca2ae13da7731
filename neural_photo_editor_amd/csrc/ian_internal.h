// Internal declarations shared by the runtime (ian_runtime.cpp) and the device code (kernels_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ian_tg_types.h"

namespace ian {

// the tap GEMM's host-built tables (TgTap, TgTapE, TgClass, TgItem, TgTile) and its two row orders: ian_tg_types.h

enum { TG_EPI_FWD = 0, TG_EPI_BWD = 1 };

// Batch statistics computed in the epilogue of the launch that PRODUCES the tensor (round 5: the training step's colstats passes
// re-read every normalised tensor -- 5 GB per update).  Per output row tile and channel, float64 partial sums over the tile's rows:
//   mode 1 (forward, Lasagne batch_norm statistics): s1 = sum v, s2 = sum v*v of the stored value v, every element widened first;
//   mode 2 (backward: dbeta, dgamma): g = v * act'(a), s1 = sum g, s2 = sum g * xhat, xhat = (yraw - mean) * inv_std -- float32
//           products, four rows added in float32, the rest in float64 (the arithmetic of colstats_kernel, kernels_train.hip).
// partial[chunk][2][C] doubles, chunk = (row tile index) * ncls + class: the second stage (tree over chunks) is unchanged, and
// the chunk boundaries (multiples of the tile height within the (image, pixel) row order) do not depend on the batch.
// Only launches whose tiles are not split over K carry it (the host falls back to colstats otherwise).
struct TgStats {
  double* partial = nullptr;
  const float* a = nullptr;       // mode 2: post-activation forward value (for act')
  const float* yraw = nullptr;    // mode 2: pre-normalisation value
  const float* mean = nullptr;
  const float* inv_std = nullptr;
  int mode = 0, act = 0, C = 0, ncls = 1;
};

struct TgEpilogue {
  const float* scale;  // per output channel (folded BN gamma*inv_std) or nullptr (=1)
  const float* shift;  // per output channel (folded beta/bias) or nullptr (=0)
  const float* res;    // residual tensor, same layout as y, added before the affine; or nullptr
  const float* yfwd;   // BWD: forward output of the layer whose pre-activation gradient is produced
  int act;             // enum ian_act
  int scale_period;    // 0: scale/shift indexed by channel; >0: by (element offset % period) -- per-feature
                       // batch-norm of a dense layer whose output is viewed as an NHWC map (IAN_simple.py:129-139)
  int mode;            // TG_EPI_FWD: y = act((acc+res)*scale+shift)
                       // TG_EPI_BWD: y = (acc [+res]) * act'(yfwd) * scale   (gradient wrt pre-affine value)
  TgStats st;          // statistics of the stored values (training step), or mode 0
};

struct TgParams {
  const float* x;
  const float* w;
  float* y;
  float* slab;
  const TgItem* items;
  const TgClass* classes;
  const TgTap* taps;         // the layer's list (tapgemm_bf16x3_kernel)
  const TgTapE* ttaps;       // the schedule's per-tile lists (tapgemm_kernel; TgItem::tap0 indexes it)
  TgEpilogue epi;
  int M;                     // rows: images * QH * QW, position-major QH * QW << b_shift
  int b_shift, nimg;         // row order (ian_tg_types.h): b_shift < 0 image-major, else position-major with 1 << b_shift >= nimg rows per position
  int IH, IW, Cin;           // Cin = padded input channels = pixel stride of x (multiple of 32)
  int qw_shift, qhw_shift;   // QW = 1<<qw_shift, QH*QW = 1<<qhw_shift
  int si, by, bx;            // input coordinate = q*si + b + d
  int so;                    // output coordinate = q*so + p
  int OH, OW, Cout, y_stride;
  int CoutPad;
  unsigned x_bytes, w_bytes;  // buffer-descriptor extents (out-of-range offsets read as zero)
  int variant;                // K-loop schedule (kernels_tapgemm.hip)
  const TgTile* tiles;        // split-K with the combine fused into this launch (fused != 0): the tile table ...
  int* counters;              // ... and one arrival counter per tile (zero between launches)
  float* raw;                 // fused == 2: one zero-at-rest accumulation tile per output tile (float atomics)
  int fused;                  // 0: slabs + a tapgemm_reduce launch; 1: write-through slabs combined by the tile's last arriver;
                              // 2: atomic accumulation into `raw`, epilogue by the last arriver (kernels_tapgemm.hip)
  const unsigned short* wsplit;  // tapgemm_bf16x3_kernel: the weights pre-split into a bf16 hi plane followed by a lo plane (or nullptr)
  int bf_sched;                  // ... and its K-loop schedule (0..2)
  int noepi;                     // libian_ablation.so: skip everything behind the K loop (timing-only)
  unsigned y_bytes;              // extent of y (and of res / yfwd, same layout) for the buffer-descriptor epilogue; 0: above the descriptor range, general epilogue
};

struct TgReduceParams {
  const float* slab;
  float* y;
  const TgTile* tiles;
  const TgClass* classes;
  TgEpilogue epi;
  int M, qw_shift, qhw_shift, so, OH, OW, Cout, y_stride;
  int b_shift, nimg;   // row order, as TgParams
};

// TgParams::variant: the K-loop schedules of tapgemm_kernel (described at the head of kernels_tapgemm.hip).  The numbers are the
// values of the options tg_variant / tg_variant_force and of the tune cache; this enum and the two predicates below are the
// ONE place that says which of them exist.
enum TgSchedule {
  TG_SCHED_PLAIN = 0,        // ablation: compiler-scheduled
  TG_SCHED_SPLIT = 1,        // LDS stores between the two halves of the MFMAs
  TG_SCHED_ROTATED = 2,      // last k group's MFMAs behind the barrier
  TG_SCHED_DMA = 3,          // ablation: LDS-DMA staging
  TG_SCHED_QUEUE3 = 4,       // register queue, three K-steps of loads in flight
  TG_VARIANT_BF16X3 = 5,     // not a schedule of tapgemm_kernel: tapgemm_bf16x3_kernel (opt-in, ian_set_option("tg_bf16x3", 1))
  TG_SCHED_ROTATED_PIN = 6,  // 2 with every fragment read pinned
  TG_SCHED_AHEAD2 = 7,       // rotated, two K-steps of loads in flight, per-tap addressing
  TG_SCHED_AHEAD3 = 8,       // ablation: 7's structure with three K-steps in flight
  TG_ABL2_FIRST = 10, TG_ABL2_LAST = 12,   // ablation: timing-only variants of schedule 2 (WRONG results)
  TG_ABL7_FIRST = 17, TG_ABL7_LAST = 23,   // ablation: timing-only variants of schedule 7 (WRONG results)
};
// the schedules every build carries: option values, autotune candidates, tune-cache entries
static inline bool tg_schedule_shipped(int v) {
  return v == TG_SCHED_SPLIT || v == TG_SCHED_ROTATED || v == TG_SCHED_QUEUE3 || v == TG_SCHED_ROTATED_PIN || v == TG_SCHED_AHEAD2;
}
// "is v a K-loop schedule this library can launch": libian_ablation.so adds the negative results and the timing-only variants
static inline bool tg_schedule_valid(int v) {
#ifdef IAN_ABLATION
  if (v == TG_SCHED_PLAIN || v == TG_SCHED_DMA || v == TG_SCHED_AHEAD3 || (v >= TG_ABL2_FIRST && v <= TG_ABL2_LAST) || (v >= TG_ABL7_FIRST && v <= TG_ABL7_LAST)) return true;
#endif
  return tg_schedule_shipped(v);
}
enum TgConfig { TG_128x128 = 0, TG_128x64 = 1, TG_64x64 = 2, TG_32x128 = 3, TG_256x128 = 4, TG_128x32 = 5,
                TG_128x128W8 = 6 /* 128x128 tile, 8 waves of 64x32 */, TG_128x64W8 = 7 /* 128x64 tile, 8 waves of 32x32 */,
                TG_NCONFIG = 8 };
struct TgShape {
  int bm, bn;
};
static inline TgShape tg_shape(int cfg) {
  switch (cfg) {
    case TG_128x128:
    case TG_128x128W8: return {128, 128};
    case TG_128x64:
    case TG_128x64W8: return {128, 64};
    case TG_64x64: return {64, 64};
    case TG_32x128: return {32, 128};
    case TG_128x32: return {128, 32};
    default: return {256, 128};
  }
}

// tile configurations whose kernel carries the in-launch split-K combine (TgParams::fused != 0): the small 4-wave tiles the
// batch-1 chains use.  The large tiles are compiled WITHOUT that epilogue (it cost the 256x128 tile 95 spilled VGPRs).
static inline bool tg_fuse_supported(int cfg) {
#ifdef IAN_NO_TG_FUSE   // libian_nofuse.so: the epilogue is compiled out of every tile (A/B build, build.py)
  (void)cfg;
  return false;
#endif
  return cfg == TG_32x128 || cfg == TG_64x64 || cfg == TG_128x64 || cfg == TG_128x32;
}

// tile configurations tapgemm_bf16x3_kernel is instantiated for (its staging pass covers 16 x waves rows: 4 threads per row)
static inline bool tg_bf16x3_supported(int cfg) {
  return cfg == TG_128x128 || cfg == TG_128x64 || cfg == TG_64x64 || cfg == TG_128x128W8;   // 256x128 compiles too but spills (1152 B of scratch)
}

// launches that can carry the GEMM-epilogue batch statistics (TgStats): a separate kernel instantiation exists for the
// register-staged K-loop schedules 1 / 2 of every tile up to 128 x 128
// -- in libian_ablation.so.  The product library carries none of them (measured: the training update got 4 % SLOWER; the colstats
// passes this replaces are HBM-bound and already run under the weight-gradient GEMMs of the second stream, the epilogue version
// puts the same bytes on the MFMA-bound kernel's critical path): there every request is answered with 0 chunks.
static inline bool tg_stats_supported(int cfg, int variant) {
#ifdef IAN_ABLATION
  return cfg != TG_256x128 && (variant == TG_SCHED_SPLIT || variant == TG_SCHED_ROTATED);
#else
  (void)cfg; (void)variant;
  return false;
#endif
}

// one-image form of the 5x5/s2 transposed conv and of its backward-data (kernels_b1.hip): whole contraction per
// workgroup (4x4 output positions x 16 channels), weights repacked as one contiguous stream per workgroup
struct B1Params {
  const float* x;      // NHWC input of this kernel (activation, or dL/d(pre-epilogue output) for the backward form)
  const float* w;      // packed [class][channel slice][tap][Cr/32][64 lanes][8]
  float* y;
  const float* scale;  // as TgEpilogue
  const float* shift;
  const float* yfwd;
  const float* res;
  long long cls_off[4];  // float offset of each output-parity class's weights (backward form: one class)
  int act, bwd, scale_period;
  int IH, IW, Cr, xs;    // input grid, reduction channels (multiple of 32), input pixel stride
  int OH, OW, ys;        // output grid and pixel stride
  int ntiles, tiles_x, nslices;  // 4x4 position blocks (per class), blocks per row, 16-channel output slices
  unsigned x_bytes;              // extent of x for the buffer descriptor (out-of-range offsets read as zero)
  int kshift;                    // log2(Cr / 32)
  int dbg;                       // scripts/ubench/b1conv_bench.cpp only (timing ablations); 0 in the product
};
hipError_t launch_b1conv(const B1Params& p, int mode, hipStream_t s);

hipError_t launch_tapgemm(int cfg, const TgParams& p, int nitems, hipStream_t s);
// fp32 weights -> bf16 hi plane | lo plane (2 n values) for tapgemm_bf16x3_kernel
hipError_t launch_wsplit(const float* w, unsigned short* out, long long n, hipStream_t s);
// ian_box_probe: register-only fp32-MFMA loop, `blocks` workgroups of 256 threads, 4 x iters MFMAs per wave (kernels_misc.hip)
hipError_t launch_box_probe(const float* in, float* out, int blocks, int iters, hipStream_t s);
// kp > 1: four lanes share the slabs of one output element (few tiles, many slabs: batch 1)
hipError_t launch_tapgemm_reduce(int cfg, const TgReduceParams& p, int ntiles, int kp, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// edge layers (3 image channels) and small ops
// ---------------------------------------------------------------------------------------------
// enc_conv1: x NCHW [n,3,H,W] -> y NHWC [n,H/2,W/2,Cout], 5x5 s2 p2 + bias + act. w packed [75][Cout].
hipError_t launch_conv1_nchw(const float* x, const float* w, const float* scale, const float* shift, float* y, int n,
                             int H, int W, int Cout, int act, hipStream_t s);
// dec_out: x NHWC [n,H,W,Cin] -> y NCHW [n,Cout(<=4),2H,2W], 5x5 s2 transposed conv + affine + act.
// w packed [25 (ky,kx)][Cout4=4][Cin].
hipError_t launch_deconv_out_nchw(const float* x, const float* w, const float* scale, const float* shift, float* y,
                                  int n, int H, int W, int Cin, int Cout, int act, hipStream_t s);
hipError_t launch_dense_fwd_gemv(const float* x, const float* w, int K, int nout, const float* scale, const float* shift, int act,
                                 float* y, hipStream_t s);
// upd_z != nullptr: row j's workgroup also applies the brush update z[j] += cg[0] * (dz[j] * cg[1]) (and mirrors z, dz)
hipError_t launch_dense_bwd_gemv(const float* g, const float* wb, int rows, int K, const float* res, float* dz, float* upd_z,
                                 const float* upd_cg, float* z_mirror, float* g_mirror, hipStream_t s);
// n brush events (ian_grad_batch / ian_brush_step_batch): g [n][gs], dz / z [n][ds]; items = the device copy of the ian_brush_item
// table (7 words per item), read for (coef, gscale) when upd_z != nullptr
hipError_t launch_dense_bwd_gemv_batch(const float* g, int gs, const float* wb, int rows, int K, int n, const float* res, float* dz, int ds,
                                       float* upd_z, const int* items, hipStream_t s);
hipError_t launch_latent_update_batch(float* z, const float* g, int stride, const int* items, int n, int zl, hipStream_t s);
hipError_t launch_deconv_out_px(const float* x, const float* w, const float* scale, const float* shift, float* y, float* mirror, int n,
                                int H, int W, int Cin, int Cout, int act, hipStream_t s);

// y = act(x*scale[c]+shift[c]) on NHWC tensors (pixel stride = stride)
hipError_t launch_affine(const float* x, float* y, const float* scale, const float* shift, long long npix, int C,
                         int stride, int act, hipStream_t s);
// MADE x2 + IAF on latent rows (stride zs): z' = (z - made_mu(z)) / exp(made_ls(z)); weights pre-masked [6][100][100]+[6][100]
hipError_t launch_made_iaf(const float* z, float* zo, const float* wts, const float* bias, int n, int d, int zs,
                           hipStream_t s);
// beta_layer x3 + concat -> NCHW output [n,3,H,W]; R,G,B are NHWC with 2 channels (stride rs)
hipError_t launch_beta(const float* R, const float* G, const float* B, float* y, int n, int hw, int rs, hipStream_t s);
// channel concat of two NHWC tensors
hipError_t launch_concat2(const float* a, int ca, int sa, const float* b, int cb, int sb, float* y, int sy,
                          long long npix, hipStream_t s);
// layout / copy helpers
hipError_t launch_rows_copy(const float* src, int src_stride, float* dst, int dst_stride, int n, int c, hipStream_t s);
hipError_t launch_nhwc_to_nchw(const float* src, int stride, float* dst, int n, int hw, int c, hipStream_t s);
// Where the loss seeds of a latent-brush launch (API.py:59,64; kernels_brush.hip) come from.  Passed to the kernels by value.
struct BrushSeedSrc {
  const int* table = nullptr;     // device-readable ian_brush_item rows (7 words: c1, r1, c2, r2, loss kind, coef, gscale), one per
                                  // item; one event = one row.  nullptr: the rectangle and loss kind below
  const float* rgb = nullptr;     // the target colour images [n,3,H,W] of the items with loss kind 1 ...
  const float* colour = nullptr;  // ... or, with a table, their constant target colours [n][3]
  int c1 = 0, r1 = 0, c2 = 0, r2 = 0, mode = 0;   // without a table (the eager single call, n = 1)
  // ... or, with a table, each item's own photo (ian_session_fit): the target of element o of item i is tanh_tab[gim[ids[i]*12288 + o]]
  const unsigned char* gim = nullptr;   // the session pool's GIM base, u8 [capacity][3*64*64]
  const int* ids = nullptr;             // device int[n]: the items' session ids
  const float* tanh_tab = nullptr;      // device float[256]: to_tanh of the uint8 levels (ian_session_tanh_table)
  // ... or, with a table, another picture of the pool, shifted (ian_session_clone; needs gim and tanh_tab too): the target of element
  // o of item i is tanh_tab[F[clone[3i] * 12288 + o + clone[3i + 2]]], F = gim, im or recon for clone[3i + 1] = 0, 1, 2
  const unsigned char* im = nullptr;    // the pool's IM and RECON bases, as gim
  const unsigned char* recon = nullptr;
  const int* clone = nullptr;           // device int[n][3]: source session, field selector, shift dr * 64 + dc
  // ... and, with a table and colours or a clone's sources, a brush tip per item (ian_session_brush_tip, ian_session_stamp_soft): inside
  // its rectangle item i's loss is weighted by tips[tipsel[i] * 4096 + (r - r1) * 64 + (c - c1)] in the place of the flat 1/N;
  // tipsel[i] = -1 keeps 1/N.  The photo target, the colour images of the stateless batched calls and the eager single call have no
  // weighted form.
  const float* tips = nullptr;          // device float[count][64 * 64], row stride 64 (ian_sessions_set_tip)
  const int* tipsel = nullptr;          // device int[n]: the items' tip indices
};
// d loss / d x_hat of n items: g NCHW [n,3,H,W], zero outside each item's rectangle
hipError_t launch_brush_seed(const BrushSeedSrc& src, int n, const float* xhat, float* g, int H, int W, hipStream_t s);
// the same seed + the output activation's derivative + the backward-data of the dec_out-like layer below, in one launch (needs a
// table): xhat NCHW [n,Cout,2H,2W], dx / yfwd NHWC [n,H,W,Cin]
hipError_t launch_brush_seed_dec_out(const BrushSeedSrc& src, int n, const float* xhat, int out_act, const float* oscale, const float* w,
                                     float* dx, const float* yfwd, const float* scale, int H, int W, int Cin, int Cout, int act,
                                     hipStream_t s);
// backward of dec_out-like layer: g NCHW [n,Cout,2H,2W] (already multiplied by act') -> dx NHWC [n,H,W,Cin]
hipError_t launch_deconv_out_bwd(const float* g, const float* w, float* dx, const float* yfwd, const float* scale,
                                 int n, int H, int W, int Cin, int Cout, int act, hipStream_t s);
// elementwise: g = g * act'(y) * scale  (NCHW small tensors, c channels of hw pixels)
hipError_t launch_dact_nchw(float* g, const float* y, const float* scale, int n, int c, int hw, int act,
                            hipStream_t s);

// few-filter MDCL forward on the VALU (RGB-Beta head).  One launch computes up to MH_MAXCO output filters that read
// the SAME input map with the SAME tap list -- the filters may belong to different layers (IAN.py:183-199: R, G_a
// and B_a all read the 128-channel feature map), each with its own weights, destination, residual and activation.
constexpr int MH_MAXCO = 8;
struct MdcHeadArgs {
  const float* x;              // NHWC, pixel stride xs
  const float* w[MH_MAXCO];    // per output filter: its row in a forward slab; tap t at + t*w_tap_stride
  const float* res[MH_MAXCO];  // per output filter: residual tensor (same addressing as y) or nullptr
  float* y[MH_MAXCO];          // per output filter: destination tensor base
  float scale[MH_MAXCO], shift[MH_MAXCO];
  int ys[MH_MAXCO], yc[MH_MAXCO], act[MH_MAXCO];  // pixel stride, channel index, activation
  int H, W, xs, ntaps;
  long long w_tap_stride;
  signed char dy[48], dx[48];
};
hipError_t launch_mdc_head(const MdcHeadArgs& a, int n, int Cin, int Cout, hipStream_t s);
// MDCL with <= 4 real input channels on the VALU (forward of G_b / B_b, backward-data of every 2-filter head layer)
struct MdcThinArgs {
  const float* x;  // NHWC, pixel stride xs (>= 4 floats readable per pixel)
  const float* w;  // slab [tap][CoutPad][CinPad]
  const float* res;
  const float* scale;
  const float* shift;
  float* y;        // NHWC, pixel stride ys
  int n, H, W, xs, ys, Cout, CoutPad, CinPad, ntaps, act;
  int no_tile;     // 1: never take the LDS-staged form (A/B tests)
  signed char dy[48], dx[48];
};
hipError_t launch_mdc_thin(const MdcThinArgs& a, hipStream_t s);
// few-filter MDCL backward-weight on the VALU; partial: [nblocks][ntaps][2 or 4][Cin] floats
struct MdcHeadWgradArgs {
  const float* x;   // layer input, NHWC, pixel stride xs
  const float* dy;  // gradient wrt the pre-activation output, NHWC, pixel stride dys
  float* partial;
  int H, W, xs, dys, ntaps, total_tiles;
  signed char dy_[48], dx_[48];
};
hipError_t launch_mdc_head_wgrad(const MdcHeadWgradArgs& a, int nblocks, int Cin, int Cout, float* dS, int f_rows,
                                 int f_cols, hipStream_t s);
// RGB-Beta head in two launches (kernels_head.hip).  head6: the six filters that read the 128-channel map (three
// 2-filter MDCL layers with one tap list) -> compact [n][H][W][8] map (filters 0..5, 2 floats padding).
struct HeadFusedArgs {
  const float* x;          // NHWC, pixel stride xs, 128 channels
  const float *w0, *w1, *w2;  // forward slabs [tap][CoutPad][128] of the three layers (rows 0,1 used)
  float* out;              // compact map
  const int* itab;         // 44 slots: [0,12) taps with dy = 0, then 4 per dy = -4..-1, 1..4; tap id | (dx+64) << 8, empty = -1
  const float* ftab;       // [0..5] scale, [8..13] shift, [16..21] activation code of the six filters
  int H, W, xs, ntaps, bands, halo;
  long long w_tap_stride;
};
hipError_t launch_head6(const HeadFusedArgs& a, int n, hipStream_t s);
hipError_t launch_head6_zbuild(const float* dy0, const float* dy1, const float* dy2, int dys, float* Z, int zs, int H, int W,
                               int ntaps, const int* taps, long long npix, hipStream_t s, int max_shift /* largest |dy|, |dx| of the taps; < 0: the per-(pixel, tap) form */);
hipError_t launch_head6_wcat(const float* slab, int f_rows, int f_cols, int kk, int ntaps, float* wcat, int nout, hipStream_t s);
hipError_t launch_head6_dS_scatter(const float* dWref, int nout, int kk, int ntaps, float* dS, int f_rows, int f_cols, hipStream_t s);
hipError_t launch_head6_scatter(const float* comp, float* y0, float* y1, float* y2, int ys, long long npix, hipStream_t s);
struct HeadTailArgs {
  const float* comp;       // compact map: (R0,R1,Ga0,Ga1,Ba0,Ba1,-,-) per pixel
  const float *w_gb, *w_bb;  // forward slabs of G_b (2 in) and B_b (4 in): [tap][CoutPad][CinPad]
  float* out;              // NCHW [n][3][H][W]
  long long gb_tap_stride, bb_tap_stride;
  int gb_cin, bb_cin;      // CinPad of the two slabs
  float scale_g[2], shift_g[2], scale_b[2], shift_b[2];
  int act_g, act_b, H, W, ntaps;
  signed char dy[48], dx[48];
};
hipError_t launch_head_tail(const HeadTailArgs& a, int n, hipStream_t s);

// dec_out of IAN_simple on the matrix cores (kernels_head.hip): x NHWC [n][H][32][128] -> y NCHW [n][Cout][2H][64]
struct DeconvSmallArgs {
  const float* x;
  const float* w;      // edge packing [25 (ky,kx)][4][128]
  const float* scale;  // per output channel or nullptr
  const float* shift;
  float* y;
  int H, W, xs, bands, act;
  int balanced;        // Cout = 3: the 16 x 16 MFMA tiling, five blocks per SIMD (kernels_head.hip; option dec_out_bal)
};
hipError_t launch_deconv_small(const DeconvSmallArgs& a, int n, int Cout, hipStream_t s);

// NPE.paint's photo blend and the uint8 image conversion on the device (kernels_npe.hip; NPE.py:218-231, 110, 261)
struct PhotoBlendArgs {
  const float* xhat;           // decoder output, NCHW [3][64][64]
  const unsigned char* recon;  // RECON uint8 [3][64][64]
  const float* error;          // ERROR float32 [3][64][64]
  unsigned char* im;           // IM uint8 [3][64][64]
  double* mask;                // MASK float64 [64][64] or nullptr
  double w[8];                 // Gaussian weights, centre outwards (scipy _gaussian_kernel1d)
  int radius;
  float* field;                // nullptr, or float32 [3][64][64]: float32(MASK * (float64(DELTA) - float64(ERROR))), the edit field of
                               // full-resolution sessions (npe_ops.edit_field); the other outputs do not depend on it
};
// what photo_blend_image<true> takes besides (local edit sessions; npe_ops.photo_blend_local / umask_paint)
struct PhotoLocalArgs {
  double* umask;               // the session's UMASK float64 [64][64]: MASK_L = MASK * UMASK; nullptr: MASK_L = MASK
  const double* falloff;       // float64 [64], npe_ops.local_falloff_table; nullptr, or an empty box: no footprint is added to UMASK
  int c1, r1, c2, r2;          // the brush rectangle whose footprint is max-ed into UMASK first
  int dampen;                  // != 0: D = where(to_tanh(float32(RECON)) + D > thresh, thresh - to_tanh(float32(RECON)), D)
  double thresh;
};
hipError_t launch_photo_blend(const PhotoBlendArgs& a, hipStream_t s);
// n images at once (blockIdx.y = item): every pointer of `a` is the base of an [n]-leading array, the weights are shared
hipError_t launch_photo_blend_batch(const PhotoBlendArgs& a, int n, hipStream_t s);
hipError_t launch_latent_update(float* z, const float* g, const float* cg, int n, float* z_mirror, float* g_mirror, hipStream_t s);
hipError_t launch_keep_warm(const int* flag, long long max_ticks, hipStream_t s);   // experiment: see kernels_npe.hip
hipError_t launch_to_uint8(const float* x, unsigned char* y, long long n, hipStream_t s);

// device-resident edit sessions (kernels_session.hip; ian_session_*): the pool's arrays, one row per session id.  Passed to kernels by
// value.  The runtime allocates, moves, frees and reads every pointer member through its row in SESS_COLUMNS (ian_rt_session.inc): a
// new array is a member here and a row there.
struct SessionPool {
  unsigned char* gim;     // GIM   u8 [capacity][3*64*64]
  unsigned char* im;      // IM    u8 [capacity][3*64*64]
  unsigned char* recon;   // RECON u8 [capacity][3*64*64]
  float* error;           // ERROR f32[capacity][3*64*64]
  float* z;               // Z     f32[capacity][zl]
  int* mode;              // 0 = photo, 1 = sample (NPE.py SAMPLE_FLAG)
  int zl;
  // full-resolution sessions (ian_sessions_reserve_hires); all nullptr / 0 without that reservation, and then nothing below is touched
  unsigned char* src;     // SRC   u8 [capacity][3*S*S], S = 64 * scale: the photo at its own resolution
  float* field;           // FIELD f32[capacity][3*64*64]: what the last call displayed, as an edit field (kind 0) or as x (kind 1)
  int* kind;              // FIELD_KIND
  int scale;              // 1..16
  // local edits (ian_sessions_reserve_local); both nullptr without that reservation, and then session_blend_kernel runs as ever
  double* umask;          // UMASK f64[capacity][64*64]: where the user has brushed (npe_ops.umask_paint)
  int* local;             // LOCAL int[capacity]: bit 0 = the blend is masked by UMASK, bit 1 = dampen
};
// undo history (ian_sessions_reserve_history): a ring of depth + 1 saved states per session, slot k of session id in row
// id * (depth + 1) + k of each array.  All nullptr / 0 without that reservation.  Beside the pool, not in it: SessionPool goes to every
// session kernel by value, and a member more would move the arguments of all of them; only the two history kernels take this one.
// The runtime manages these pointers through SESS_COLUMNS like the pool's.
struct SessionRings {
  float* hist_z;          // f32[capacity][depth+1][zl]: saved Z rows
  double* hist_umask;     // f64[capacity][depth+1][64*64]: saved UMASK rows; nullptr when the pool had no local reservation
  int depth;              // 1..64
};
// open, input side: row i = photos[i] (u8 [n][3*64*64]) or, without photos, the session's GIM (source 0) / IM (source 1) -> GIM, IM and
// x[i] = table[byte] (float32 NCHW, the encoder's input slot); ids = device int[n]; table = 256 floats, to_tanh per level
hipError_t launch_session_open_in(const unsigned char* photos, const SessionPool& P, const int* ids, int source, const float* table,
                                  float* x, int n, hipStream_t s);
// open / sample, output side: RECON, ERROR (against IM), Z (row i of the latent slot, stride zs) and the mode flag of session ids[i];
// shown (or nullptr) [n][3*64*64] receives RECON (shown_recon != 0) or IM
hipError_t launch_session_store(const float* xhat, const float* zslot, int zs, const SessionPool& P, const int* ids, int new_mode,
                                int shown_recon, unsigned char* shown, int n, hipStream_t s);
hipError_t launch_session_gather_z(const SessionPool& P, const int* ids, float* zslot, int zs, int n, hipStream_t s);
struct SessionBlendArgs {
  const float* xhat;      // decoder output, NCHW [n][3][64][64]
  const float* zslot;     // latent slot, row i = item i (stride zs): written back to the session's Z
  int zs;
  SessionPool P;
  const int* ids;         // device int[n]
  const int* items;       // device ian_brush_item table (7 words per item; word 4 = loss kind) or nullptr = every item paints
  unsigned char* shown;   // [n][3*64*64]
  int store;              // photo mode: != 0 the blend also becomes the session's IM
  double w[8];            // as PhotoBlendArgs
  int radius;
  const double* falloff;  // pools with the local reservation: device f64[64] (ian_sessions_set_local) and the dampen threshold
  double thresh;
  const int* tips;        // pools with the local reservation under ian_sessions_set_soft_mask: device int[n], the items' tip indices.  An
                          // item with a tip >= 0 adds no rectangle footprint: launch_session_tip_umask added its tip's.  nullptr: none
};
// P.umask == nullptr: session_blend_kernel; otherwise session_blend_local_kernel, which reads the sessions' LOCAL flags
hipError_t launch_session_blend(const SessionBlendArgs& a, int n, hipStream_t s);
// UMASK row of session ids[i] := 0 and, with flags (device int[n]), LOCAL[ids[i]] := flags[i]
hipError_t launch_session_local_set(const SessionPool& P, const int* ids, const int* flags, int n, hipStream_t s);
// ian_session_stroke: UMASK row of session ids[g] := max(UMASK, the footprint of every rectangle of stroke g) for g = first .. first +
// n - 1, under the blend's conditions (LOCAL bit 0, a paint stroke, photo mode).  items = the call's ian_brush_item rows (7 words
// each), step after step; rows = device int[steps + 1]: step k's rows start at rows[k], one per stroke with more than k points in
// stroke order, so stroke g's row of step k is rows[k] + g while g < rows[k + 1] - rows[k]; falloff = device f64[64].
// tips (device int[], indexed like ids; nullptr: none): a stroke whose tip index is >= 0 is launch_session_tip_umask's and is skipped.
constexpr int STROKE_MAX_POINTS = 64;
hipError_t launch_session_stroke_umask(const SessionPool& P, const int* ids, const int* items, const int* rows, int steps, int first,
                                       const double* falloff, const int* tips, int n, hipStream_t s);
// ian_sessions_set_soft_mask: the same for the items with a tip: UMASK row of session ids[g] := max(UMASK, npe_ops.tip_footprint of
// every rectangle of item g with the shape of tip tips[g]) under the same conditions; an item with tips[g] < 0 is skipped.  shapes =
// device f64[count][64 * 64] (tip_shape_slot).  rows == nullptr: item g has the one row g (a brush or clone event), steps = 1.
hipError_t launch_session_tip_umask(const SessionPool& P, const int* ids, const int* items, const int* rows, int steps, int first,
                                    const double* falloff, const int* tips, const double* shapes, int n, hipStream_t s);
// ian_session_fit.  begin: IM := GIM of sessions ids[0..n).  adam: rows 0..n-1 of the latent slot z (stride zs) move by one Adam step
// (ian_fit_step.h) on the gradient rows g (same stride); m, v = the moments, [n][zl]; c1, c2 = the step's bias corrections.
// loss: loss[i * loss_stride] = the float64 mean of (xhat[i] - table[GIM of ids[i]])^2 over the rectangle of row i of the
// ian_brush_item table `items`, 0 for an empty one; xhat NCHW [n][3][64][64].
hipError_t launch_session_fit_begin(const SessionPool& P, const int* ids, int n, hipStream_t s);
hipError_t launch_session_fit_adam(float* z, const float* g, int zs, float* m, float* v, int n, int zl, float lr, float c1, float c2,
                                   hipStream_t s);
hipError_t launch_session_fit_loss(const float* xhat, const SessionPool& P, const int* ids, const int* items, const float* table,
                                   double* loss, int loss_stride, int n, hipStream_t s);
// undo history.  ids / save / load = device int[n]; slots are 0..depth (a slot outside that range is skipped).
// save: ring slot save[i] of session ids[i] := its live Z row (and UMASK row, when hist_umask exists)
hipError_t launch_session_history_save(const SessionPool& P, const SessionRings& R, const int* ids, const int* save, int n, hipStream_t s);
// move: the same save where save[i] >= 0, then ring slot load[i] -> row i of the latent slot (stride zs; the blend that follows writes
// it back to the session's Z) and -> the session's UMASK row
hipError_t launch_session_history_move(const SessionPool& P, const SessionRings& R, const int* ids, const int* save, const int* load,
                                       float* zslot, int zs, int n, hipStream_t s);
// saved sessions (ian_session_save / ian_session_load): a record's body is every array the pool has, each padded to 16
// bytes.  One entry per array, built by the runtime from SESS_COLUMNS; passed to the two kernels by value.
enum SessionRecordRule { SESS_REC_PLAIN = 0, SESS_REC_SOURCE = 1 /* zero / unwritten without a source */, SESS_REC_RING = 2 /* slots of a history ring */ };
struct SessionRecordCol {
  unsigned off;             // byte offset in the body, a multiple of 16
  unsigned unit;            // bytes of one row (of one ring slot), a multiple of 4; a multiple of 16 takes the 16-byte path
  unsigned slots;           // 1, or depth + 1 for a ring
  unsigned short member;    // byte offset of the array's pointer in SessionPool / SessionRings
  unsigned char in_rings;   // which of the two
  unsigned char rule;       // SessionRecordRule
};
constexpr int SESS_REC_MAX_COLS = 13;
struct SessionRecordCols {
  int ncols;
  unsigned body_bytes;      // a multiple of 16
  SessionRecordCol col[SESS_REC_MAX_COLS];
};
struct SessionRecordBases {   // what the launchers hand the kernels: the pointer of each table entry's array
  char* p[SESS_REC_MAX_COLS];
};
// items = device int[n][4]: session id, has_source, the ring's base slot, the history's length.  body = device bytes [n][body_bytes],
// 16-byte aligned.  pack: the sessions' rows -> body, history entry k (ring slot (base + k) % slots) -> record slot k, zeros for
// the slots >= length, for SRC without a source and for the padding.  unpack: body -> rows, record slot k -> ring slot k, and what
// pack zero-fills is not written.
hipError_t launch_session_pack(const SessionPool& P, const SessionRings& R, const SessionRecordCols& T, const int* items,
                               unsigned char* body, int n, hipStream_t s);
hipError_t launch_session_unpack(const SessionPool& P, const SessionRings& R, const SessionRecordCols& T, const int* items,
                                 const unsigned char* body, int n, hipStream_t s);
// full-resolution open, input side: SRC row of ids[i] := photos[i] (u8 [n][3*S*S]; nullptr: the row already holds the photo), its exact
// box mean -> GIM, IM and x[i] = table[byte], the outputs of launch_session_open_in
hipError_t launch_session_hires_open(const unsigned char* photos, const SessionPool& P, const int* ids, const float* table, float* x, int n,
                                     hipStream_t s);
// The window launches (kernels_window.hip).  They take table (the oriented one has no guided form), zoom and format:
//   table   nullptr: the plain arithmetic.  Otherwise device float[766], the range weights by summed absolute byte difference
//           (ian_sessions_reserve_guide; ian_sessions_reserve_edges, 4.13): the guided arithmetic, the guide of a
//           session being its own GIM and the photo the session's SRC or the canvas.
//   zoom    1: the windows as they are.  2..16: the same windows at 1/zoom.  Output pixel (Y, X) of window i is
//           npe_ops.zoom_box_mean of the 1:1 result of the source window (x, y, zoom * vw, zoom * vh), which must lie inside the
//           picture: x and y of views / windows stay in full-resolution pixels, vw x vh is the OUTPUT size, out is never nullptr
//           and 4-byte aligned.  No full-resolution result is written anywhere.
//   format  the pixels of out (ian_sessions_set_pixels; npe_ops.pack_window).  PIXELS_PLANAR: u8 [n][3][vh][vw], the
//           kernels as they were before the formats.  PIXELS_RGB / _RGBA / _BGRA: interleaved, u8 [n][vh][vw][window_bpp], A = 255;
//           a lane then owns its four pixels in all three channels and stores them at once, guided or not.  out is never nullptr
//           under a packed format: what is written in place is planar.
// npe_ops.hires_render[_guided] of n windows: views = device int[n][3] (session, x, y), every window vw x vh with x and vw multiples
// of 4.  out u8 [n][3][vh][vw]; out == nullptr: the whole picture (vw = vh = S, x = y = 0) written over the session's own SRC row
constexpr int SESSION_GUIDE_TABLE_LEN = 3 * 255 + 1;
constexpr int PIXELS_PLANAR = 0, PIXELS_RGB = 1, PIXELS_RGBA = 2, PIXELS_BGRA = 3;
constexpr int pixels_bpp(int format) { return format == PIXELS_RGBA || format == PIXELS_BGRA ? 4 : 3; }   // bytes a pixel of out, planar: over its planes
hipError_t launch_session_render(const SessionPool& P, const float* table, const int* views, int vw, int vh, int zoom, unsigned char* out, int n,
                                 int format, hipStream_t s);
// canvases (ian_sessions_reserve_canvas): whole photos in device memory and, per canvas, the table of the sessions
// placed on it.  Beside the pool for SessionRings' reason; only the canvas kernels take it.  All nullptr / 0 without the reservation.
constexpr int CANVAS_MAX_PLACED = 8;
struct SessionCanvases {
  unsigned char* pix;     // u8 [count][3][max_h][max_w]: row stride max_w whatever a picture's own width (size_t offsets throughout)
  int* table;             // int[count][CANVAS_MAX_PLACED][4]: (session, x, y, scale) in ascending session id, session -1 ends the list
  int count, max_w, max_h;
  int feather;            // 0..16, in field pixels
};
// what every canvas launcher checks of it
inline bool canvases_ok(const SessionCanvases& C) {
  return C.pix && C.table && C.count >= 1 && C.max_w >= 64 && C.max_h >= 64 && (C.max_w & 3) == 0 && C.feather >= 0 && C.feather <= 16 &&
         (reinterpret_cast<uintptr_t>(C.pix) & 3) == 0;
}
// place: items = device int[n][5] (ian_canvas_placement: session, canvas, x, y, scale).  The exact box mean of the canvas's square ->
// GIM, IM of the session and x[i] = table[byte]: the outputs of launch_session_hires_open, without an SRC copy, the square at any
// byte alignment, the scale per item.
hipError_t launch_canvas_place(const SessionCanvases& C, const SessionPool& P, const int* items, const float* table, float* x, int n,
                               hipStream_t s);
// npe_ops.canvas_compose[_guided] of n windows: windows = device int[n][3] (canvas, x, y), every window vw x vh with x and vw multiples
// of 4; table, zoom and format as for launch_session_render.  out u8 [n][3][vh][vw], 4-byte aligned; out == nullptr: n == 1 and the window is
// a whole picture (x = y = 0), written over the canvas itself
hipError_t launch_canvas_compose(const SessionCanvases& C, const SessionPool& P, const float* table, const int* windows, int vw, int vh, int zoom,
                                 unsigned char* out, int n, int format, hipStream_t s);
// oriented placements (ian_place_oriented).  The canvases' second table, device int[count][CANVAS_MAX_PLACED][8]:
// (session, cx2, cy2, ax, ay, bx, by, m) in ascending session id, session -1 ends the list.  It is not a member of SessionCanvases,
// so the kernels above keep their arguments.
// place: items = device int[n][6] (ian_canvas_oriented: session, canvas, cx2, cy2, ax, ay), every sample on the picture (the host
// has checked).  npe_ops.canvas_crop_mean_oriented -> what launch_canvas_place writes.
hipError_t launch_canvas_place_oriented(const SessionCanvases& C, const SessionPool& P, const int* items, const float* table, float* x, int n,
                                        hipStream_t s);
// npe_ops.canvas_compose_oriented[_zoom] of n windows of canvases that hold oriented placements; windows, zoom and out as for
// launch_canvas_compose, no guided form
hipError_t launch_canvas_compose_oriented(const SessionCanvases& C, const int* otable, const SessionPool& P, const int* windows, int vw, int vh,
                                          int zoom, unsigned char* out, int n, int format, hipStream_t s);

// identity-edge gradient hand-over: gd[p,c] (+)= gs[p,coff+c] * act'(y[p,c]) * scale[c]   (NHWC, strides ss / ds)
hipError_t launch_grad_pass(const float* gs, int ss, int coff, float* gd, const float* y, int ds, const float* scale,
                            long long npix, int C, int act, int accumulate, hipStream_t s);
// backward of beta_layer x3 + concat
struct BetaBwdArgs {
  const float* v[3];      // forward values of the three 2-channel maps (after their sigmoid)
  float* g[3];            // gradient buffers of the same maps (pre-epilogue of their producers)
  const float* scale[3];  // producer scale vectors (or nullptr)
  int act[3];             // producer activations
  int accumulate[3];
};
hipError_t launch_beta_bwd(const float* gout, const BetaBwdArgs& a, int n, int hw, int rs, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// training step (train_IAN.py:47-352): backward-weight tap GEMM, parameter (re)packing, elementwise / reductions
// ---------------------------------------------------------------------------------------------
struct WgItem {  // one workgroup of tapwgrad: a (tap, Cout tile, Cin tile, pixel range) -> one partial-slab tile
  int cls, tap;  // class index, GLOBAL tap index (== slab index of the forward packing)
  int co0, ci0;
  int m0, m1;    // contraction range over (image, qy, qx), multiples of 32 except the tail
  int split;     // which partial slab
  int pad;
};
struct WgParams {
  const float* x;   // layer input, NHWC, pixel stride Cin
  const float* dy;  // gradient wrt the layer's (pre-epilogue) output, NHWC, pixel stride dy_stride
  float* partial;   // [nsplit][ntaps][CoutPad][CinPad]
  const WgItem* items;
  const TgClass* classes;
  const TgTap* taps;
  int M, IH, IW, Cin, qw_shift, qhw_shift, si, by, bx, so, OH, OW;
  int dy_stride, CoutPad, CinPad;
  long long slab_total;
  unsigned x_bytes, dy_bytes;
};
enum WgConfig { WG_128x128 = 0, WG_32x128 = 1, WG_128x32 = 2, WG_128x128W8 = 3 /* 8 waves of 64x32 */, WG_128x128P = 4 /* the same tile, software-pipelined K loop */, WG_128x128P2 = 5 /* ... rotated, three fragment buffers */,
                WG_128x128P3 = 6 /* ... P with the loads of two K-steps in flight */ };
hipError_t launch_tapwgrad(int cfg, const WgParams& p, int nitems, hipStream_t s);
hipError_t launch_wgrad_reduce(const float* partial, long long slab_total, int nsplit, const int* inv, float* out,
                               long long count, int accumulate, hipStream_t s);
// the slab -> reference map of a layer when it is affine (kernels_wgrad.hip wgrad_reduce_tiled_kernel); valid == false keeps the gather
struct WgReduceTiledDesc {
  bool valid = false;
  int ntaps = 0, CoutPad = 0, CinPad = 0, Cout = 0, Cin = 0, tco = 16, tci = 16, s_co = 0, s_ci = 0;
  bool ci_inner = true;                       // which axis walks the reference contiguously (stride = ntaps)
  const int* co_off = nullptr;                // device tables replacing co * s_co / ci * s_ci where a permutation makes that axis non-linear
  const int* ci_off = nullptr;
  unsigned char tap_off[48] = {0}, tap_inv[48] = {0};
};
hipError_t launch_wgrad_reduce_tiled(const WgReduceTiledDesc& d, const float* partial, long long slab_total, int nsplit, float* out,
                                     int accumulate, hipStream_t s);
hipError_t launch_pack_tiled(const WgReduceTiledDesc& d, const float* ref, float* slab, hipStream_t s);
hipError_t launch_gather_pack(const float* src, const int* map, float* dst, long long count, hipStream_t s);

constexpr int MDC_MAX_BRANCH = 5;  // base 3x3 + up to IAN_MAX_SCALES dilated branches
struct MdcPackArgs {
  const float* W;                      // (Cout,Cin,3,3) reference layout
  const float* coeff[MDC_MAX_BRANCH];  // per-filter coefficients of the 3x3 branches: [0] = base, then dilations in order
  const float* coeff_1x1;              // or nullptr
  float* slab_f;                       // [ntaps][f_rows][f_cols]
  float* slab_b;                       // [ntaps][b_rows][b_cols] (transposed)
  int ntaps, cout, cin, nbranch, f_rows, f_cols, b_rows, b_cols;
  int tap_start[48];                   // entries of tap t: [tap_start[t], tap_start[t+1])
  unsigned char ent_branch[48], ent_pq[48];
};
struct MdcCoeffGrads {
  float* d[MDC_MAX_BRANCH];
  float* d1x1;
};
hipError_t launch_mdc_pack(const MdcPackArgs& a, hipStream_t s);
hipError_t launch_mdc_unpack_grad(const MdcPackArgs& a, const float* dS, float* dW, const MdcCoeffGrads& g,
                                  int accumulate, hipStream_t s);

struct ColStatsArgs {
  const float* x;  // mode 0: the tensor; modes 1,2: dA
  const float* a;  // post-activation output (for act'), modes 1,2
  const float* y;  // raw (pre-batch-norm) value, mode 1
  const float* mean;
  const float* inv_std;
  double* partial; // [nchunks][2][C] float64 partial sums (kernels_train.hip: NUMERICS)
  long long rows;
  int C, stride, mode, act;
};
hipError_t launch_colstats(const ColStatsArgs& a, int nchunks, double* sums, hipStream_t s);
// single-process batch-norm statistics, second stage fused (kernels_train.hip: bn_finish_kernel / bn_bwd_finish_kernel)
hipError_t launch_bn_stats_affine(const ColStatsArgs& a, int nchunks, double* sums, float count, float eps, const float* gamma,
                                  const float* beta, float* mean, float* inv_std, float* scale, float* shift, float* run_mean,
                                  float* run_inv_std, float keep, float alpha, hipStream_t s);
hipError_t launch_bn_bwd_stats(const ColStatsArgs& a, int nchunks, double* sums, float* gbeta, int acc_beta, float* ggamma,
                               int acc_gamma, hipStream_t s);
// the second stages alone (partials already in place: GEMM-epilogue statistics, TgStats)
hipError_t launch_bn_finish(const double* partial, int nchunks, int C, double* sums, float count, float eps, const float* gamma,
                            const float* beta, float* mean, float* inv_std, float* scale, float* shift, float* run_mean,
                            float* run_inv_std, float keep, float alpha, hipStream_t s);
hipError_t launch_bn_bwd_finish(const double* partial, int nchunks, int C, double* sums, float* gbeta, int acc_beta, float* ggamma,
                                int acc_gamma, hipStream_t s);
// out[i] = pairwise tree over k < count of partial[k*width + i] (fixed order: see kernels_train.hip)
hipError_t launch_tree_sum(const double* partial, int count, int width, double* out, hipStream_t s);
hipError_t launch_bn_make_affine(const double* sums, float count, float eps, const float* gamma, const float* beta,
                                 int C, float* mean, float* inv_std, float* scale, float* shift, hipStream_t s);
hipError_t launch_bn_running(float* run_mean, const float* mean, float* run_inv_std, const float* inv_std, int C, float keep,
                             float alpha, hipStream_t s);
struct BnBwdArgs {
  const float* dA;
  const float* a;
  const float* y;
  const float* mean;
  const float* inv_std;
  const float* scale;
  const double* sums; // [2][C] float64 (sum g, sum g*xhat) or nullptr: activation backward only
  float* dy;
  long long rows;
  int C, stride, act;
  float count;
};
hipError_t launch_bn_bwd_apply(const BnBwdArgs& a, hipStream_t s);
hipError_t launch_axpy(float alpha, const float* x, float* y, long long n, int accumulate, hipStream_t s);
hipError_t launch_axpy_f64(double alpha, const double* x, float* y, long long n, int accumulate, hipStream_t s);
hipError_t launch_nchw_to_nhwc(const float* src, float* dst, int n, int hw, int c, int stride, hipStream_t s);
hipError_t launch_globalpool(const float* x, float* y, int n, int hw, int C, int xs, int ys, hipStream_t s);
hipError_t launch_globalpool_bwd(const float* dy, float* dx, int n, int hw, int C, int xs, int ys, int accumulate,
                                 hipStream_t s);
hipError_t launch_mb_weight(const float* theta, const float* lws, float* W, float* colscale, int nin, int ncol, hipStream_t s);
hipError_t launch_mb_weight_bwd(const float* theta, const float* colscale, const float* dW, float* dtheta, float* dlws,
                                int nin, int ncol, int accumulate, hipStream_t s);
hipError_t launch_mb_forward(const float* act_all, int nall, int as, int row0, int n, int nk, int nd, const float* bias,
                             const float* feat, int fs, int fin, float* mb, int ms, hipStream_t s);
hipError_t launch_mb_backward(const float* act_all, int nall, int as, int row0, int n, int nk, int nd, const float* df_all,
                              int dfs, float* dact, int das, hipStream_t s);
struct DiscHeadArgs {
  float* p;       // [n][3]
  float* loss;    // [n][4]: -log p[target0], -log p[target1], argmax==acc_target, 0
  int target[2];  // -1 = unused
  int acc_target;
};
hipError_t launch_disc_head(const float* mb, int ms, int nfeat, const float* Wd, int ncls, int n, const DiscHeadArgs& a,
                            hipStream_t s);
hipError_t launch_disc_head_bwd(const float* p, const float* Wd, int ncls, int nfeat, int n, int t0, float w0, int t1,
                                float w1, float* dlogits, float* dmb, int ms, hipStream_t s);
hipError_t launch_disc_head_wgrad(const float* mb, int ms, int nfeat, int n, const float* dlogits, int ncls, float* dWd,
                                  int accumulate, hipStream_t s);
hipError_t launch_sample(const float* mu, const float* ls, const float* eps, float* z0, float* klterm, int n, int d,
                         int stride, int es, hipStream_t s);
hipError_t launch_sample_bwd(const float* mu, const float* ls, const float* eps, const float* dz0, float* dmu, float* dls,
                             int n, int d, int stride, int es, float klw, hipStream_t s);
hipError_t launch_made_iaf_bwd(const float* z0, const float* dz, float* dz0, const float* wts, const float* bias, int n,
                               int d, int zs, hipStream_t s);
hipError_t launch_pair_loss(const float* a, const float* b, float* da, long long rows, int C, int stride, int mode,
                            float w, int accumulate, float* partial, int nblocks, float scale, float* out, hipStream_t s);
hipError_t launch_sum_rows(const float* x, int n, int width, float scale, float* out, hipStream_t s);
hipError_t launch_ortho(const float* W, float* dW, int A, int B, int K, float c, float* vals, hipStream_t s);
hipError_t launch_adam(float* p, const float* g, float* m, float* v, long long n, float a_t, float b1, float b2, float eps,
                       hipStream_t s);

}  // namespace ian
