// ian_tg_types.h -- the host-built tables of the tap GEMM (kernels_tapgemm.hip), as plain data.
// Plain C++: no HIP.  Shared by the device code (through ian_internal.h) and by the planner (ian_tg_plan.h), which
// tests/tg_plan_main.cpp runs on the CPU.
#ifndef IAN_TG_TYPES_H
#define IAN_TG_TYPES_H

namespace ian {

// ---------------------------------------------------------------------------------------------
// "tap GEMM": every dense-channel layer of the IAN (5x5/s2 conv, 5x5/s2 transposed conv split into
// its 4 output-parity classes, composite multiscale-dilated 3x3, dense) is one implicit GEMM
//     C[m][co] = sum_t sum_ci  X[pixel(m) + d_t][ci] * Wt[t][co][ci]
// over a list of taps t = (dy,dx, weight slab).  m enumerates the rows (image, qy, qx) of a per-class output
// grid; input pixel = q*si + b + d_t, output pixel = q*so + p_class.
// Row order (tg_row, kernels_tapgemm.hip):
//   image-major     m = (n * QH + qy) * QW + qx                          M = images * QH * QW
//   position-major  m = pos * Bp + n, pos = qy * QW + qx, Bp = 1 << b_shift >= images (rows with n >= images are padding)
//                   M = QH * QW * Bp.  A tile then covers few positions x many images, so the taps that fall outside the image
//                   for ALL its rows can be left out of its tap list (ian_tg_plan.h).  Only the rows are re-ordered: the
//                   tensors keep their NHWC layout.
// ---------------------------------------------------------------------------------------------
struct TgTap {
  int dy, dx;
};
// an entry of a schedule's tap table (tapgemm_kernel): a tile's list names the class's taps it keeps, in class order, each with the
// index of its weight slab in the class.  A full list has slab == position in the list.
struct TgTapE {
  int dy, dx;
  int slab;
  int pad;
};
struct TgClass {
  int ntaps, tap0;  // taps[tap0 .. tap0+ntaps)
  int py, px;       // output parity offset
  long long w_off;  // float offset of this class's first weight slab; slab t at w_off + t*CoutPad*Cin
};
struct TgItem {  // one workgroup's job (host-built table, 64 B = one s_load_dwordx16)
  int cls, m0, n0;
  int ks0, ks1;  // K-step range [ks0,ks1) of 32-channel steps over (tap of the tile's list, ci-chunk)
  int slab;      // split-K: slab tile index; -1 = direct epilogue
  int tile;      // split-K: index of the output tile in the TgTile table (fused combine: counter + slab range)
  // the item's class and the tap its K range starts in, COPIED here (tg_plan, ian_tg_plan.h) so that the kernel's
  // prologue is one table fetch instead of three dependent ones (item -> class -> tap: ~0.5-1 us each from a cold L2, before the
  // first operand load can be addressed).  ntaps / tap0 are the TILE's tap list in the schedule's TgTapE table (tapgemm_kernel); the
  // split-bf16 kernel reads the class table and the layer's TgTap list instead.
  int ntaps, tap0, py, px;
  int dy0, dx0;  // ttaps[tap0 + ks0 / (Cin / 32)] ...
  int slab0;     // ... and its weight slab
  long long w_off;
};
static_assert(sizeof(TgItem) == 64, "TgItem is fetched as one 64-byte scalar load");
struct TgTile {  // reduce pass: one output tile
  int cls, m0, n0, slab0, nsplit;
  int py, px;  // the class's output parity offset, copied here so that the reduce pass needs ONE table load, not two dependent ones
  int pad2;
};

}  // namespace ian

#endif
