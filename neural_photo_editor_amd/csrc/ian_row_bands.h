// ian_row_bands.h -- into how many row bands the image-producing kernels of kernels_head.hip cut one image.  Plain C++ (no HIP): the
// runtime includes it, and tests/row_bands_main.cpp compiles it on its own.
//
// head6_kernel (the RGB-Beta head of the full IAN) and deconv_small_kernel (IAN_simple's dec_out) give one workgroup a band of
// rows of one image.  A batch that fills the chip alone keeps whole images (no halo row is computed twice); a smaller one is
// halved until `wgs` workgroups exist: 1, 2, 4 or 8 bands.
#pragma once

namespace ian {

//   n         images of the launch
//   wgs       stop splitting once n * bands reaches this many workgroups (options head_wgs / dec_out_wgs)
//   H         rows of the map the kernel walks (its INPUT rows)
//   gran      a band is a whole number of `gran`-row steps, and so is half of it: H % (2 * bands * gran) == 0 before every
//             doubling.  1 for the head (it walks single rows), 2 for dec_out (it walks row pairs)
//   min_rows  ... and half of it keeps at least this many rows: 2 * halo for the head (a band re-reads `halo` rows per side), 0 for
//             dec_out (one halo row per side whatever the band)
// Every result divides H, and with gran = 2 every band is a whole number of row pairs (H % (2 * bands) == 0), as long as H itself is
// a multiple of gran.
inline int row_bands(int n, int wgs, int H, int gran, int min_rows) {
  int bands = 1;
  while ((long long)n * bands < wgs && bands < 8 && (H % (bands * 2 * gran)) == 0 && H / (bands * 2) >= min_rows) bands *= 2;
  return bands;
}

}  // namespace ian
