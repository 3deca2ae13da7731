// Window kernels of the edit sessions: what a call displays of a full-resolution picture or of a canvas.
//   session_render_kernel<GUIDED, PACKED>       a window of a session's picture: SRC + 127.5 * FIELD sampled at full size (4.3; guided 4.11)
//   canvas_compose_kernel<GUIDED, PACKED>       a window of a whole photo: the canvas plus every placed session's feathered field (4.7; 4.13)
//   session_render_zoom_kernel<GUIDED, PACKED>, canvas_compose_zoom_kernel<GUIDED, PACKED>   the same windows at 1/k, never written at 1:1 (4.14)
//   canvas_compose_oriented_kernel<PACKED>, canvas_compose_oriented_zoom_kernel<PACKED>      a canvas whose placements have any size and tilt
//                                       (4.16): ComposeOrientedPx4 in the same loops and sinks, the taps read from global memory, no staging
// PACKED: the window is written as interleaved rgb, rgba or bgra pixels (ian_sessions_set_pixels, 4.17; npe_ops.pack_window).
// GUIDED: the field's four taps weighted by the photo (ian_sessions_reserve_guide / _edges).  Every result byte is specified by
// npe_ops.py (hires_render[_guided], canvas_compose[_guided], zoom_box_mean) and matched bit for bit.  Three layers, each written once:
//   staging  the field rows a band of output rows taps (and, guided, the same rows of GIM and the range weights) -> LDS
//   px4      the result bytes of one aligned uchar4 of the source: RenderPx4 (a session), ComposePx4 (a canvas)
//   sink     where a lane's bytes go: a uchar4 store (StoreRows, 1:1) or integer sums in LDS (ZoomSums, 1/k); packed pixels (4.17):
//            one 12- or 16-byte store of a lane's four interleaved pixels (PackedRows, zoom_store_packed)
// A kernel is stage, loop (px_rows / px_columns), px4, sink.
#include <cstdint>

#include "ian_internal.h"
#include "ian_oriented.h"   // oriented_bbox, shared with the host
#include "npe_blend.h"  // floating-point contraction off from here on: every expression below depends on it

namespace ian {

// ---- the arithmetic of one tap (npe_ops.hires_axis_taps / hires_render / hires_guide_field) -------------------------------------------
// The photo lives in the pool at S x S, S = 64 * scale; what a call displays is kept as FIELD / FIELD_KIND, and a window of the picture
// at full size is SRC + 127.5 * sample(FIELD) (kind 0: the unedited part of the photo stays pixel-exact) or 127.5 * (bilinear(FIELD) + 1)
// (kind 1: FIELD holds x, a sample has no photo under it).

// hires_axis_taps for one output coordinate: half-pixel centres in integers, a = 2Y + 1 - s in (-2s, 128s), i0 = floor(a / 2s) >= -1,
// t = float32(a - 2s * i0) / float32(2s) (one division), both taps clamped to 0..63
__device__ __forceinline__ void hires_taps(int Y, int s, int& lo, int& hi, float& t) {
  const int s2 = 2 * s, a = 2 * Y + 1 - s;
  const int i0 = (a + s2) / s2 - 1;   // a + 2s > 0: truncation is the floor
  t = (float)(a - s2 * i0) / (float)s2;
  lo = min(max(i0, 0), 63);
  hi = min(max(i0 + 1, 0), 63);
}

// the field at square coordinate u of the output row whose two tapped field rows are top and bot (weight ty): hires_render's bilinear
// tap, float32, in exactly this order of operations
__device__ __forceinline__ float field_bilinear(const float* top, const float* bot, int s, int u, float ty) {
  int c0, c1;
  float tx;
  hires_taps(u, s, c0, c1, tx);
  const float a0 = top[c0], a1 = bot[c0];
  const float t = a0 + tx * (top[c1] - a0);
  const float b = a1 + tx * (bot[c1] - a1);
  return t + ty * (b - t);
}
// np.clip(np.rint(q), 0, 255).astype(uint8)
__device__ __forceinline__ unsigned char round_u8(float q) { return (unsigned char)fminf(fmaxf(rintf(q), 0.0f), 255.0f); }

// ---- staging ---------------------------------------------------------------------------------------------------------------------
// Band heights.  Plain: the traffic is 2 bytes per output byte plus the staged rows, so the band only has to keep the staging small
// against 8 * vw bytes of output and the grid large; 8 rows give 384 workgroups (1.5 per CU) for ONE whole 1024 x 1024 picture and
// 2 uchar4 per lane at a 256-wide window.  Guided: the range weights need all three channels of a pixel and are computed once per
// pixel, so the channel planes leave the grid and a lane owns its 4 pixels in ALL THREE channels; ONE whole 1024 x 1024 picture is
// then 128 workgroups at 8 rows and 256 at 4, against 256 CUs.  Both were measured in one run on an MI355X: that
// picture takes 16.1 us at 4 rows and 24.7 us at 8 (the bilinear kernel: 15.7), sixteen of them 86.6 against 89.5 us, a 256 x 256
// window 9.3 against 12.4 us.  For a canvas, 8 placements x 3 channels x (band + 2) rows of 256 B field and 64 B GIM are 45 KB at 4
// rows and 75 KB at 8, plus the 3 KB table: only the 4-row band fits the 64 KB of static LDS.  So 4 rows, guided, in both families.
constexpr int RENDER_BAND = 8, GUIDE_BAND = 4;
static_assert(GUIDE_BAND >= 1 && GUIDE_BAND <= RENDER_BAND, "field_rows stages at most RENDER_BAND + 2 rows");

// The field rows that output rows u0..u1 (square coordinates, both inclusive) of a picture at scale s tap: n <= ceil((band - 1) / s)
// + 2 <= band + 2 consecutive rows of 64 floats, from row fr0.  field_rows says which (a session: every lane; a canvas: one lane per
// kept placement, into LDS).
struct FieldRows {
  int fr0, n;
};
__device__ __forceinline__ FieldRows field_rows(int u0, int u1, int s) {
  int fr0, fr1, unused;
  float tunused;
  hires_taps(u0, s, fr0, unused, tunused);
  hires_taps(u1, s, unused, fr1, tunused);
  return FieldRows{fr0, min(fr1 - fr0 + 1, RENDER_BAND + 2)};
}
// rows r of a field plane -> f, all 256 lanes; the caller's barrier publishes f
__device__ __forceinline__ void stage_field_rows(float* f, const float* plane, const FieldRows r) {
  const float* frow = plane + r.fr0 * 64;
  for (int j = threadIdx.x; j < r.n * 64; j += 256) f[j] = frow[j];
}
// the same rows of a session's GIM, as bytes, beside its staged field rows: all 256 lanes, 16 words a row
__device__ __forceinline__ void stage_gim_rows(unsigned char* g, const unsigned char* plane, const FieldRows r) {
  const unsigned* grow = reinterpret_cast<const unsigned*>(plane + r.fr0 * 64);
  unsigned* gl = reinterpret_cast<unsigned*>(g);
  for (int j = threadIdx.x; j < r.n * 16; j += 256) gl[j] = grow[j];
}

// What one session contributes to a band, in LDS: its field rows in the NCH channels a lane owns and, guided, the same rows of GIM.
// A lane owns one channel (plain, planar out: the channel planes are in the grid) or all three (guided; or packed out, DESIGN.md
// 4.17: an interleaved pixel needs its three bytes in one lane).  Three channels take the 4-row band whatever asks for them, for the
// guided kernels' reason: 6 rows of 3 channels are 4.6 KB field (and, guided, 1.1 KB GIM).
template <bool GUIDED, int NCH>
struct StagedRows;
template <int NCH>
struct StagedRows<false, NCH> {
  static constexpr int NC = NCH, BAND = NCH == 3 ? GUIDE_BAND : RENDER_BAND;
  float f[NC][(BAND + 2) * 64];
};
template <>
struct StagedRows<true, 3> {
  static constexpr int NC = 3, BAND = GUIDE_BAND;
  float f[NC][(BAND + 2) * 64];
  alignas(4) unsigned char g[NC][(BAND + 2) * 64];
};
// the channels a lane owns in a kernel: one only where nothing asks for all three
constexpr int window_nc(bool guided, bool packed) { return guided || packed ? 3 : 1; }
// rows fr of session id, channels c0 .. c0 + NC - 1 -> r.  A band of BAND output rows taps at most BAND + 2 field rows; the cap keeps
// whatever a caller computed inside r (a guided compose's 4 output rows tap at most 5 field rows, field_rows itself caps at 10).
template <bool GUIDED, int NC>
__device__ __forceinline__ void stage_rows(StagedRows<GUIDED, NC>& r, const SessionPool& P, int id, int c0, FieldRows fr) {
  fr.n = min(fr.n, StagedRows<GUIDED, NC>::BAND + 2);
  for (int c = 0; c < NC; ++c) {
    const size_t plane = ((size_t)id * 3 + c0 + c) * (64 * 64);
    stage_field_rows(r.f[c], P.field + plane, fr);
    if constexpr (GUIDED) stage_gim_rows(r.g[c], P.gim + plane, fr);
  }
}
// the 766 range weights, computed on the host (no exp here) -> LDS, 3 KB
__device__ __forceinline__ void stage_guide_table(float* tab, const float* __restrict__ table) {
  for (int j = threadIdx.x; j < SESSION_GUIDE_TABLE_LEN; j += 256) tab[j] = table[j];
}

// ---- px4: a session ------------------------------------------------------------------------------------------------------------------
// hires_guide_field's v of the three channels at square coordinate u of the output row whose two tapped rows start at o0 and o1 of the
// staged rows (weight ty): the four bilinear taps of the field weighted by how close the photo's pixel p[0..2] is to each tap's pixel
// of GIM; tab the range weights.  float32 in hires_render_guided's order, and the division is IEEE.
__device__ __forceinline__ void guide_sample(const StagedRows<true, 3>& r, const float* tab, int o0, int o1, int s, int u, float ty, const int p[3],
                                             float v[3]) {
  int c0, c1;
  float tx;
  hires_taps(u, s, c0, c1, tx);
  const float wy0 = 1.0f - ty, wx0 = 1.0f - tx;
  const int at[4] = {o0 + c0, o0 + c1, o1 + c0, o1 + c1};
  const float sw[4] = {wy0 * wx0, wy0 * tx, ty * wx0, ty * tx};
  float w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = abs(p[0] - (int)r.g[0][at[k]]) + abs(p[1] - (int)r.g[1][at[k]]) + abs(p[2] - (int)r.g[2][at[k]]);
    w[k] = sw[k] * tab[d];
  }
  const float den = ((w[0] + w[1]) + w[2]) + w[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float num = ((w[0] * r.f[c][at[0]] + w[1] * r.f[c][at[1]]) + w[2] * r.f[c][at[2]]) + w[3] * r.f[c][at[3]];
    v[c] = num / den;
  }
}
// the field of a lane's NC channels at that place: the guided tap where the guide is on and a photo lies under the field (PHOTO:
// kind 0), the bilinear tap otherwise (a kind 1 field is a sample: there is no photo to guide by)
template <bool GUIDED, bool PHOTO, int NC>
__device__ __forceinline__ void field_sample(const StagedRows<GUIDED, NC>& r, const float* tab, int o0, int o1, int s, int u, float ty, const int* p,
                                             float* v) {
  if constexpr (GUIDED && PHOTO) {
    guide_sample(r, tab, o0, o1, s, u, ty, p, v);
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = field_bilinear(r.f[c] + o0, r.f[c] + o1, s, u, ty);
  }
}
__device__ __forceinline__ void unpack4(const uchar4 v, int b[4]) {
  b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
}

// The result bytes of the aligned uchar4 at (X, Y) of a session's picture, in the lane's NC channels: hires_render[_guided].  rows
// holds the field rows from fr0 on; src is channel c0's plane of the session's SRC.  All arithmetic is float32 in hires_render's order.
template <bool GUIDED, int NCH>
struct RenderPx4 {
  static constexpr int NC = NCH;
  const StagedRows<GUIDED, NC>& rows;
  const float* tab;
  const unsigned char* src;
  size_t plane;
  int S, s, kind, fr0;
  // a sample has no photo under it: nothing is read
  __device__ __forceinline__ void load(int X, int Y, uchar4 pv[NC]) const {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      pv[c] = kind == 0 ? *reinterpret_cast<const uchar4*>(src + c * plane + (size_t)Y * S + X) : make_uchar4(0, 0, 0, 0);
  }
  __device__ __forceinline__ void operator()(int X, int Y, const uchar4 pv[NC], unsigned char ob[NC][4]) const {
    int r0, r1, pb[NC][4];
    float ty;
    hires_taps(Y, s, r0, r1, ty);
    const int o0 = (r0 - fr0) * 64, o1 = (r1 - fr0) * 64;
#pragma unroll
    for (int c = 0; c < NC; ++c) unpack4(pv[c], pb[c]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // The kind is uniform over the workgroup.  Guided, the kinds take different taps: ONE branch per pixel around everything that
      // depends on the kind (a test at the tap and another at the result cost the guided kernels up to 10 %).
      // Plain, they share the tap and a select at the result suffices.
      if constexpr (!GUIDED) px1<-1>(o0, o1, ty, X, e, pb, ob);
      else if (kind == 0) px1<0>(o0, o1, ty, X, e, pb, ob);
      else px1<1>(o0, o1, ty, X, e, pb, ob);
    }
  }
  // pixel e of the uchar4; KIND: the field's kind, -1: this->kind, at run time
  template <int KIND>
  __device__ __forceinline__ void px1(int o0, int o1, float ty, int X, int e, const int pb[NC][4], unsigned char ob[NC][4]) const {
    const int kd = KIND < 0 ? kind : KIND;
    int p[NC];
    float v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = pb[c][e];
    field_sample<GUIDED, KIND == 0, NC>(rows, tab, o0, o1, s, X + e, ty, p, v);
#pragma unroll
    for (int c = 0; c < NC; ++c) ob[c][e] = round_u8(kd == 0 ? (float)p[c] + 127.5f * v[c] : 127.5f * (v[c] + 1.0f));
  }
};

// ---- px4: a canvas (npe_ops.canvas_ramp / canvas_compose[_guided]) ------------------------------------------------------
// A canvas is a whole photo of w x hgt pixels in rows of C.max_w bytes; a session is placed on it as a square of 64 * s pixels at
// (ox, oy), s per placement.

// canvas_ramp for one square coordinate u: f2s = 2 * feather * s (0: no feather)
__device__ __forceinline__ float canvas_ramp1(int u, int S, int f2s) {
  if (f2s == 0) return 1.0f;
  const int d = min(u, S - 1 - u);
  return fminf(1.0f, (float)(2 * d + 1) / (float)f2s);
}
struct CanvasKept {
  int id, ox, oy, s, kind;
};
// What a band of a canvas needs, in LDS: the placements whose squares meet it, which field rows each taps, and those rows
// (StagedRows per kept placement: 20 KB plain, 45 KB guided, 36 KB plain with three channels a lane).
template <bool GUIDED, int NC>
struct CanvasStage {
  StagedRows<GUIDED, NC> rows[CANVAS_MAX_PLACED];
  CanvasKept kept[CANVAS_MAX_PLACED];
  FieldRows frows[CANVAS_MAX_PLACED];   // the staged field rows of each kept placement
  int nkept;
};
// The result bytes of the aligned uchar4 at (X, Y) of a canvas, in the lane's NC channels: acc starts from the canvas bytes and walks
// the kept placements in the table's order, so it lives in registers.  A square starts at any ox while a lane's 4 pixels are aligned
// to the window, so the inside-the-square test is per pixel.  Guided, the sample of a kind 0 placement is guide_sample's, the photo's
// pixel being the STORED canvas byte.  All arithmetic is float32 in canvas_compose's order.  src is channel c0's plane of the canvas.
template <bool GUIDED, int NCH>
struct ComposePx4 {
  static constexpr int NC = NCH;
  const CanvasStage<GUIDED, NC>& st;
  const float* tab;
  const unsigned char* src;
  size_t plane;
  int stride, feather, nk;
  __device__ __forceinline__ void load(int X, int Y, uchar4 pv[NC]) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) pv[c] = *reinterpret_cast<const uchar4*>(src + c * plane + (size_t)Y * stride + X);
  }
  __device__ __forceinline__ void operator()(int X, int Y, const uchar4 pv[NC], unsigned char ob[NC][4]) const {
    int pb[NC][4];
    float acc[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      unpack4(pv[c], pb[c]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[c][e] = (float)pb[c][e];
    }
    for (int k = 0; k < nk; ++k) {
      const CanvasKept q = st.kept[k];
      const int S = 64 * q.s, uy = Y - q.oy;
      if (uy < 0 || uy >= S || X + 3 < q.ox || X > q.ox + S - 1) continue;
      const int f2s = 2 * feather * q.s, fr0 = st.frows[k].fr0;
      int r0, r1;
      float ty;
      hires_taps(uy, q.s, r0, r1, ty);
      const int o0 = (r0 - fr0) * 64, o1 = (r1 - fr0) * 64;
      const float wy = canvas_ramp1(uy, S, f2s);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ux = X + e - q.ox;
        if (ux < 0 || ux >= S) continue;
        const float w = wy * canvas_ramp1(ux, S, f2s);
        if (q.kind == 0) place1<true>(st.rows[k], o0, o1, ty, q.s, ux, w, e, pb, acc);   // uniform over the workgroup: ONE branch per pixel
        else place1<false>(st.rows[k], o0, o1, ty, q.s, ux, w, e, pb, acc);
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[c][e] = round_u8(acc[c][e]);
  }
  // one placement's field at column ux of its square (weight w) onto pixel e of acc: a photo's edit is added, a sample is blended in
  template <bool PHOTO>
  __device__ __forceinline__ void place1(const StagedRows<GUIDED, NC>& r, int o0, int o1, float ty, int s, int ux, float w, int e,
                                         const int pb[NC][4], float acc[NC][4]) const {
    int p[NC];
    float v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = pb[c][e];
    field_sample<GUIDED, PHOTO, NC>(r, tab, o0, o1, s, ux, ty, p, v);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (PHOTO) {
        acc[c][e] = acc[c][e] + (127.5f * v[c]) * w;
      } else {
        const float tv = 127.5f * (v[c] + 1.0f);
        acc[c][e] = w == 1.0f ? tv : acc[c][e] + (tv - acc[c][e]) * w;
      }
    }
  }
};

// one lane's walk of canvas cv's placement table: the placements whose squares meet rows Y0..Y1 (both inclusive) of a window at columns
// vx .. vx + vw - 1 go to kept, in the table's order, each with the field rows those rows tap inside its square -> how many
__device__ __forceinline__ int canvas_keep_band(const SessionCanvases& C, const SessionPool& P, int cv, int vx, int vw, int Y0, int Y1,
                                                CanvasKept* kept, FieldRows* frows) {
  int nk = 0;
  const int* tb = C.table + (size_t)cv * (CANVAS_MAX_PLACED * 4);
  for (int k = 0; k < CANVAS_MAX_PLACED; ++k) {
    const int id = tb[4 * k], ox = tb[4 * k + 1], oy = tb[4 * k + 2], s = tb[4 * k + 3];
    if (id < 0) break;
    const int S = 64 * s;
    if (s < 1 || s > 16 || Y1 < oy || Y0 > oy + S - 1 || vx + vw - 1 < ox || vx > ox + S - 1) continue;
    frows[nk] = field_rows(max(Y0, oy) - oy, min(Y1, oy + S - 1) - oy, s);   // the band's rows inside the square, in its coordinates
    kept[nk++] = CanvasKept{id, ox, oy, s, P.kind[id]};
  }
  return nk;
}
// canvas_keep_band's field rows of one kept placement for rows Y0..Y1 of the canvas (a chunk of the band it was kept for)
__device__ __forceinline__ FieldRows canvas_chunk_rows(const CanvasKept& q, int Y0, int Y1) {
  const int a = max(Y0, q.oy), b = min(Y1, q.oy + 64 * q.s - 1);
  return a <= b ? field_rows(a - q.oy, b - q.oy, q.s) : FieldRows{0, 0};
}
// Lane 0 reads the canvas's placement table once per workgroup (a walk in global memory by one lane; the test is uniform over the
// workgroup) and keeps the placements that meet rows Y0..Y1, columns X0 .. X0 + W - 1; guided, the range weights follow if anything
// is kept -> how many.  Rows that meet no square are a plain copy.
template <bool GUIDED, int NC>
__device__ __forceinline__ int canvas_keep(CanvasStage<GUIDED, NC>& st, float* tab, const SessionCanvases& C, const SessionPool& P,
                                           const float* __restrict__ table, int cv, int X0, int W, int Y0, int Y1) {
  if (threadIdx.x == 0) st.nkept = canvas_keep_band(C, P, cv, X0, W, Y0, Y1, st.kept, st.frows);
  __syncthreads();
  const int nk = st.nkept;
  if constexpr (GUIDED)
    if (nk) stage_guide_table(tab, table);
  return nk;
}
// Each kept placement's rows for rows Y0..Y1 -> LDS; the caller's barrier publishes them.  chunk: Y0..Y1 are a part of the rows the
// placements were kept for, and lane p first says which field rows THIS part taps inside kept placement p (none: n = 0).
template <bool GUIDED, int NC>
__device__ __forceinline__ void canvas_stage(CanvasStage<GUIDED, NC>& st, const SessionPool& P, int nk, int c0, bool chunk, int Y0, int Y1) {
  if (chunk) {
    if (threadIdx.x < nk) st.frows[threadIdx.x] = canvas_chunk_rows(st.kept[threadIdx.x], Y0, Y1);
    __syncthreads();
  }
  for (int p = 0; p < nk; ++p) stage_rows(st.rows[p], P, st.kept[p].id, c0, st.frows[p]);
}

// ---- px4: a canvas of oriented placements (npe_ops.canvas_compose_oriented) -----------------------------------------
// A placement is a similarity transform in integers: centre (cx2, cy2) in half pixels, (bx, by) field pixels per canvas pixel in Q20.
// A pixel's field coordinates are Uq = dx*bx + dy*by (u - 32 in Q21) and Vq = dy*bx - dx*by with dx = 2X+1-cx2, dy = 2Y+1-cy2: up to
// 2^36, so 64 bits until the inside test (-2^26 <= Q < 2^26) has passed, 32 from there.  A band that crosses a tilted square can tap
// any of the 64 field rows, so nothing is staged: the four taps are read from the session's FIELD plane in global memory (16 KB a
// channel, read-only during a compose, shared by every workgroup of the launch: L2 and the vector cache serve them).
struct OrientedKept {
  int id, cx2, cy2, bx, by, kind;
  OrientedBox box;
};
struct OrientedStage {
  OrientedKept kept[CANVAS_MAX_PLACED];
  int nkept;
};
constexpr int ORIENTED_LIM = 1 << 26;
// the taps of one axis at field coordinate Q: a = Q + 2^26 - 2^20 in [-2^20, 2^27), t exact in float32 (21 bits over a power of two)
__device__ __forceinline__ void oriented_taps(int Q, int& lo, int& hi, float& t) {
  const int a = Q + ORIENTED_LIM - (1 << 20), i0 = a >> 21;
  t = (float)(a & ((1 << 21) - 1)) / 2097152.0f;
  lo = min(max(i0, 0), 63);
  hi = min(max(i0 + 1, 0), 63);
}
// the feather along one axis: f16 = feather << 16 (0: none); d <= 2^21 is exact in float32
__device__ __forceinline__ float oriented_ramp1(int Q, int f16) {
  if (f16 == 0) return 1.0f;
  const int d = min(Q + ORIENTED_LIM, ORIENTED_LIM - Q) >> 5;
  return fminf(1.0f, (float)d / (float)f16);
}
// The result bytes of the aligned uchar4 at (X, Y) of a canvas in channel c0: ComposePx4's walk of the kept placements with the
// oriented geometry.  A lane's four pixels advance (Uq, Vq) by (2bx, -2by) from one 64-bit base per row and placement.
template <int NCH>
struct ComposeOrientedPx4 {
  static constexpr int NC = NCH;
  const OrientedStage& st;
  const float* field;   // channel c0's plane of session 0: a session's is 3 * 4096 floats on
  const unsigned char* src;
  size_t plane;
  int stride, feather, nk;
  __device__ __forceinline__ void load(int X, int Y, uchar4 pv[NC]) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) pv[c] = *reinterpret_cast<const uchar4*>(src + c * plane + (size_t)Y * stride + X);
  }
  // the geometry (taps, weights, feather) is the pixel's, computed once; the channels differ in the field plane and the accumulator
  __device__ __forceinline__ void operator()(int X, int Y, const uchar4 pv[NC], unsigned char ob[NC][4]) const {
    int pb[4];
    float acc[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      unpack4(pv[c], pb);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[c][e] = (float)pb[e];
    }
    const int f16 = feather << 16;
    for (int k = 0; k < nk; ++k) {
      const OrientedKept q = st.kept[k];
      if (Y < q.box.y0 || Y > q.box.y1 || X + 3 < q.box.x0 || X > q.box.x1) continue;
      const long long dx = 2 * X + 1 - q.cx2, dy = 2 * Y + 1 - q.cy2;
      long long Uq = dx * q.bx + dy * q.by, Vq = dy * q.bx - dx * q.by;
      const float* F = field + (size_t)q.id * (3 * 64 * 64);
#pragma unroll
      for (int e = 0; e < 4; ++e, Uq += 2 * q.bx, Vq -= 2 * q.by) {
        if (Uq < -ORIENTED_LIM || Uq >= ORIENTED_LIM || Vq < -ORIENTED_LIM || Vq >= ORIENTED_LIM) continue;
        const int U = (int)Uq, V = (int)Vq;
        int c0, c1, r0, r1;
        float tx, ty;
        oriented_taps(U, c0, c1, tx);
        oriented_taps(V, r0, r1, ty);
        float v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float* top = F + c * (64 * 64) + r0 * 64;
          const float* bot = F + c * (64 * 64) + r1 * 64;
          const float a0 = top[c0], a1 = bot[c0];
          const float t = a0 + tx * (top[c1] - a0);
          const float b = a1 + tx * (bot[c1] - a1);
          v[c] = t + ty * (b - t);
        }
        const float w = oriented_ramp1(V, f16) * oriented_ramp1(U, f16);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (q.kind == 0) {   // uniform over the workgroup
            acc[c][e] = acc[c][e] + (127.5f * v[c]) * w;
          } else {
            const float tv = 127.5f * (v[c] + 1.0f);
            acc[c][e] = w == 1.0f ? tv : acc[c][e] + (tv - acc[c][e]) * w;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[c][e] = round_u8(acc[c][e]);
  }
};
// Lane 0 walks canvas cv's oriented table (int[8][8]: session, cx2, cy2, ax, ay, bx, by, m; session -1 ends the list) once per
// workgroup and keeps the placements whose bounding boxes meet rows Y0..Y1, columns X0 .. X0 + W - 1, in the table's order -> how many
__device__ __forceinline__ int oriented_keep(OrientedStage& st, const int* __restrict__ otable, const SessionPool& P, int cv, int X0, int W, int Y0,
                                             int Y1) {
  if (threadIdx.x == 0) {
    int nk = 0;
    const int* tb = otable + (size_t)cv * (CANVAS_MAX_PLACED * 8);
    for (int k = 0; k < CANVAS_MAX_PLACED; ++k) {
      const int* t = tb + 8 * k;
      const int id = t[0];
      if (id < 0) break;
      const OrientedBox box = oriented_bbox(t[1], t[2], t[3], t[4]);
      if (Y1 < box.y0 || Y0 > box.y1 || X0 + W - 1 < box.x0 || X0 > box.x1) continue;
      st.kept[nk++] = OrientedKept{id, t[1], t[2], t[5], t[6], P.kind[id], box};
    }
    st.nkept = nk;
  }
  __syncthreads();
  return st.nkept;
}

// ---- sinks and loops -------------------------------------------------------------------------------------------------------------
// 1:1: the bytes of item (ry, cx) of a band go to row row0 + ry, column col0 + cx of plane c.  A window of `out` (u8 [n][3][vh][vw]),
// or, out == nullptr, the whole picture over the source itself (commit): a lane stores exactly the bytes it loaded, after loading
// all of them in every channel it owns, and the fields, GIM and the table live elsewhere, so this is safe in place (overlapping
// squares included); neither pointer is __restrict__.
struct StoreRows {
  unsigned char* base;
  size_t plane;
  int stride, row0, col0;
  template <int NC>
  __device__ __forceinline__ void put(int ry, int cx, const unsigned char (&ob)[NC][4]) const {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      *reinterpret_cast<uchar4*>(base + c * plane + (size_t)(row0 + ry) * stride + col0 + cx) = make_uchar4(ob[c][0], ob[c][1], ob[c][2], ob[c][3]);
  }
};
// Packed pixels (npe_ops.pack_window): a lane's four pixels in all three channels, interleaved, as ONE store of 12
// (rgb) or 16 bytes (rgba, bgra; A = 255) at `at`, which is 4-byte aligned: `out` is, and x, vw and the lane's column are multiples
// of 4 pixels.  Consecutive lanes store consecutive addresses.  The format is uniform over the grid: the byte order is a select.
typedef unsigned Packed12 __attribute__((ext_vector_type(3), aligned(4)));   // vectors at the alignment `out` promises: dwordx3 / dwordx4
typedef unsigned Packed16 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void store_packed4(unsigned char* at, int format, const unsigned char (&ob)[3][4]) {
  if (format == PIXELS_RGB) {
    Packed12 v;
    v[0] = ob[0][0] | ob[1][0] << 8 | ob[2][0] << 16 | (unsigned)ob[0][1] << 24;
    v[1] = ob[1][1] | ob[2][1] << 8 | ob[0][2] << 16 | (unsigned)ob[1][2] << 24;
    v[2] = ob[2][2] | ob[0][3] << 8 | ob[1][3] << 16 | (unsigned)ob[2][3] << 24;
    *reinterpret_cast<Packed12*>(at) = v;
  } else {
    const bool bgr = format == PIXELS_BGRA;
    Packed16 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (bgr ? ob[2][e] : ob[0][e]) | ob[1][e] << 8 | (bgr ? ob[0][e] : ob[2][e]) << 16 | 0xff000000u;
    *reinterpret_cast<Packed16*>(at) = v;
  }
}
// 1:1, packed: the pixels of item (ry, cx) of a band go to row row0 + ry, pixel cx of a window (u8 [vh][vw][bpp]) of `out`
struct PackedRows {
  unsigned char* base;
  int vw, row0, format;
  __device__ __forceinline__ void put(int ry, int cx, const unsigned char (&ob)[3][4]) const {
    store_packed4(base + ((size_t)(row0 + ry) * vw + cx) * pixels_bpp(format), format, ob);
  }
};
// A lane owns 4 consecutive bytes of a row of the source window rows x 4L at (X0, Y0), in Px::NC channels: NC uchar4 loads, px4, one
// put.  Consecutive lanes, consecutive uchar4.
template <typename Px, typename Sink>
__device__ __forceinline__ void px_rows(const Px& px, int X0, int Y0, int rows, int L, const Sink& to) {
  for (int idx = threadIdx.x; idx < rows * L; idx += 256) {
    const int ry = idx / L, cx = (idx - ry * L) * 4;
    uchar4 pv[Px::NC];
    unsigned char ob[Px::NC][4];
    px.load(X0 + cx, Y0 + ry, pv);
    px(X0 + cx, Y0 + ry, pv, ob);
    to.put(ry, cx, ob);
  }
}

// ---- zoomed views (npe_ops.zoom_box_mean over hires_render[_guided] / canvas_compose[_guided]) ----------------------------
// Output pixel (Y, X) of a window at 1/k is (sum of the k x k block of 1:1 result bytes + k*k/2) / (k*k), the block at source
// (vy + k*Y, vx + k*X).  The zoomed kernels are the 1:1 kernels with another sink: the byte that enters a sum comes from the same px4,
// so it IS the byte the 1:1 kernel stores, and integer sums are exact in any order.  No 1:1 byte reaches memory; 3 * vw * vh bytes a
// window are written.
//   Work split.  A workgroup owns a tile of the SOURCE: `orows` = max(1, band / k) output rows, i.e. k * orows source rows, by at
// most `tile` source columns, i.e. ow <= (tile / k) & ~3 output columns (a multiple of 4, so a tile starts on an aligned uchar4 of
// the source and of the output).  blockIdx.x = row group * column tiles + column tile; y, z as in the 1:1 kernel.
//   Staging.  The source rows of the tile are walked in chunks of at most `band` rows, band = the 1:1 kernel's band height, and each
// chunk stages exactly what that kernel stages for a band: 16 source rows at scale 1 tap 18 field rows, which field_rows would
// silently cap at 10.  A canvas keeps its placements once, for the tile (canvas_keep), and each chunk refreshes their rows
// (canvas_stage).  The sums stay in LDS across the chunks.
//   Lanes.  Consecutive lanes load consecutive aligned uchar4 of a source row (box_mean_row's ownership), compute the four result
// bytes, merge those that fall into the same output pixel and do one LDS add per pixel touched (zoom_add4).  The plain kernels sum
// a column of source rows in registers first, as box_mean_row does (px_columns): measured on an MI355X, one 1024 x 1024 picture at
// k = 16 takes 16.1 us so and 24.1 us with one LDS add per source row.  After the last chunk orows * ow / 4 lanes
// divide and store one uchar4 each (zoom_store).
//   Sizes.  Plain: band 8, tile 1024 columns (one lane pass per source row at the widest), sums orows * ow <= 8 * 1024 / 4 ints,
// 8 KB.  Guided (no channel planes in the grid, three channels per lane): band 4, tile 256 columns, so a chunk is one pass of the 256
// lanes (px_rows) and ONE 1024 x 1024 picture at k = 16 is 64 x 4 = 256 workgroups; sums 3 * 4 * 256 / 4 ints, 3 KB.  The shape
// goes with the channels a lane owns, not with the guide: the packed plain kernels take the guided one.
constexpr int ZOOM_MAX = 16;
template <int NC>
struct ZoomShape {
  static constexpr int BAND = NC == 3 ? GUIDE_BAND : RENDER_BAND, TILE = NC == 3 ? 256 : 1024, SUMS = BAND * TILE / 4;   // sums per channel; k >= 2
};
struct ZoomSplit {
  int orows, ow_tile, ntiles;
};
__host__ __device__ inline ZoomSplit zoom_split(int band, int tile, int k, int vw) {
  const int ow_tile = (tile / k) & ~3;
  return ZoomSplit{band / k > 1 ? band / k : 1, ow_tile, (vw + ow_tile - 1) / ow_tile};
}
// this workgroup's tile: output rows oy0 .. oy0 + orows - 1, output columns ox0 .. ox0 + ow - 1 of the window
struct ZoomTileAt {
  int oy0, orows, ox0, ow;
};
__device__ __forceinline__ ZoomTileAt zoom_tile_at(int band, int tile, int k, int vw, int vh) {
  const ZoomSplit z = zoom_split(band, tile, k, vw);
  const int grp = blockIdx.x / z.ntiles, t = blockIdx.x - grp * z.ntiles;
  const int oy0 = grp * z.orows, ox0 = t * z.ow_tile;
  return ZoomTileAt{oy0, min(z.orows, vh - oy0), ox0, min(z.ow_tile, vw - ox0)};
}
// the four result bytes of the aligned uchar4 at source column cx of the tile -> the sums of its output row
template <typename T>
__device__ __forceinline__ void zoom_add4(int* row, int cx, int k, const T ob[4]) {
  int bin = cx / k, r = cx - bin * k, t = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    t += ob[e];
    if (++r == k) {
      atomicAdd(&row[bin], t);
      ++bin;
      r = 0;
      t = 0;
    }
  }
  if (r) atomicAdd(&row[bin], t);   // r bytes (at most 4 of them this lane's) of a pixel that goes on in the next uchar4
}
// 1/k: the bytes of item (ry, cx) of the chunk that starts at source row row0 of the tile go to the sums of output row
// (row0 + ry) / k; sum is [channel][per], a channel's sums [orows][ow]
struct ZoomSums {
  int* sum;
  int per, ow, k, row0;
  template <typename T, int NC>
  __device__ __forceinline__ void put(int ry, int cx, const T (&ob)[NC][4]) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) zoom_add4(sum + c * per + ((row0 + ry) / k) * ow, cx, k, ob[c]);
  }
};
// The output rows a chunk of `rows` source rows meets, for the kernels whose lanes sum a column of source rows in registers first
// (box_mean_row's order): k <= band: the tile is ONE chunk of orows whole output rows, k source rows each; k > band: the tile is one
// output row and every chunk a part of it.  A lane's work item is (output row of the chunk, aligned uchar4 column): `each` source rows.
struct ZoomChunk {
  int nor, each;
};
__device__ __forceinline__ ZoomChunk zoom_chunk(int band, int k, int orows, int rows) {
  const int nor = k <= band ? orows : 1;
  return ZoomChunk{nor, rows / nor};
}
// px_rows for one channel per lane with the column summed first: the item's source bytes are loaded first, every load in flight at
// once (the rows are at most RENDER_BAND), then px4 per row into col, then one put
template <typename Px>
__device__ __forceinline__ void px_columns(const Px& px, int X0, int Y0, const ZoomChunk ch, int L, const ZoomSums& to) {
  static_assert(Px::NC == 1, "one channel per lane");
  for (int idx = threadIdx.x; idx < ch.nor * L; idx += 256) {
    const int oy = idx / L, cx = (idx - oy * L) * 4;
    const int X = X0 + cx, Yb = Y0 + oy * ch.each;
    int col[1][4] = {{0, 0, 0, 0}};
    uchar4 pvs[RENDER_BAND][1];
#pragma unroll
    for (int r = 0; r < RENDER_BAND; ++r) {
      pvs[r][0] = make_uchar4(0, 0, 0, 0);
      if (r < ch.each) px.load(X, Yb + r, pvs[r]);
    }
#pragma unroll
    for (int r = 0; r < RENDER_BAND; ++r) {
      if (r >= ch.each) break;
      unsigned char ob[1][4];
      px(X, Yb + r, pvs[r], ob);
#pragma unroll
      for (int e = 0; e < 4; ++e) col[0][e] += ob[0][e];
    }
    to.put(oy * ch.each, cx, col);
  }
}
// one chunk of a tile -> the sums: `rows` source rows of 4L bytes at (X0, Y0), source row row0 of the tile
template <typename Px>
__device__ __forceinline__ void zoom_chunk_sum(const Px& px, int (*sum)[ZoomShape<Px::NC>::SUMS], const ZoomTileAt& z, int k, int X0, int Y0,
                                               int row0, int rows, int L) {
  const ZoomSums to{&sum[0][0], ZoomShape<Px::NC>::SUMS, z.ow, k, row0};
  if constexpr (Px::NC == 3) px_rows(px, X0, Y0, rows, L, to);
  else px_columns(px, X0, Y0, zoom_chunk(ZoomShape<Px::NC>::BAND, k, z.orows, rows), L, to);
}
template <int NC, int SUMS>
__device__ __forceinline__ void zoom_clear(int (*sum)[SUMS], const ZoomTileAt& z) {
  for (int c = 0; c < NC; ++c)
    for (int j = threadIdx.x; j < z.orows * z.ow; j += 256) sum[c][j] = 0;
}
// sum[c][orows][ow] -> the tile's bytes of NC output planes (u8[vh][vw]) from `planes` on: (sum + k*k/2) / (k*k), one uchar4 per lane
template <int NC, int SUMS>
__device__ __forceinline__ void zoom_store(const int (*sum)[SUMS], const ZoomTileAt& z, int k, unsigned char* planes, int vw, int vh) {
  const int L = z.ow >> 2, d = k * k, half = d / 2;
  for (int c = 0; c < NC; ++c)
    for (int j = threadIdx.x; j < z.orows * L; j += 256) {
      const int ry = j / L, q = (j - ry * L) * 4;
      const int* p = sum[c] + ry * z.ow + q;
      *reinterpret_cast<uchar4*>(planes + ((size_t)c * vh + z.oy0 + ry) * vw + z.ox0 + q) =
          make_uchar4((unsigned char)((p[0] + half) / d), (unsigned char)((p[1] + half) / d), (unsigned char)((p[2] + half) / d),
                      (unsigned char)((p[3] + half) / d));
    }
}
// the same, packed: the three sums of each of a lane's four pixels divided, then store_packed4 into the window (u8 [vh][vw][bpp])
template <int SUMS>
__device__ __forceinline__ void zoom_store_packed(const int (*sum)[SUMS], const ZoomTileAt& z, int k, unsigned char* window, int vw, int format) {
  const int L = z.ow >> 2, d = k * k, half = d / 2;
  for (int j = threadIdx.x; j < z.orows * L; j += 256) {
    const int ry = j / L, q = (j - ry * L) * 4;
    unsigned char ob[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[c][e] = (unsigned char)((sum[c][ry * z.ow + q + e] + half) / d);
    store_packed4(window + ((size_t)(z.oy0 + ry) * vw + z.ox0 + q) * pixels_bpp(format), format, ob);
  }
}
// where window i of a call starts in `out`, and the sink of its band that starts at row y0: planar, channel c0's plane (StoreRows
// over `out`, or over the source itself for out == nullptr); packed, the window's pixels
__device__ __forceinline__ unsigned char* packed_window(unsigned char* out, int i, int vw, int vh, int format) {
  return out + (size_t)i * vh * vw * pixels_bpp(format);
}

// ---- the kernels ---------------------------------------------------------------------------------------------------------------------
// Plain: grid (bands or tiles, 3, n), a lane owns 4 consecutive bytes of channel blockIdx.y.  Guided: grid (bands or tiles, 1, n), a
// lane owns its 4 pixels in all three channels.  A call may mix kinds; the kind is uniform over the workgroup.
// PACKED: `out` holds interleaved pixels of `format` (PIXELS_*), u8 [n][vh][vw][bpp].  A lane owns all three channels
// with or without a guide, so the grid is the guided one (y = 1) and so are band and tile; out is never nullptr.  Not PACKED, `format`
// is not read: these instantiations are the planar kernels as they always were.

// render.  grid x: bands of BAND output rows.  The band's field rows go to LDS once; every tap reads from there.
template <bool GUIDED, bool PACKED>
__global__ __launch_bounds__(256) void session_render_kernel(SessionPool P, const float* __restrict__ table, const int* __restrict__ views,
                                                             int vw, int vh, unsigned char* out, int format) {
  constexpr int NC = window_nc(GUIDED, PACKED), BAND = StagedRows<GUIDED, NC>::BAND;
  __shared__ StagedRows<GUIDED, NC> rows;
  __shared__ float tab[GUIDED ? SESSION_GUIDE_TABLE_LEN : 1];
  const int s = P.scale, S = 64 * s, c0 = NC == 3 ? 0 : blockIdx.y, i = blockIdx.z;
  const int id = views[3 * i], vx = views[3 * i + 1], vy = views[3 * i + 2];
  const int y0 = blockIdx.x * BAND, nrows = min(BAND, vh - y0);
  const FieldRows fr = field_rows(vy + y0, vy + y0 + nrows - 1, s);
  stage_rows(rows, P, id, c0, fr);
  if constexpr (GUIDED) stage_guide_table(tab, table);
  __syncthreads();
  const size_t plane = (size_t)S * S;
  unsigned char* src = P.src + ((size_t)id * 3 + c0) * plane;
  const RenderPx4<GUIDED, NC> px{rows, tab, src, plane, S, s, P.kind[id], fr.fr0};
  if constexpr (PACKED) {
    px_rows(px, vx, vy + y0, nrows, vw >> 2, PackedRows{packed_window(out, i, vw, vh, format), vw, y0, format});
  } else {
    const StoreRows to = out ? StoreRows{out + ((size_t)i * 3 + c0) * vh * vw, (size_t)vh * vw, vw, y0, 0} : StoreRows{src, plane, S, vy + y0, vx};
    px_rows(px, vx, vy + y0, nrows, vw >> 2, to);
  }
}

// compose.  grid x: bands of BAND output rows
template <bool GUIDED, bool PACKED>
__global__ __launch_bounds__(256) void canvas_compose_kernel(SessionCanvases C, SessionPool P, const float* __restrict__ table,
                                                             const int* __restrict__ windows, int vw, int vh, unsigned char* out, int format) {
  constexpr int NC = window_nc(GUIDED, PACKED), BAND = StagedRows<GUIDED, NC>::BAND;
  __shared__ CanvasStage<GUIDED, NC> st;
  __shared__ float tab[GUIDED ? SESSION_GUIDE_TABLE_LEN : 1];
  const int c0 = NC == 3 ? 0 : blockIdx.y, i = blockIdx.z;
  const int cv = windows[3 * i], vx = windows[3 * i + 1], vy = windows[3 * i + 2];
  const int y0 = blockIdx.x * BAND, nrows = min(BAND, vh - y0);
  const int Y0 = vy + y0, Y1 = Y0 + nrows - 1;   // the band's rows on the canvas, both inclusive
  const int nk = canvas_keep(st, tab, C, P, table, cv, vx, vw, Y0, Y1);
  canvas_stage(st, P, nk, c0, false, Y0, Y1);
  __syncthreads();
  const size_t plane = (size_t)C.max_h * C.max_w;
  unsigned char* src = C.pix + ((size_t)cv * 3 + c0) * plane;
  const ComposePx4<GUIDED, NC> px{st, tab, src, plane, C.max_w, C.feather, nk};
  if constexpr (PACKED) {
    px_rows(px, vx, Y0, nrows, vw >> 2, PackedRows{packed_window(out, i, vw, vh, format), vw, y0, format});
  } else {
    const StoreRows to = out ? StoreRows{out + ((size_t)i * 3 + c0) * vh * vw, (size_t)vh * vw, vw, y0, 0} : StoreRows{src, plane, C.max_w, Y0, vx};
    px_rows(px, vx, Y0, nrows, vw >> 2, to);
  }
}

// render at 1/k.  grid x: row groups * column tiles
template <bool GUIDED, bool PACKED>
__global__ __launch_bounds__(256) void session_render_zoom_kernel(SessionPool P, const float* __restrict__ table,
                                                                  const int* __restrict__ views, int vw, int vh, int k,
                                                                  unsigned char* __restrict__ out, int format) {
  constexpr int NC = window_nc(GUIDED, PACKED);
  using Z = ZoomShape<NC>;
  __shared__ StagedRows<GUIDED, NC> rows;
  __shared__ float tab[GUIDED ? SESSION_GUIDE_TABLE_LEN : 1];
  __shared__ int sum[NC][Z::SUMS];
  const int s = P.scale, S = 64 * s, c0 = NC == 3 ? 0 : blockIdx.y, i = blockIdx.z;
  const int id = views[3 * i], vx = views[3 * i + 1], vy = views[3 * i + 2];
  const ZoomTileAt z = zoom_tile_at(Z::BAND, Z::TILE, k, vw, vh);
  const int X0 = vx + k * z.ox0, Y0 = vy + k * z.oy0, R = k * z.orows, L = (k * z.ow) >> 2;   // the tile in the picture
  zoom_clear<NC>(sum, z);
  if constexpr (GUIDED) stage_guide_table(tab, table);
  const size_t plane = (size_t)S * S;
  const int kind = P.kind[id];
  for (int y0 = 0; y0 < R; y0 += Z::BAND) {
    const int nrows = min(Z::BAND, R - y0);
    const FieldRows fr = field_rows(Y0 + y0, Y0 + y0 + nrows - 1, s);
    stage_rows(rows, P, id, c0, fr);
    __syncthreads();   // the first one also publishes the zeroed sums
    const RenderPx4<GUIDED, NC> px{rows, tab, P.src + ((size_t)id * 3 + c0) * plane, plane, S, s, kind, fr.fr0};
    zoom_chunk_sum(px, sum, z, k, X0, Y0 + y0, y0, nrows, L);
    __syncthreads();   // rows is restaged; after the last chunk: the sums are complete
  }
  if constexpr (PACKED) zoom_store_packed(sum, z, k, packed_window(out, i, vw, vh, format), vw, format);
  else zoom_store<NC>(sum, z, k, out + ((size_t)i * 3 + c0) * vh * vw, vw, vh);
}

// compose at 1/k.  grid x: row groups * column tiles
template <bool GUIDED, bool PACKED>
__global__ __launch_bounds__(256) void canvas_compose_zoom_kernel(SessionCanvases C, SessionPool P, const float* __restrict__ table,
                                                                  const int* __restrict__ windows, int vw, int vh, int k,
                                                                  unsigned char* __restrict__ out, int format) {
  constexpr int NC = window_nc(GUIDED, PACKED);
  using Z = ZoomShape<NC>;
  __shared__ CanvasStage<GUIDED, NC> st;
  __shared__ float tab[GUIDED ? SESSION_GUIDE_TABLE_LEN : 1];
  __shared__ int sum[NC][Z::SUMS];
  const int c0 = NC == 3 ? 0 : blockIdx.y, i = blockIdx.z;
  const int cv = windows[3 * i], vx = windows[3 * i + 1], vy = windows[3 * i + 2];
  const ZoomTileAt z = zoom_tile_at(Z::BAND, Z::TILE, k, vw, vh);
  const int X0 = vx + k * z.ox0, Y0 = vy + k * z.oy0, R = k * z.orows, L = (k * z.ow) >> 2;   // the tile on the canvas
  zoom_clear<NC>(sum, z);
  const int nk = canvas_keep(st, tab, C, P, table, cv, X0, k * z.ow, Y0, Y0 + R - 1);   // once: the tile's rows
  const size_t plane = (size_t)C.max_h * C.max_w;
  const ComposePx4<GUIDED, NC> px{st, tab, C.pix + ((size_t)cv * 3 + c0) * plane, plane, C.max_w, C.feather, nk};
  for (int y0 = 0; y0 < R; y0 += Z::BAND) {
    const int nrows = min(Z::BAND, R - y0);
    canvas_stage(st, P, nk, c0, R > Z::BAND, Y0 + y0, Y0 + y0 + nrows - 1);
    __syncthreads();   // the first one also publishes the zeroed sums
    zoom_chunk_sum(px, sum, z, k, X0, Y0 + y0, y0, nrows, L);
    __syncthreads();   // frows and rows are rewritten; after the last chunk: the sums are complete
  }
  if constexpr (PACKED) zoom_store_packed(sum, z, k, packed_window(out, i, vw, vh, format), vw, format);
  else zoom_store<NC>(sum, z, k, out + ((size_t)i * 3 + c0) * vh * vw, vw, vh);
}

// compose over oriented placements: the plain kernels' grid and loops, nothing staged but the kept placements
template <bool PACKED>
__global__ __launch_bounds__(256) void canvas_compose_oriented_kernel(SessionCanvases C, const int* __restrict__ otable, SessionPool P,
                                                                      const int* __restrict__ windows, int vw, int vh, unsigned char* out,
                                                                      int format) {
  constexpr int NC = window_nc(false, PACKED), BAND = ZoomShape<NC>::BAND;
  __shared__ OrientedStage st;
  const int c0 = NC == 3 ? 0 : blockIdx.y, i = blockIdx.z;
  const int cv = windows[3 * i], vx = windows[3 * i + 1], vy = windows[3 * i + 2];
  const int y0 = blockIdx.x * BAND, nrows = min(BAND, vh - y0);
  const int Y0 = vy + y0;
  const int nk = oriented_keep(st, otable, P, cv, vx, vw, Y0, Y0 + nrows - 1);
  const size_t plane = (size_t)C.max_h * C.max_w;
  unsigned char* src = C.pix + ((size_t)cv * 3 + c0) * plane;
  const ComposeOrientedPx4<NC> px{st, P.field + c0 * (64 * 64), src, plane, C.max_w, C.feather, nk};
  if constexpr (PACKED) {
    px_rows(px, vx, Y0, nrows, vw >> 2, PackedRows{packed_window(out, i, vw, vh, format), vw, y0, format});
  } else {
    const StoreRows to = out ? StoreRows{out + ((size_t)i * 3 + c0) * vh * vw, (size_t)vh * vw, vw, y0, 0} : StoreRows{src, plane, C.max_w, Y0, vx};
    px_rows(px, vx, Y0, nrows, vw >> 2, to);
  }
}
// the same at 1/k: canvas_compose_zoom_kernel<false>'s tiles and chunks; the sums are LDS adds, so the chunks need no barrier between them
template <bool PACKED>
__global__ __launch_bounds__(256) void canvas_compose_oriented_zoom_kernel(SessionCanvases C, const int* __restrict__ otable, SessionPool P,
                                                                           const int* __restrict__ windows, int vw, int vh, int k,
                                                                           unsigned char* __restrict__ out, int format) {
  constexpr int NC = window_nc(false, PACKED);
  using Z = ZoomShape<NC>;
  __shared__ OrientedStage st;
  __shared__ int sum[NC][Z::SUMS];
  const int c0 = NC == 3 ? 0 : blockIdx.y, i = blockIdx.z;
  const int cv = windows[3 * i], vx = windows[3 * i + 1], vy = windows[3 * i + 2];
  const ZoomTileAt z = zoom_tile_at(Z::BAND, Z::TILE, k, vw, vh);
  const int X0 = vx + k * z.ox0, Y0 = vy + k * z.oy0, R = k * z.orows, L = (k * z.ow) >> 2;   // the tile on the canvas
  zoom_clear<NC>(sum, z);
  const int nk = oriented_keep(st, otable, P, cv, X0, k * z.ow, Y0, Y0 + R - 1);   // its barrier also publishes the zeroed sums
  const size_t plane = (size_t)C.max_h * C.max_w;
  const ComposeOrientedPx4<NC> px{st, P.field + c0 * (64 * 64), C.pix + ((size_t)cv * 3 + c0) * plane, plane, C.max_w, C.feather, nk};
  for (int y0 = 0; y0 < R; y0 += Z::BAND) zoom_chunk_sum(px, sum, z, k, X0, Y0 + y0, y0, min(Z::BAND, R - y0), L);
  __syncthreads();   // the sums are complete
  if constexpr (PACKED) zoom_store_packed(sum, z, k, packed_window(out, i, vw, vh, format), vw, format);
  else zoom_store<NC>(sum, z, k, out + ((size_t)i * 3 + c0) * vh * vw, vw, vh);
}

// ---- the launchers ---------------------------------------------------------------------------------------------------------------
// what all check alike: the count, the zoom, the window against its source, the table of windows, at 1/k the result, and the pixel
// format (0 planar, PIXELS_*), which needs an `out`: in place is planar
static bool window_args_ok(int n, int zoom, int vw, int vh, int src_w, int src_h, const void* win, const unsigned char* out, int format) {
  return n >= 1 && n <= 65535 && zoom >= 1 && zoom <= ZOOM_MAX && win && vw >= 4 && (vw & 3) == 0 && vh >= 1 && vw <= src_w / zoom &&
         vh <= src_h / zoom && (zoom == 1 || (out && (reinterpret_cast<uintptr_t>(out) & 3) == 0)) && format >= 0 && format <= PIXELS_BGRA &&
         (format == 0 || (out && (reinterpret_cast<uintptr_t>(out) & 3) == 0));
}
// wide: a lane owns all three channels (guided, or packed pixels)
static dim3 window_grid(bool wide, int zoom, int vw, int vh, int n) {
  const int band = wide ? GUIDE_BAND : RENDER_BAND, planes = wide ? 1 : 3;
  if (zoom == 1) return dim3((vh + band - 1) / band, planes, n);
  const ZoomSplit z = zoom_split(band, wide ? ZoomShape<3>::TILE : ZoomShape<1>::TILE, zoom, vw);
  return dim3((unsigned)((vh + z.orows - 1) / z.orows) * z.ntiles, planes, n);
}
hipError_t launch_session_render(const SessionPool& P, const float* table, const int* views, int vw, int vh, int zoom, unsigned char* out, int n,
                                 int format, hipStream_t s) {
  const int S = 64 * P.scale;
  if (P.scale < 1 || P.scale > 16 || !P.src || !P.field || !P.kind || (table && !P.gim) ||
      !window_args_ok(n, zoom, vw, vh, S, S, views, out, format))
    return hipErrorInvalidValue;
  if (!out && (vw != S || vh != S)) return hipErrorInvalidValue;
  const dim3 grid = window_grid(table || format, zoom, vw, vh, n);
  if (zoom == 1) {
    auto kernel = format ? (table ? session_render_kernel<true, true> : session_render_kernel<false, true>)
                         : (table ? session_render_kernel<true, false> : session_render_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, P, table, views, vw, vh, out, format);
  } else {
    auto kernel = format ? (table ? session_render_zoom_kernel<true, true> : session_render_zoom_kernel<false, true>)
                         : (table ? session_render_zoom_kernel<true, false> : session_render_zoom_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, P, table, views, vw, vh, zoom, out, format);
  }
  return hipGetLastError();
}
hipError_t launch_canvas_compose(const SessionCanvases& C, const SessionPool& P, const float* table, const int* windows, int vw, int vh, int zoom,
                                 unsigned char* out, int n, int format, hipStream_t s) {
  if (!canvases_ok(C) || !P.field || !P.kind || (table && !P.gim) || !window_args_ok(n, zoom, vw, vh, C.max_w, C.max_h, windows, out, format))
    return hipErrorInvalidValue;
  if (out ? (reinterpret_cast<uintptr_t>(out) & 3) != 0 : n != 1) return hipErrorInvalidValue;
  const dim3 grid = window_grid(table || format, zoom, vw, vh, n);
  if (zoom == 1) {
    auto kernel = format ? (table ? canvas_compose_kernel<true, true> : canvas_compose_kernel<false, true>)
                         : (table ? canvas_compose_kernel<true, false> : canvas_compose_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, C, P, table, windows, vw, vh, out, format);
  } else {
    auto kernel = format ? (table ? canvas_compose_zoom_kernel<true, true> : canvas_compose_zoom_kernel<false, true>)
                         : (table ? canvas_compose_zoom_kernel<true, false> : canvas_compose_zoom_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, C, P, table, windows, vw, vh, zoom, out, format);
  }
  return hipGetLastError();
}
hipError_t launch_canvas_compose_oriented(const SessionCanvases& C, const int* otable, const SessionPool& P, const int* windows, int vw, int vh,
                                          int zoom, unsigned char* out, int n, int format, hipStream_t s) {
  if (!canvases_ok(C) || !otable || !P.field || !P.kind || !window_args_ok(n, zoom, vw, vh, C.max_w, C.max_h, windows, out, format))
    return hipErrorInvalidValue;
  if (out ? (reinterpret_cast<uintptr_t>(out) & 3) != 0 : n != 1) return hipErrorInvalidValue;
  const dim3 grid = window_grid(format != 0, zoom, vw, vh, n);
  if (zoom == 1) {
    auto kernel = format ? canvas_compose_oriented_kernel<true> : canvas_compose_oriented_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, C, otable, P, windows, vw, vh, out, format);
  } else {
    auto kernel = format ? canvas_compose_oriented_zoom_kernel<true> : canvas_compose_oriented_zoom_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, C, otable, P, windows, vw, vh, zoom, out, format);
  }
  return hipGetLastError();
}

}  // namespace ian
