// ian_tip_check.h -- brush tips (ian_sessions_set_tip, ian_session_brush_tip, ian_session_path_tip): the checks that
// need nothing but the numbers.  Host only, no HIP and no handle: the runtime (ian_rt_session.inc) turns a refusal into its -7
// message, and a stand-alone program (tests/tip_check_main.cpp) drives the same functions under the sanitizers.
#ifndef IAN_TIP_CHECK_H_
#define IAN_TIP_CHECK_H_

#include <cmath>
#include <cstdint>

namespace ian {

constexpr int TIP_MAX_SIDE = 64;    // 1 <= tw, th <= 64: a tip is at most the 64x64 image, and a slot of the device array holds that
constexpr int TIP_MAX_COUNT = 64;   // ian_sessions_reserve_tips: count 0..64
constexpr int TIP_SLOT = TIP_MAX_SIDE * TIP_MAX_SIDE;   // floats per tip on the device, row stride TIP_MAX_SIDE

enum TipRefusal {
  TIP_OK = 0,
  TIP_BAD_SIZE,      // tw or th outside 1..64
  TIP_BAD_WEIGHT,    // a weight that is negative, infinite or NaN
  TIP_OUTSIDE,       // an event's tip outside -1..count-1
  TIP_NEVER_SET,     // an event's tip was never given weights
  TIP_RECT_SIZE,     // an event's rectangle is not exactly tw x th
};

inline TipRefusal tip_check_size(int tw, int th) {
  return (tw >= 1 && tw <= TIP_MAX_SIDE && th >= 1 && th <= TIP_MAX_SIDE) ? TIP_OK : TIP_BAD_SIZE;
}

// wn: [th][tw] of a size that passed tip_check_size.  *at: the index of the first refused weight.  All zero is allowed.
inline TipRefusal tip_check_weights(const float* wn, int tw, int th, int* at) {
  for (int i = 0; i < tw * th; ++i)
    if (!(wn[i] >= 0.0f) || std::isinf(wn[i])) {   // !(>= 0): negative or NaN
      if (at) *at = i;
      return TIP_BAD_WEIGHT;
    }
  return TIP_OK;
}

// One event (or one point of a path) against its tip.  wh: [count][2] = (tw, th) per tip of the reservation, (0, 0) for a tip never
// set.  tip == -1 names no tip: the event is a rectangle event and nothing here concerns it.  The differences are taken in 64 bits: the
// rectangle's own checks may not have run yet.
inline TipRefusal tip_check_event(int tip, int count, const int32_t* wh, int c1, int r1, int c2, int r2) {
  if (tip == -1) return TIP_OK;
  if (tip < -1 || tip >= count) return TIP_OUTSIDE;
  const int tw = wh[2 * tip], th = wh[2 * tip + 1];
  if (tw < 1 || th < 1) return TIP_NEVER_SET;
  if ((long long)c2 - c1 != tw || (long long)r2 - r1 != th) return TIP_RECT_SIZE;
  return TIP_OK;
}

// a tip's weights [th][tw] into / out of its slot [64][64] (the rest of the slot is zero)
inline void tip_to_slot(const float* wn, int tw, int th, float* slot) {
  for (int i = 0; i < TIP_SLOT; ++i) slot[i] = 0.0f;
  for (int r = 0; r < th; ++r)
    for (int c = 0; c < tw; ++c) slot[r * TIP_MAX_SIDE + c] = wn[r * tw + c];
}
// a tip's shape for the footprint it leaves in the user mask (npe_ops.tip_footprint): s = float64(wn) / float64(max wn), one float64
// division per pixel, into a slot [64][64] of doubles (the rest of the slot is zero); all zeros when max wn == 0
inline void tip_shape_slot(const float* wn, int tw, int th, double* slot) {
  double m = 0.0;
  for (int i = 0; i < tw * th; ++i) m = (double)wn[i] > m ? (double)wn[i] : m;
  for (int i = 0; i < TIP_SLOT; ++i) slot[i] = 0.0;
  if (!(m > 0.0)) return;
  for (int r = 0; r < th; ++r)
    for (int c = 0; c < tw; ++c) slot[r * TIP_MAX_SIDE + c] = (double)wn[r * tw + c] / m;
}
inline void tip_from_slot(const float* slot, int tw, int th, float* wn) {
  for (int r = 0; r < th; ++r)
    for (int c = 0; c < tw; ++c) wn[r * tw + c] = slot[r * TIP_MAX_SIDE + c];
}

}  // namespace ian

#endif  // IAN_TIP_CHECK_H_
