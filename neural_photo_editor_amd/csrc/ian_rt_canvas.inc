// ian_rt_canvas.inc -- canvases: whole photos in device memory, edit sessions placed on them as squares, the composed result.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp after ian_rt_session.inc (whose helpers it uses, and
// which declares, at its top, what the session calls need from here).  DESIGN.md 4.7; include/ian.h has the contract.
//
// One reservation (ian_sessions_reserve_canvas) owns everything here: `count` pictures u8[3,max_h,max_w] in one allocation, the device
// table of CANVAS_MAX_PLACED placements per canvas, the window table of a compose call, and the range weights of
// ian_sessions_reserve_edges while they are set.  The arrays are per canvas, not per
// session, so they are not columns of SESS_COLUMNS; a placement is not part of a saved session.  The host owns the placements
// (S.placed, one entry per session id; S.ctab_shadow, the device table's copy in ascending session id per canvas); a canvas whose
// list changed is marked dirty and its 8 entries are uploaded on the stream of the call that changed it.  A pool without the
// reservation has S.canv.pix == nullptr and S.placed empty, and every hook below returns at once.
// Oriented placements (ian_place_oriented, DESIGN.md 4.16) are a second form of the same thing: S.oplaced beside S.placed (a session is
// in at most one, a canvas holds one form), a second device table S.d_otab from the first oriented place on, and the same hooks.
namespace {

constexpr int CANVAS_MAX_COUNT = 64, CANVAS_MIN_SIDE = 64, CANVAS_MAX_SIDE = 8192, CANVAS_MAX_FEATHER = 16;
static_assert(CANVAS_MAX_PLACED == IAN_CANVAS_MAX_PLACED, "the kernels' table and the header agree");
static_assert(sizeof(ian_canvas_placement) == 5 * sizeof(int32_t), "ian_canvas_placement is 5 words");
static_assert(sizeof(ian_canvas_window) == 3 * sizeof(int32_t), "ian_canvas_window is 3 words");
static_assert(sizeof(ian_canvas_oriented) == 6 * sizeof(int32_t), "ian_canvas_oriented is 6 words");

size_t canvas_plane_bytes(const SessionCanvases& C) { return (size_t)C.max_h * (size_t)C.max_w; }
unsigned char* canvas_pixels(const SessionCanvases& C, int canvas) { return C.pix + (size_t)canvas * 3 * canvas_plane_bytes(C); }

void canvases_free(ian_handle* h) {
  auto& S = h->sess;
  if (S.canv.pix) (void)hipFree(S.canv.pix);
  if (S.canv.table) (void)hipFree(S.canv.table);
  if (S.d_cwin) (void)hipFree(S.d_cwin);
  if (S.d_edges) (void)hipFree(S.d_edges);
  if (S.d_otab) (void)hipFree(S.d_otab);
  S.canv = SessionCanvases{};
  S.d_cwin = nullptr;
  S.d_edges = nullptr;
  S.d_otab = nullptr;
  S.canvas_wh.clear();
  S.placed.clear();
  S.ctab_shadow.clear();
  S.cdirty.clear();
  S.oplaced.clear();
  S.otab_shadow.clear();
  S.odirty.clear();
}

// placed in either form (ian_canvas_place / ian_place_oriented); a session is in at most one
bool canvas_is_oriented(const ian_handle* h, int id) {
  const auto& S = h->sess;
  return (size_t)id < S.oplaced.size() && S.oplaced[id].canvas >= 0;
}
bool canvas_is_placed(const ian_handle* h, int id) {
  const auto& S = h->sess;
  return ((size_t)id < S.placed.size() && S.placed[id].canvas >= 0) || canvas_is_oriented(h, id);
}
// how many oriented placements a canvas holds (canvas < 0: all canvases together)
int canvas_oriented_count(const ian_handle* h, int canvas) {
  int k = 0;
  for (const ian_canvas_oriented& p : h->sess.oplaced)
    if (p.canvas >= 0 && (canvas < 0 || p.canvas == canvas)) ++k;
  return k;
}

// the lists of one canvas, rebuilt from S.placed and S.oplaced: ascending session id, -1 behind the last.  The oriented table exists
// from the first ian_place_oriented of a reservation on (S.otab_shadow is empty before): 8 words an entry, (bx, by, m) derived here.
void canvas_table_rebuild(ian_handle* h, int canvas) {
  auto& S = h->sess;
  int32_t* t = S.ctab_shadow.data() + (size_t)canvas * CANVAS_MAX_PLACED * 4;
  int k = 0;
  for (size_t id = 0; id < S.placed.size() && k < CANVAS_MAX_PLACED; ++id) {
    const ian_canvas_placement& p = S.placed[id];
    if (p.canvas != canvas) continue;
    t[4 * k] = (int32_t)id; t[4 * k + 1] = p.x; t[4 * k + 2] = p.y; t[4 * k + 3] = p.scale;
    ++k;
  }
  for (; k < CANVAS_MAX_PLACED; ++k) { t[4 * k] = -1; t[4 * k + 1] = t[4 * k + 2] = t[4 * k + 3] = 0; }
  S.cdirty[canvas] = 1;
  if (S.otab_shadow.empty()) return;
  int32_t* o = S.otab_shadow.data() + (size_t)canvas * CANVAS_MAX_PLACED * 8;
  k = 0;
  for (size_t id = 0; id < S.oplaced.size() && k < CANVAS_MAX_PLACED; ++id) {
    const ian_canvas_oriented& p = S.oplaced[id];
    OrientedDerived d;
    if (p.canvas != canvas || !oriented_derive(p.ax, p.ay, &d)) continue;   // a placement has passed oriented_derive when it was made
    const int32_t e[8] = {(int32_t)id, p.cx2, p.cy2, p.ax, p.ay, d.bx, d.by, d.m};
    memcpy(o + 8 * k++, e, sizeof e);
  }
  for (; k < CANVAS_MAX_PLACED; ++k) {
    memset(o + 8 * k, 0, 8 * sizeof(int32_t));
    o[8 * k] = -1;
  }
  S.odirty[canvas] = 1;
}

void canvas_unplace(ian_handle* h, int id) {
  if (!canvas_is_placed(h, id)) return;
  auto& S = h->sess;
  const bool oriented = canvas_is_oriented(h, id);
  const int canvas = oriented ? S.oplaced[id].canvas : S.placed[id].canvas;
  if (oriented) S.oplaced[id].canvas = -1;
  else S.placed[id].canvas = -1;
  canvas_table_rebuild(h, canvas);
}

int canvas_table_flush(ian_handle* h, hipStream_t st) {
  auto& S = h->sess;
  for (size_t c = 0; c < S.cdirty.size(); ++c) {
    if (S.cdirty[c]) {
      const size_t at = c * CANVAS_MAX_PLACED * 4;
      HIPCHK(h, hipMemcpyAsync(S.canv.table + at, S.ctab_shadow.data() + at, CANVAS_MAX_PLACED * 4 * sizeof(int32_t), hipMemcpyHostToDevice, st));
      S.cdirty[c] = 0;
    }
    if (S.odirty[c] && S.d_otab) {
      const size_t at = c * CANVAS_MAX_PLACED * 8;
      HIPCHK(h, hipMemcpyAsync(S.d_otab + at, S.otab_shadow.data() + at, CANVAS_MAX_PLACED * 8 * sizeof(int32_t), hipMemcpyHostToDevice, st));
      S.odirty[c] = 0;
    }
  }
  return 0;
}

// ian_sessions_reserve(capacity) has rebuilt the pool (the device is idle): S.placed and S.oplaced follow the capacity
int canvases_pool_resized(ian_handle* h) {
  auto& S = h->sess;
  if (!S.canv.pix) return 0;
  for (size_t id = (size_t)S.capacity; id < S.placed.size(); ++id) canvas_unplace(h, (int)id);
  S.placed.resize((size_t)S.capacity, ian_canvas_placement{0, -1, 0, 0, 0});
  S.oplaced.resize((size_t)S.capacity, ian_canvas_oriented{0, -1, 0, 0, 0, 0});
  int rc = canvas_table_flush(h, nullptr);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(nullptr));
  return 0;
}

int canvas_need(ian_handle* h, const char* fn) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (!h->sess.canv.pix) return fail(h, -6, "%s: no canvas reservation (call ian_sessions_reserve_canvas first)", fn);
  return 0;
}
// a canvas id of this reservation that holds a picture; item < 0: the call names one canvas only
int canvas_check_id(ian_handle* h, const char* fn, int item, int canvas, bool need_put) {
  auto& S = h->sess;
  char where[32] = "";
  if (item >= 0) snprintf(where, sizeof where, "item %d: ", item);
  if (canvas < 0 || canvas >= S.canv.count) return fail(h, -7, "%s: %scanvas %d outside 0..%d", fn, where, canvas, S.canv.count - 1);
  if (need_put && !S.canvas_wh[2 * canvas]) return fail(h, -7, "%s: %scanvas %d holds no picture (call ian_canvas_put first)", fn, where, canvas);
  return 0;
}

int sessions_reserve_canvas(ian_handle* h, int count, int max_w, int max_h, int feather) {
  const char* fn = "ian_sessions_reserve_canvas";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_HIRES))) return rc;
  if (count < 0 || count > CANVAS_MAX_COUNT) return fail(h, -7, "%s: count %d outside 0..%d", fn, count, CANVAS_MAX_COUNT);
  if (count > 0 && S.d_guide)   // the compose shares the plain bilinear tap and promises ian_session_render's bytes
    return fail(h, -6, "%s: a guide is reserved: free it first (ian_sessions_reserve_guide(NULL, 0))", fn);
  if (count > 0) {
    if (max_w < CANVAS_MIN_SIDE || max_w > CANVAS_MAX_SIDE || max_h < CANVAS_MIN_SIDE || max_h > CANVAS_MAX_SIDE)
      return fail(h, -7, "%s: %d x %d: both sizes must be in %d..%d", fn, max_w, max_h, CANVAS_MIN_SIDE, CANVAS_MAX_SIDE);
    if (max_w & 3) return fail(h, -7, "%s: max_w %d is not a multiple of 4", fn, max_w);
    if (feather < 0 || feather > CANVAS_MAX_FEATHER) return fail(h, -7, "%s: feather %d outside 0..%d", fn, feather, CANVAS_MAX_FEATHER);
  }
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the arrays that are freed
  h->last_pending = false;
  if (count == 0) {
    canvases_free(h);
    return 0;
  }
  SessionCanvases N = {};
  N.count = count; N.max_w = max_w; N.max_h = max_h; N.feather = feather;
  int* cwin = nullptr;
  const size_t bytes = (size_t)count * 3 * canvas_plane_bytes(N), tbytes = (size_t)count * CANVAS_MAX_PLACED * 4 * sizeof(int32_t);
  hipError_t e = hipMalloc((void**)&N.pix, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&N.table, tbytes);
  if (e == hipSuccess) e = hipMalloc((void**)&cwin, (size_t)BATCH_MAX * 3 * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemset(N.table, 0xff, tbytes);   // every list empty (session -1)
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {   // the old canvases, their pictures and placements stay
    if (N.pix) (void)hipFree(N.pix);
    if (N.table) (void)hipFree(N.table);
    if (cwin) (void)hipFree(cwin);
    (void)hipGetLastError();
    return fail(h, -2, "%s: %s for %d canvases of %zu bytes", fn, hipGetErrorString(e), count, 3 * canvas_plane_bytes(N));
  }
  canvases_free(h);
  S.canv = N;
  S.d_cwin = cwin;
  S.canvas_wh.assign((size_t)2 * count, 0);
  S.placed.assign((size_t)S.capacity, ian_canvas_placement{0, -1, 0, 0, 0});
  S.ctab_shadow.assign((size_t)count * CANVAS_MAX_PLACED * 4, 0);
  S.cdirty.assign((size_t)count, 0);
  S.oplaced.assign((size_t)S.capacity, ian_canvas_oriented{0, -1, 0, 0, 0, 0});   // the oriented table: by the first ian_place_oriented
  S.odirty.assign((size_t)count, 0);
  for (int c = 0; c < count; ++c)
    for (int k = 0; k < CANVAS_MAX_PLACED; ++k) S.ctab_shadow[((size_t)c * CANVAS_MAX_PLACED + k) * 4] = -1;
  return 0;
}

// The edge-aware compose is a setting of the canvas reservation, as the guide is one of the pool: one device table that goes with the
// canvases (canvases_free), and while it exists canvas_compose_enqueue launches the guided kernel.  Records, history and
// ian_session_read know nothing of it.
int sessions_reserve_edges(ian_handle* h, const float* table, int count) {
  const char* fn = "ian_sessions_reserve_edges";
  if (int rc = canvas_need(h, fn)) return rc;
  if ((table || count) && canvas_oriented_count(h, -1))   // the guided compose has no oriented form
    return fail(h, -6, "%s: %d oriented placements exist: the edge-aware compose is for upright squares", fn, canvas_oriented_count(h, -1));
  return guide_table_set(h, fn, h->sess.d_edges, table, count);
}
int sessions_edges(ian_handle* h, float* table_out) {
  const char* fn = "ian_sessions_edges";
  if (int rc = canvas_need(h, fn)) return rc;
  return guide_table_get(h, fn, h->sess.d_edges, table_out);
}

// the three planes of a picture of w x hgt between a packed array [3][hgt][w] and a canvas's rows of max_w bytes
int canvas_copy(ian_handle* h, int canvas, int w, int hgt, unsigned char* packed, bool to_canvas, hipStream_t st) {
  const SessionCanvases& C = h->sess.canv;
  const bool dev = is_device_ptr(packed);
  for (int c = 0; c < 3; ++c) {
    unsigned char* cp = canvas_pixels(C, canvas) + (size_t)c * canvas_plane_bytes(C);
    unsigned char* pp = packed + (size_t)c * hgt * w;
    if (to_canvas)
      HIPCHK(h, hipMemcpy2DAsync(cp, (size_t)C.max_w, pp, (size_t)w, (size_t)w, (size_t)hgt, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    else
      HIPCHK(h, hipMemcpy2DAsync(pp, (size_t)w, cp, (size_t)C.max_w, (size_t)w, (size_t)hgt, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  }
  return 0;
}

int canvas_put(ian_handle* h, int canvas, int w, int hgt, const uint8_t* pixels, void* stream) {
  const char* fn = "ian_canvas_put";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = canvas_check_id(h, fn, -1, canvas, false))) return rc;
  if (!pixels) return fail(h, -1, "null pointer passed to %s", fn);
  if (w < CANVAS_MIN_SIDE || w > S.canv.max_w || hgt < CANVAS_MIN_SIDE || hgt > S.canv.max_h)
    return fail(h, -7, "%s: picture %d x %d outside %d x %d .. %d x %d", fn, w, hgt, CANVAS_MIN_SIDE, CANVAS_MIN_SIDE, S.canv.max_w, S.canv.max_h);
  if (w & 3) return fail(h, -7, "%s: width %d is not a multiple of 4", fn, w);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  if ((rc = canvas_copy(h, canvas, w, hgt, const_cast<uint8_t*>(pixels), true, st))) return rc;
  for (size_t id = 0; id < S.placed.size(); ++id)   // the squares showed another picture; the sessions keep their 64x64 state
    if (S.placed[id].canvas == canvas) S.placed[id].canvas = -1;
  for (ian_canvas_oriented& p : S.oplaced)
    if (p.canvas == canvas) p.canvas = -1;
  canvas_table_rebuild(h, canvas);
  if ((rc = canvas_table_flush(h, st))) return rc;
  S.canvas_wh[2 * canvas] = w;
  S.canvas_wh[2 * canvas + 1] = hgt;
  return session_rows_leave(h, st, is_device_ptr(pixels));
}

int canvas_read(ian_handle* h, int canvas, uint8_t* out, int32_t* wh, void* stream) {
  const char* fn = "ian_canvas_read";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = canvas_check_id(h, fn, -1, canvas, true))) return rc;
  if (wh && is_device_ptr(wh)) return fail(h, -7, "%s: wh must be a host array", fn);
  const int w = S.canvas_wh[2 * canvas], hgt = S.canvas_wh[2 * canvas + 1];
  if (wh) { wh[0] = w; wh[1] = hgt; }
  if (!out) return 0;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  if ((rc = canvas_copy(h, canvas, w, hgt, out, false, st))) return rc;
  return session_rows_leave(h, st, is_device_ptr(out));
}

int canvas_placements(ian_handle* h, int canvas, ian_canvas_placement* out8, int32_t* count) {
  const char* fn = "ian_canvas_placements";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = canvas_check_id(h, fn, -1, canvas, false))) return rc;
  if (!out8 || !count) return fail(h, -1, "null pointer passed to %s", fn);
  int k = 0;
  for (size_t id = 0; id < S.placed.size() && k < CANVAS_MAX_PLACED; ++id)
    if (S.placed[id].canvas == canvas) {
      out8[k] = S.placed[id];
      out8[k++].session = (int32_t)id;
    }
  *count = k;
  return 0;
}

int canvas_placements_oriented(ian_handle* h, int canvas, ian_canvas_oriented* out8, int32_t* count) {
  const char* fn = "ian_placements_oriented";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = canvas_check_id(h, fn, -1, canvas, false))) return rc;
  if (!out8 || !count) return fail(h, -1, "null pointer passed to %s", fn);
  int k = 0;
  for (size_t id = 0; id < S.oplaced.size() && k < CANVAS_MAX_PLACED; ++id)
    if (S.oplaced[id].canvas == canvas) {
      out8[k] = S.oplaced[id];
      out8[k++].session = (int32_t)id;
    }
  *count = k;
  return 0;
}

// Item: ian_canvas_placement (ian_canvas_place) or ian_canvas_oriented (ian_place_oriented); both start (session, canvas)
template <typename Item>
constexpr bool canvas_item_oriented = std::is_same<Item, ian_canvas_oriented>::value;

// What both place calls check once every item is valid on its own: no canvas ends up with placements of both forms, and none with
// more than CANVAS_MAX_PLACED.  A session that is placed, in either form, moves: it leaves its canvas first.
template <typename Item>
int canvas_place_check_load(ian_handle* h, const char* fn, int n, const Item* items) {
  auto& S = h->sess;
  constexpr bool ORIENTED = canvas_item_oriented<Item>;
  std::vector<int> load((size_t)S.canv.count, 0), other((size_t)S.canv.count, 0);   // per canvas: every placement; those of the other form
  auto count = [&](int id, int by) {
    if (S.placed[id].canvas >= 0) { load[S.placed[id].canvas] += by; if (ORIENTED) other[S.placed[id].canvas] += by; }
    if (S.oplaced[id].canvas >= 0) { load[S.oplaced[id].canvas] += by; if (!ORIENTED) other[S.oplaced[id].canvas] += by; }
  };
  for (size_t id = 0; id < S.placed.size(); ++id) count((int)id, 1);
  for (int i = 0; i < n; ++i) count(items[i].session, -1);
  for (int i = 0; i < n; ++i) {
    const int c = items[i].canvas;
    if (other[c] > 0)
      return fail(h, -7, "%s: item %d: canvas %d holds %d %s placements: a canvas holds one form (place upright squares at angle 0)", fn, i, c,
                  other[c], ORIENTED ? "upright" : "oriented");
    if (++load[c] > CANVAS_MAX_PLACED) return fail(h, -7, "%s: item %d: canvas %d already holds %d sessions", fn, i, c, CANVAS_MAX_PLACED);
  }
  return 0;
}

// the box mean (the oriented gather) of n squares -> GIM, IM and the encoder's input, then the open every session call ends in; the
// sessions are placed
template <typename Item>
int canvas_place_run(ian_handle* h, int n, const Item* items, uint8_t* shown, hipStream_t st) {
  auto& S = h->sess;
  constexpr bool ORIENTED = canvas_item_oriented<Item>;
  constexpr int WORDS = sizeof(Item) / sizeof(int32_t);
  int rc = 0;
  // d_tab: n ids (what the open's kernels index), then the n items
  S.tab_shadow.resize((size_t)(1 + WORDS) * n);
  std::vector<int32_t> ids((size_t)n);
  for (int i = 0; i < n; ++i) S.tab_shadow[i] = ids[i] = items[i].session;
  memcpy(S.tab_shadow.data() + n, items, (size_t)n * sizeof(Item));
  HIPCHK(h, hipMemcpyAsync(S.d_tab, S.tab_shadow.data(), (size_t)(1 + WORDS) * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  Slot& xs = h->slots[h->desc.x_slot];
  if ((rc = ensure_slot(h, h->desc.x_slot, n))) return rc;
  if constexpr (ORIENTED) HIPCHK(h, launch_canvas_place_oriented(S.canv, S.arr.pool, S.d_tab + n, S.d_tanh, xs.d, n, st));
  else HIPCHK(h, launch_canvas_place(S.canv, S.arr.pool, S.d_tab + n, S.d_tanh, xs.d, n, st));
  std::vector<char> touched((size_t)S.canv.count, 0);
  for (int i = 0; i < n; ++i) {
    const int id = items[i].session;
    if (S.placed[id].canvas >= 0) touched[S.placed[id].canvas] = 1;   // a session that moves
    if (S.oplaced[id].canvas >= 0) touched[S.oplaced[id].canvas] = 1;
    S.placed[id].canvas = S.oplaced[id].canvas = -1;
    if constexpr (ORIENTED) S.oplaced[id] = items[i];
    else S.placed[id] = items[i];
    touched[items[i].canvas] = 1;
  }
  for (int c = 0; c < S.canv.count; ++c)
    if (touched[c]) canvas_table_rebuild(h, c);
  if ((rc = canvas_table_flush(h, st))) return rc;
  return session_open_finish(h, n, ids.data(), shown, false, 0, st);
}

int canvas_place(ian_handle* h, int n, const ian_canvas_placement* items, uint8_t* shown, void* stream) {
  const char* fn = "ian_canvas_place";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  if ((rc = session_check(h, fn, n, items ? &items->session : nullptr, 5, false, false))) return rc;
  auto& S = h->sess;
  for (int i = 0; i < n; ++i) {
    const ian_canvas_placement& p = items[i];
    if ((rc = canvas_check_id(h, fn, i, p.canvas, true))) return rc;
    if (p.scale < 1 || p.scale > 16) return fail(h, -7, "%s: item %d: scale %d outside 1..16", fn, i, p.scale);
    const int w = S.canvas_wh[2 * p.canvas], hgt = S.canvas_wh[2 * p.canvas + 1], side = 64 * p.scale;
    if (p.x < 0 || p.y < 0 || p.x > w - side || p.y > hgt - side)
      return fail(h, -7, "%s: item %d: square (%d,%d) + %d outside the %d x %d canvas", fn, i, p.x, p.y, side, w, hgt);
  }
  if ((rc = canvas_place_check_load(h, fn, n, items))) return rc;
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);
  TotalTimer tt(h, st);
  return canvas_place_run(h, n, items, shown, st);
}

// the canvases' second device table, by the first oriented place of a reservation: every list empty
int canvas_oriented_table(ian_handle* h, const char* fn) {
  auto& S = h->sess;
  if (S.d_otab) return 0;
  const size_t words = (size_t)S.canv.count * CANVAS_MAX_PLACED * 8;
  int* t = nullptr;
  hipError_t e = hipMalloc((void**)&t, words * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemset(t, 0xff, words * sizeof(int32_t));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    if (t) (void)hipFree(t);
    (void)hipGetLastError();
    return fail(h, -2, "%s: %s for the oriented table of %d canvases", fn, hipGetErrorString(e), S.canv.count);
  }
  S.d_otab = t;
  S.otab_shadow.assign(words, 0);
  for (size_t k = 0; k < words; k += 8) S.otab_shadow[k] = -1;
  return 0;
}

int canvas_place_oriented(ian_handle* h, int n, const ian_canvas_oriented* items, uint8_t* shown, void* stream) {
  const char* fn = "ian_place_oriented";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if (S.d_edges) return fail(h, -6, "%s: an edges table is reserved: free it first (ian_sessions_reserve_edges(NULL, 0))", fn);
  if ((rc = session_check(h, fn, n, items ? &items->session : nullptr, 6, false, false))) return rc;
  for (int i = 0; i < n; ++i) {
    const ian_canvas_oriented& p = items[i];
    if ((rc = canvas_check_id(h, fn, i, p.canvas, true))) return rc;
    OrientedDerived d;
    if (!oriented_derive(p.ax, p.ay, &d))
      return fail(h, -7, "%s: item %d: ax*ax + ay*ay of (%d,%d) outside 2^32..2^40 (a side of 64..1024 pixels)", fn, i, p.ax, p.ay);
    const int w = S.canvas_wh[2 * p.canvas], hgt = S.canvas_wh[2 * p.canvas + 1];
    if (!oriented_inside(w, hgt, p.cx2, p.cy2, p.ax, p.ay, d.m))
      return fail(h, -7, "%s: item %d: square (%d,%d,%d,%d) samples outside the %d x %d canvas", fn, i, p.cx2, p.cy2, p.ax, p.ay, w, hgt);
  }
  if ((rc = canvas_place_check_load(h, fn, n, items))) return rc;
  if ((rc = canvas_oriented_table(h, fn))) return rc;
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);
  TotalTimer tt(h, st);
  return canvas_place_run(h, n, items, shown, st);
}

// what ian_canvas_compose and ian_canvas_brush check about the windows, before anything is enqueued
// zoom: as in session_view_check
int canvas_window_check(ian_handle* h, const char* fn, int n, const ian_canvas_window* w, int vw, int vh, const uint8_t* out, int zoom) {
  int rc = canvas_need(h, fn);
  if (rc || (rc = zoom_check(h, fn, zoom))) return rc;
  auto& S = h->sess;
  if (n < 1 || n > BATCH_MAX) return fail(h, -7, "%s: %d windows outside 1..%d", fn, n, BATCH_MAX);
  if (!w || !out) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(w)) return fail(h, -7, "%s: the windows must be a host array", fn);
  if (vw < 1 || vh < 1) return fail(h, -7, "%s: window %d x %d: both sizes must be at least 1", fn, vw, vh);
  if (vw & 3) return fail(h, -7, "%s: window width %d is not a multiple of 4", fn, vw);
  for (int i = 0; i < n; ++i) {
    if ((rc = canvas_check_id(h, fn, i, w[i].canvas, true))) return rc;
    const int cw = S.canvas_wh[2 * w[i].canvas], ch = S.canvas_wh[2 * w[i].canvas + 1];
    if (w[i].x & 3) return fail(h, -7, "%s: item %d: window x %d is not a multiple of 4", fn, i, w[i].x);
    if (zoom == 1 && (w[i].x < 0 || w[i].y < 0 || w[i].x > cw - vw || w[i].y > ch - vh))
      return fail(h, -7, "%s: item %d: window (%d,%d) + %d x %d outside the %d x %d canvas", fn, i, w[i].x, w[i].y, vw, vh, cw, ch);
    if (zoom_outside(w[i].x, vw, zoom, cw) || zoom_outside(w[i].y, vh, zoom, ch))
      return fail(h, -7, "%s: item %d: window (%d,%d) + %d x %d at zoom %d outside the %d x %d canvas", fn, i, w[i].x, w[i].y, vw, vh, zoom,
                  cw, ch);
  }
  return 0;
}

// the windows of n canvases into d_out (device, u8[n,3,vh,vw]; packed under S.pixels), or, d_out == nullptr, one whole picture over
// its own canvas, planar whatever the pool's format.
// zoom > 1: the windows at 1/zoom.  S.d_edges (ian_sessions_reserve_edges): each photo-mode field's taps weighted by the canvas
int canvas_compose_enqueue(ian_handle* h, int n, const ian_canvas_window* w, int vw, int vh, unsigned char* d_out, hipStream_t st, int zoom) {
  auto& S = h->sess;
  S.cwin_shadow.resize((size_t)3 * n);
  memcpy(S.cwin_shadow.data(), w, (size_t)n * sizeof(ian_canvas_window));
  HIPCHK(h, hipMemcpyAsync(S.d_cwin, S.cwin_shadow.data(), (size_t)n * sizeof(ian_canvas_window), hipMemcpyHostToDevice, st));
  // A canvas holds placements of one form, so a window belongs to one kernel family.  Consecutive windows of one form share a launch
  // and write their own part of d_out, which keeps the call's order; a pool without oriented placements launches once, as ever.
  std::vector<char> oriented((size_t)S.canv.count, 0);
  for (const ian_canvas_oriented& p : S.oplaced)
    if (p.canvas >= 0) oriented[p.canvas] = 1;
  const int format = d_out ? S.pixels : PIXELS_PLANAR;
  const size_t each = (size_t)pixels_bpp(format) * vh * vw;
  for (int a = 0; a < n;) {
    const bool form = oriented[w[a].canvas] != 0;
    int b = a + 1;
    while (b < n && (oriented[w[b].canvas] != 0) == form) ++b;
    unsigned char* out = d_out ? d_out + (size_t)a * each : nullptr;
    if (form) HIPCHK(h, launch_canvas_compose_oriented(S.canv, S.d_otab, S.arr.pool, S.d_cwin + 3 * a, vw, vh, zoom, out, b - a, format, st));
    else HIPCHK(h, launch_canvas_compose(S.canv, S.arr.pool, S.d_edges, S.d_cwin + 3 * a, vw, vh, zoom, out, b - a, format, st));
    a = b;
  }
  return 0;
}

int canvas_compose(ian_handle* h, const char* fn, int n, const ian_canvas_window* w, int vw, int vh, int zoom, uint8_t* out, void* stream) {
  if (int rc = canvas_window_check(h, fn, n, w, vw, vh, out, zoom)) return rc;
  return window_call(h, n, vw, vh, out, stream,
                     [&](unsigned char* d, hipStream_t st) { return canvas_compose_enqueue(h, n, w, vw, vh, d, st, zoom); });
}

int canvas_commit(ian_handle* h, int canvas, uint8_t* shown, void* stream) {
  const char* fn = "ian_canvas_commit";
  int rc = canvas_need(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = canvas_check_id(h, fn, -1, canvas, true))) return rc;
  std::vector<ian_canvas_placement> items;
  std::vector<ian_canvas_oriented> oitems;   // a canvas holds one form: one of the two lists is empty
  for (size_t id = 0; id < S.placed.size(); ++id) {
    if (S.placed[id].canvas == canvas) {
      items.push_back(S.placed[id]);
      items.back().session = (int32_t)id;
    }
    if (S.oplaced[id].canvas == canvas) {
      oitems.push_back(S.oplaced[id]);
      oitems.back().session = (int32_t)id;
    }
  }
  if (items.empty() && oitems.empty()) return 0;   // nothing is placed: the compose is the picture itself
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);
  TotalTimer tt(h, st);
  const ian_canvas_window whole = {canvas, 0, 0};
  if ((rc = canvas_compose_enqueue(h, 1, &whole, S.canvas_wh[2 * canvas], S.canvas_wh[2 * canvas + 1], nullptr, st))) return rc;
  if (!oitems.empty()) return canvas_place_run(h, (int)oitems.size(), oitems.data(), shown, st);
  return canvas_place_run(h, (int)items.size(), items.data(), shown, st);
}

}  // namespace

extern "C" {

int ian_sessions_reserve_canvas(ian_handle* h, int32_t count, int32_t max_w, int32_t max_h, int32_t feather) {
  return h ? sessions_reserve_canvas(h, count, max_w, max_h, feather) : -1;
}
int ian_sessions_reserve_edges(ian_handle* h, const float* table, int32_t count) { return h ? sessions_reserve_edges(h, table, count) : -1; }
int ian_sessions_edges(ian_handle* h, float* table_out) { return h ? sessions_edges(h, table_out) : -1; }
int ian_canvas_put(ian_handle* h, int32_t canvas, int32_t w, int32_t hgt, const uint8_t* pixels, void* stream) {
  return h ? canvas_put(h, canvas, w, hgt, pixels, stream) : -1;
}
int ian_canvas_place(ian_handle* h, int32_t n, const ian_canvas_placement* items, uint8_t* shown, void* stream) {
  return h ? canvas_place(h, n, items, shown, stream) : -1;
}
int ian_canvas_compose(ian_handle* h, int32_t n, const ian_canvas_window* windows, int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  return h ? canvas_compose(h, "ian_canvas_compose", n, windows, vw, vh, 1, out, stream) : -1;
}
int ian_compose_zoom(ian_handle* h, int32_t n, const ian_canvas_window* windows, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out,
                            void* stream) {
  return h ? canvas_compose(h, "ian_compose_zoom", n, windows, vw, vh, zoom, out, stream) : -1;
}
int ian_compose_brush_zoom(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, int32_t m,
                          const ian_canvas_window* windows, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out, void* stream) {
  if (!h) return -1;
  if (!windows) return fail(h, -1, "null pointer passed to ian_compose_brush_zoom");
  return session_brush(h, n, events, shown, stream,
                       BrushWindows{BrushWindows::CANVAS, nullptr, windows, m, vw, vh, out, zoom, "ian_compose_brush_zoom"});
}
int ian_canvas_brush(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, int32_t m,
                     const ian_canvas_window* windows, int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  if (!h) return -1;
  if (!windows) return fail(h, -1, "null pointer passed to ian_canvas_brush");
  return session_brush(h, n, events, shown, stream, BrushWindows{BrushWindows::CANVAS, nullptr, windows, m, vw, vh, out});
}
int ian_compose_brush_soft(ian_handle* h, int32_t n, const ian_session_event* events, const int32_t* tips, uint8_t* shown, int32_t m,
                         const ian_canvas_window* windows, int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  if (!h) return -1;
  if (!windows) return fail(h, -1, "null pointer passed to ian_compose_brush_soft");
  return session_brush(h, n, events, shown, stream,
                       BrushWindows{BrushWindows::CANVAS, nullptr, windows, m, vw, vh, out, 1, "ian_compose_brush_soft"}, true, tips);
}
int ian_canvas_commit(ian_handle* h, int32_t canvas, uint8_t* shown, void* stream) {
  return h ? canvas_commit(h, canvas, shown, stream) : -1;
}
int ian_canvas_read(ian_handle* h, int32_t canvas, uint8_t* out, int32_t wh[2], void* stream) {
  return h ? canvas_read(h, canvas, out, wh, stream) : -1;
}
int ian_canvas_placements(ian_handle* h, int32_t canvas, ian_canvas_placement* out8, int32_t* count) {
  return h ? canvas_placements(h, canvas, out8, count) : -1;
}
int ian_place_oriented(ian_handle* h, int32_t n, const ian_canvas_oriented* items, uint8_t* shown, void* stream) {
  return h ? canvas_place_oriented(h, n, items, shown, stream) : -1;
}
int ian_placements_oriented(ian_handle* h, int32_t canvas, ian_canvas_oriented* out8, int32_t* count) {
  return h ? canvas_placements_oriented(h, canvas, out8, count) : -1;
}

}  // extern "C"
