// ian_rt_session.inc -- device-resident edit sessions: the pool, open / set_latent / brush / read by session id.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
//
// What NPE.py keeps in host globals per editor (GIM, IM, RECON, ERROR, Z, SAMPLE_FLAG) is one row per session id in each array of
// h->sess.arr.pool (SessionPool).  A call names sessions by id; per brush call the only host -> device traffic is the event table
// (11 words per event) and the only device -> host traffic the canvas images.  The host keeps, per session, whether it was opened
// and a counter of its latent's versions (the residency key of ian_session_brush is n ids + n counters, not the latents' bytes).
//
// The pool's arrays (and the history's rings beside it: SessionArrays) are described once, in SESS_COLUMNS: member, bytes per
// session, owning reservation, whether fresh rows start at zero, and the ian_session_field that reads it.  Allocation, the copy of
// the surviving rows, rollback, freeing, the byte count of the -2 messages, ian_session_read and the body of a saved session
// (ian_session_save / ian_session_load: whole sessions as bytes, ian_session_record.h) are loops over that table;
// SESS_SCRATCH does the same for the per-handle device buffers.
// Five reservations own them (sess_free_group frees exactly one):
//   base   ian_sessions_reserve        GIM IM RECON ERROR Z MODE; reserve(0) frees all five groups
//   hires  ian_sessions_reserve_hires  SRC (the photo at S x S, S = 64 * scale), FIELD and FIELD_KIND (what the last call displayed,
//          as something ian_session_render can apply to SRC; DESIGN.md 4.3), and a per-session host flag "SRC holds a photo"
//   local  ian_sessions_reserve_local  UMASK (where the user has brushed) and the LOCAL flags, and per handle the falloff table of
//          the brush footprint (DESIGN.md 4.4)
//   history ian_sessions_reserve_history  per session a ring of depth + 1 saved states: its Z rows and, when the local reservation
//          exists at that moment, its UMASK rows; per session on the host the list and cursor of ian_session_history.h (DESIGN.md 4.5)
//   tips   ian_sessions_reserve_tips   no column: per handle the brush tips' weights (d_tips) and shapes (d_tip_shape) and, on the host,
//          their sizes and the tip-footprint setting (DESIGN.md 4.12, 4.18)
// Without a reservation its pointers are null, no kernel touches them, and launch_session_blend runs session_blend_kernel.
namespace {

constexpr size_t SESS_IMG = 3 * 64 * 64;
constexpr size_t EDIT_TABLE_FLOOR = (size_t)BATCH_MAX * 12;   // words: the table of BATCH_MAX one-step events with tips (ian_edit_plan.h); d_stab never has less
constexpr int SESS_MAX_CAPACITY = 1 << 20;
size_t sess_src_bytes(int scale) { return 3 * (size_t)(64 * scale) * (size_t)(64 * scale); }

enum SessGroup { SESS_BASE, SESS_HIRES, SESS_LOCAL, SESS_HISTORY, SESS_TIPS };
using SessionArrays = ian_handle::SessionState::SessionArrays;
struct SessColumn {
  size_t at;                                  // offsetof(SessionArrays, pool.member / rings.member): both structs go to kernels by value
  size_t (*row_bytes)(const SessionArrays&);  // bytes per session; 0: this pool does not have the column
  SessGroup group;
  bool zero;                                  // rows that were not copied from an old pool start at zero
  int field;                                  // the ian_session_field that reads it; -1: none
};
#define SESS_COL(member, bytes, group, zero, field)                                                            \
  {offsetof(SessionArrays, member), [](const SessionArrays& A) -> size_t {                                     \
     const SessionPool& P = A.pool; const SessionRings& R = A.rings; (void)P; (void)R; return bytes; }, group, zero, field}
const SessColumn SESS_COLUMNS[] = {
    SESS_COL(pool.gim, SESS_IMG, SESS_BASE, false, IAN_SESSION_GIM),
    SESS_COL(pool.im, SESS_IMG, SESS_BASE, false, IAN_SESSION_IM),
    SESS_COL(pool.recon, SESS_IMG, SESS_BASE, false, IAN_SESSION_RECON),
    SESS_COL(pool.error, SESS_IMG * sizeof(float), SESS_BASE, false, IAN_SESSION_ERROR),
    SESS_COL(pool.z, (size_t)P.zl * sizeof(float), SESS_BASE, false, IAN_SESSION_Z),
    SESS_COL(pool.mode, sizeof(int), SESS_BASE, false, IAN_SESSION_MODE),
    SESS_COL(pool.src, sess_src_bytes(P.scale), SESS_HIRES, false, IAN_SESSION_SOURCE),
    SESS_COL(pool.field, SESS_IMG * sizeof(float), SESS_HIRES, true, IAN_SESSION_FIELD),   // zero: a session opened before the reservation
    SESS_COL(pool.kind, sizeof(int), SESS_HIRES, true, IAN_SESSION_FIELD_KIND),            // reads as "nothing edited"
    SESS_COL(pool.umask, 64 * 64 * sizeof(double), SESS_LOCAL, true, IAN_SESSION_UMASK),
    SESS_COL(pool.local, sizeof(int), SESS_LOCAL, true, IAN_SESSION_LOCAL),
    // the rings: no zero fill, a slot is never read before it was written.  After umask: hist_umask exists where umask does.
    SESS_COL(rings.hist_z, (size_t)(R.depth + 1) * P.zl * sizeof(float), SESS_HISTORY, false, -1),
    SESS_COL(rings.hist_umask, P.umask ? (size_t)(R.depth + 1) * 64 * 64 * sizeof(double) : 0, SESS_HISTORY, false, -1),
};
#undef SESS_COL
using SessionScratch = ian_handle::SessionScratch;
struct SessScratchBuf {
  size_t at;      // offsetof(SessionScratch, member)
  size_t bytes;   // allocated with its group; 0: by the call that first needs it
  SessGroup group;
};
const SessScratchBuf SESS_SCRATCH[] = {
    {offsetof(SessionScratch, d_tab), (size_t)BATCH_MAX * 7 * sizeof(int32_t), SESS_BASE},
    {offsetof(SessionScratch, d_photo), 0, SESS_BASE},
    {offsetof(SessionScratch, d_shown), (size_t)BATCH_MAX * SESS_IMG, SESS_BASE},
    {offsetof(SessionScratch, d_rtab), 0, SESS_BASE},
    {offsetof(SessionScratch, d_stage), 0, SESS_BASE},
    {offsetof(SessionScratch, d_fit), 0, SESS_BASE},
    {offsetof(SessionScratch, d_fit_loss), 0, SESS_BASE},
    {offsetof(SessionScratch, d_stab), EDIT_TABLE_FLOOR * sizeof(int32_t), SESS_BASE},   // grown on demand beyond that (stab_cap)
    {offsetof(SessionScratch, d_tanh), 256 * sizeof(float), SESS_BASE},   // last of its group: a failed build never leaves it without its upload
    {offsetof(SessionScratch, d_views), (size_t)BATCH_MAX * 3 * sizeof(int32_t), SESS_HIRES},
    {offsetof(SessionScratch, d_out), 0, SESS_HIRES},
    {offsetof(SessionScratch, d_guide), 0, SESS_HIRES},   // by ian_sessions_reserve_guide; goes with its group
    {offsetof(SessionScratch, d_falloff), 64 * sizeof(double), SESS_LOCAL},
    {offsetof(SessionScratch, d_ltab), (size_t)BATCH_MAX * 2 * sizeof(int32_t), SESS_LOCAL},
    {offsetof(SessionScratch, d_htab), (size_t)BATCH_MAX * 3 * sizeof(int32_t), SESS_HISTORY},
    {offsetof(SessionScratch, d_tips), 0, SESS_TIPS},   // by ian_sessions_reserve_tips, at its count
    {offsetof(SessionScratch, d_tip_shape), 0, SESS_TIPS},   // with d_tips
};

// the pointer member at byte `at` of a SessionArrays / SessionScratch (members of several pointer types: copied, not aliased)
void* slot_get(const void* base, size_t at) {
  void* p;
  memcpy(&p, (const char*)base + at, sizeof p);
  return p;
}
void slot_set(void* base, size_t at, void* p) { memcpy((char*)base + at, &p, sizeof p); }

// canvases (ian_rt_canvas.inc, included after this file): what the session calls need of them.  All of it is a no-op in a pool without
// the canvas reservation.
void canvases_free(ian_handle* h);                                  // the arrays, the table, every placement
int canvases_pool_resized(ian_handle* h);                           // ian_sessions_reserve: the placements of ids that left the pool go
bool canvas_is_placed(const ian_handle* h, int id);
void canvas_unplace(ian_handle* h, int id);                         // host side; the table's upload follows with canvas_table_flush
int canvas_table_flush(ian_handle* h, hipStream_t st);
int canvas_window_check(ian_handle* h, const char* fn, int n, const ian_canvas_window* w, int vw, int vh, const uint8_t* out, int zoom = 1);
int canvas_compose_enqueue(ian_handle* h, int n, const ian_canvas_window* w, int vw, int vh, unsigned char* d_out, hipStream_t st,
                           int zoom = 1);

bool sess_has(const SessionArrays& P, SessGroup g) {
  for (const SessColumn& c : SESS_COLUMNS)
    if (c.group == g) return slot_get(&P, c.at) != nullptr;
  return false;
}
size_t sess_row_bytes(const SessionArrays& P, unsigned groups) {
  size_t sum = 0;
  for (const SessColumn& c : SESS_COLUMNS)
    if (groups >> c.group & 1) sum += c.row_bytes(P);
  return sum;
}
// The body of a saved session (ian_session_save / _load, DESIGN.md 4.6): every column the pool has, in table order, each padded to 16
// bytes.  A column of the history group is a ring of depth + 1 slots, the column that IAN_SESSION_SOURCE reads follows the session's
// source bit; nothing else about a column matters here.  -> false: a body beyond 2 GB (the kernels count bytes in 32 bits).
bool sess_record_cols(const SessionArrays& P, SessionRecordCols& T) {
  static_assert(sizeof(SESS_COLUMNS) / sizeof(SESS_COLUMNS[0]) <= SESS_REC_MAX_COLS, "SessionRecordCols holds every column");
  memset(&T, 0, sizeof T);
  size_t off = 0;
  for (const SessColumn& c : SESS_COLUMNS) {
    const size_t row = slot_get(&P, c.at) ? c.row_bytes(P) : 0;
    if (!row) continue;
    const bool ring = c.group == SESS_HISTORY, in_rings = c.at >= offsetof(SessionArrays, rings);
    SessionRecordCol& r = T.col[T.ncols++];
    r.off = (unsigned)off;
    r.slots = ring ? (unsigned)P.rings.depth + 1 : 1;
    r.unit = (unsigned)(row / r.slots);
    r.member = (unsigned short)(c.at - (in_rings ? offsetof(SessionArrays, rings) : offsetof(SessionArrays, pool)));
    r.in_rings = in_rings;
    r.rule = ring ? SESS_REC_RING : (c.field == IAN_SESSION_SOURCE ? SESS_REC_SOURCE : SESS_REC_PLAIN);
    off += session_record_pad(row);
    if (off > 0x7fffffffu) return false;
  }
  T.body_bytes = (unsigned)off;
  return true;
}
// every column of `groups` that N lacks: rows for `capacity` sessions, the first `keep` copied from O, the others zero where the
// column asks for it; the zeros are there before any stream reads them
hipError_t sess_build(SessionArrays& N, const SessionArrays& O, unsigned groups, size_t capacity, size_t keep) {
  bool zeroed = false;
  for (const SessColumn& c : SESS_COLUMNS) {
    if (!(groups >> c.group & 1) || slot_get(&N, c.at)) continue;
    const size_t row = c.row_bytes(N);
    if (!row) continue;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, capacity * row);
    if (e != hipSuccess) return e;
    slot_set(&N, c.at, p);
    if (keep) e = hipMemcpy(p, slot_get(&O, c.at), keep * row, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && c.zero && capacity > keep) {
      e = hipMemset((char*)p + keep * row, 0, (capacity - keep) * row);
      zeroed = true;
    }
    if (e != hipSuccess) return e;
  }
  return zeroed ? hipDeviceSynchronize() : hipSuccess;
}
// frees the columns of `groups` that A holds and B does not
void sess_drop(SessionArrays& A, const SessionArrays& B, unsigned groups = ~0u) {
  for (const SessColumn& c : SESS_COLUMNS) {
    void* p = slot_get(&A, c.at);
    if (!(groups >> c.group & 1) || !p || p == slot_get(&B, c.at)) continue;
    (void)hipFree(p);
    slot_set(&A, c.at, nullptr);
  }
}
// a failed build: the half-built pool N goes, the handle's pool stays as it was
int sess_build_failed(ian_handle* h, const char* fn, hipError_t e, SessionArrays& N, unsigned groups, int capacity) {
  sess_drop(N, h->sess.arr);
  (void)hipGetLastError();
  return fail(h, -2, "%s: %s for %d sessions of %zu bytes", fn, hipGetErrorString(e), capacity, sess_row_bytes(N, groups));
}
hipError_t scratch_build(SessionScratch& S, SessGroup g) {
  for (const SessScratchBuf& b : SESS_SCRATCH) {
    if (b.group != g || !b.bytes || slot_get(&S, b.at)) continue;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, b.bytes);
    if (e != hipSuccess) return e;
    slot_set(&S, b.at, p);
  }
  return hipSuccess;
}
void scratch_free(SessionScratch& S, SessGroup g) {
  for (const SessScratchBuf& b : SESS_SCRATCH) {
    if (b.group != g) continue;
    if (void* p = slot_get(&S, b.at)) (void)hipFree(p);
    slot_set(&S, b.at, nullptr);
  }
}
// everything one reservation owns: its columns, its scratch, and what the host keeps about them
void sess_free_group(decltype(ian_handle::sess)& S, SessGroup g) {
  sess_drop(S.arr, SessionArrays{}, 1u << g);
  scratch_free(S, g);
  if (g == SESS_HIRES) {
    S.arr.pool.scale = 0;
    S.out_cap = 0;
    std::fill(S.has_src.begin(), S.has_src.end(), 0);
  } else if (g == SESS_LOCAL) {   // the table too: a later reservation starts from nothing
    S.falloff_set = false;
    std::fill(S.local_flags.begin(), S.local_flags.end(), 0);
  } else if (g == SESS_HISTORY) {
    S.arr.rings.depth = 0;
    std::fill(S.hist.begin(), S.hist.end(), SessionHistory{});
  } else if (g == SESS_TIPS) {
    S.tip_count = 0;
    S.tip_wh.clear();
    S.tip_footprint = false;
  } else {
    S.arr.pool.zl = 0;
    S.capacity = 0;
    S.stage_cap = 0;
    S.stab_cap = 0;
    S.opened.clear(); S.version.clear(); S.has_src.clear(); S.local_flags.clear(); S.hist.clear();
    S.res_valid = false;
  }
}
// ian_sessions_reserve(0) and ian_destroy: w, radius (ian_sessions_set_blend) and dampen_thresh stay, the pixel format does not
void sessions_free(ian_handle* h) {
  h->sess.pixels = PIXELS_PLANAR;
  canvases_free(h);
  for (SessGroup g : {SESS_TIPS, SESS_HISTORY, SESS_LOCAL, SESS_HIRES, SESS_BASE}) sess_free_group(h->sess, g);
}
// the refusal of a call that needs the pool (SESS_BASE) or one of the other reservations
int session_need(ian_handle* h, const char* fn, SessGroup g) {
  const auto& S = h->sess;
  if (g == SESS_BASE) return S.capacity > 0 ? 0 : fail(h, -6, "%s: no session pool (call ian_sessions_reserve first)", fn);
  if (g == SESS_TIPS) return S.tip_count > 0 ? 0 : fail(h, -6, "%s: no tip reservation (call ian_sessions_reserve_tips first)", fn);
  if (sess_has(S.arr, g)) return 0;
  if (g == SESS_HIRES) return fail(h, -6, "%s: no full-resolution reservation (call ian_sessions_reserve_hires first)", fn);
  if (g == SESS_HISTORY) return fail(h, -6, "%s: no history reservation (call ian_sessions_reserve_history first)", fn);
  return fail(h, -6, "%s: no local reservation (call ian_sessions_reserve_local first)", fn);
}

// np.asarray([to_tanh(IM)], dtype=np.float32) per uint8 level: float64 2.0*(v/255.0)-1.0, then one rounding to float32
void session_tanh_table(float* out) {
  for (int v = 0; v < 256; ++v) {
    volatile double q = (double)v / 255.0;
    volatile double t = 2.0 * q;
    out[v] = (float)(t - 1.0);
  }
}

// a finalized handle, and the 3x64x64 image on both ends (the pool rows, the blend and the open kernels are written for it)
int session_ready(ian_handle* h, const char* fn) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  const Slot& os = h->slots[h->desc.out_slot];
  const Slot& xs = h->slots[h->desc.x_slot];
  if (os.h != 64 || os.w != 64 || os.c != 3 || !os.nchw || xs.h != 64 || xs.w != 64 || xs.c != 3 || !xs.nchw)
    return fail(h, -7, "%s: edit sessions need a model with a 3x64x64 image", fn);
  return 0;
}

int sessions_reserve(ian_handle* h, int capacity) {
  const char* fn = "ian_sessions_reserve";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  if (capacity < 0 || capacity > SESS_MAX_CAPACITY) return fail(h, -7, "%s: capacity %d outside 0..%d", fn, capacity, SESS_MAX_CAPACITY);
  auto& S = h->sess;
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that move
  h->last_pending = false;
  S.res_valid = false;
  if (capacity == 0) {
    sessions_free(h);
    return 0;
  }
  if (capacity != S.capacity) {   // a new pool with the groups the old one has: every column follows the capacity
    SessionArrays N = S.arr;
    N.pool.zl = h->desc.num_latents;
    unsigned groups = 1u << SESS_BASE;
    for (SessGroup g : {SESS_HIRES, SESS_LOCAL, SESS_HISTORY})
      if (sess_has(S.arr, g)) groups |= 1u << g;
    for (const SessColumn& c : SESS_COLUMNS) slot_set(&N, c.at, nullptr);
    const size_t c = (size_t)capacity;
    hipError_t e = sess_build(N, S.arr, groups, c, (size_t)std::min(capacity, S.capacity));
    if (e != hipSuccess) return sess_build_failed(h, fn, e, N, groups, capacity);
    sess_drop(S.arr, N);
    S.arr = N;
    S.capacity = capacity;
    S.opened.resize(c, 0);
    S.version.resize(c, 0);
    S.has_src.resize(c, 0);
    S.local_flags.resize(c, 0);
    S.hist.resize(c);   // the surviving ids keep their histories: their rings moved with the rest
    if ((rc = canvases_pool_resized(h))) return rc;
  }
  const bool had_table = S.d_tanh != nullptr;   // the table is uploaded once, when its buffer is new
  HIPCHK(h, scratch_build(S, SESS_BASE));
  S.stab_cap = std::max(S.stab_cap, EDIT_TABLE_FLOOR);   // a d_stab this call built has the floor, one a stroke grew keeps its size
  if (!had_table) {
    float tab[256];
    session_tanh_table(tab);
    HIPCHK(h, hipMemcpy(S.d_tanh, tab, sizeof tab, hipMemcpyHostToDevice));
  }
  return 0;
}

// ian_sessions_reserve_hires / _local: what N lacks of group g, and the group's scratch, at the pool's capacity, then N becomes the pool
int sess_add_group(ian_handle* h, const char* fn, SessionArrays& N, SessGroup g) {
  auto& S = h->sess;
  const bool had = sess_has(S.arr, g);
  hipError_t e = sess_build(N, S.arr, 1u << g, (size_t)S.capacity, 0);
  if (e == hipSuccess) e = scratch_build(S, g);
  if (e != hipSuccess) {
    if (!had) scratch_free(S, g);
    return sess_build_failed(h, fn, e, N, 1u << g, S.capacity);
  }
  sess_drop(S.arr, N);
  S.arr = N;
  return 0;
}

int sessions_reserve_hires(ian_handle* h, int scale) {
  const char* fn = "ian_sessions_reserve_hires";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (scale < 0 || scale > 16) return fail(h, -7, "%s: scale %d outside 0..16", fn, scale);
  if (scale == 0 && S.canv.pix)   // the placements' FIELD and FIELD_KIND would go
    return fail(h, -6, "%s: canvases are reserved: free them first (ian_sessions_reserve_canvas(0))", fn);
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that are freed
  h->last_pending = false;
  if (scale == S.arr.pool.scale) return 0;
  if (scale == 0) {
    sess_free_group(S, SESS_HIRES);
    return 0;
  }
  // a new scale: a new SRC array (no photo survives, its size differs); FIELD and FIELD_KIND are built once
  SessionArrays N = S.arr;
  N.pool.scale = scale;
  N.pool.src = nullptr;
  if ((rc = sess_add_group(h, fn, N, SESS_HIRES))) return rc;
  std::fill(S.has_src.begin(), S.has_src.end(), 0);
  return 0;
}

// A table of range weights (ian_sessions_reserve_guide; ian_sessions_reserve_edges in ian_rt_canvas.inc): count 766 checks the host
// table, synchronises the device and uploads it to slot, allocating the buffer the first time; (any, 0) frees it.  A refusal leaves
// slot and its table as they were.
int guide_table_set(ian_handle* h, const char* fn, float*& slot, const float* table, int count) {
  if (count != 0 && count != SESSION_GUIDE_TABLE_LEN) return fail(h, -7, "%s: count %d (0 frees, %d sets the table)", fn, count, SESSION_GUIDE_TABLE_LEN);
  if (count) {
    if (!table) return fail(h, -7, "%s: null table", fn);
    if (is_device_ptr(table)) return fail(h, -7, "%s: the table must be a host array", fn);
    for (int d = 0; d < count; ++d)
      if (!std::isfinite(table[d]) || !(table[d] > 0.0f)) return fail(h, -7, "%s: table[%d] = %g is not a finite positive weight", fn, d, (double)table[d]);
  }
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read the table that is replaced or freed
  h->last_pending = false;
  if (!count) {
    if (slot) (void)hipFree(slot);
    slot = nullptr;
    return 0;
  }
  float* d = slot;
  if (!d) {
    hipError_t e = hipMalloc((void**)&d, SESSION_GUIDE_TABLE_LEN * sizeof(float));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, -2, "%s: %s for the table of %zu bytes", fn, hipGetErrorString(e), SESSION_GUIDE_TABLE_LEN * sizeof(float));
    }
  }
  hipError_t e = hipMemcpy(d, table, SESSION_GUIDE_TABLE_LEN * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {   // a new buffer goes; an old one keeps the table it had or has half of the new one: the error is fatal either way
    if (!slot) (void)hipFree(d);
    HIPCHK(h, e);
  }
  slot = d;
  return 0;
}
// 1 and the table of slot in table_out (host; may be null), or 0 without one
int guide_table_get(ian_handle* h, const char* fn, const float* slot, float* table_out) {
  if (!slot) return 0;
  if (table_out) {
    if (is_device_ptr(table_out)) return fail(h, -7, "%s: table_out must be a host array", fn);
    HIPCHK(h, hipMemcpy(table_out, slot, SESSION_GUIDE_TABLE_LEN * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 1;
}

// The guide is a setting of the pool, not session state: one device table beside the pool (S.d_guide, freed with the hires group), and
// while it exists session_render_enqueue launches the guided kernel.  Records, history and ian_session_read know nothing of it.
int sessions_reserve_guide(ian_handle* h, const float* table, int count) {
  const char* fn = "ian_sessions_reserve_guide";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_HIRES))) return rc;
  if (S.canv.pix)   // canvas_compose_kernel promises ian_session_render's bytes with the plain bilinear tap
    return fail(h, -6, "%s: canvases are reserved: free them first (ian_sessions_reserve_canvas(0))", fn);
  return guide_table_set(h, fn, S.d_guide, table, count);
}
int sessions_guide(ian_handle* h, float* table_out) {
  const char* fn = "ian_sessions_guide";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_HIRES))) return rc;
  return guide_table_get(h, fn, S.d_guide, table_out);
}

// The pixel format of `out` in every window call (DESIGN.md 4.17) is a setting of the pool like the guide, and host state only: the
// enqueue of the next call reads it.  Records, history and ian_session_read know nothing of it.
int sessions_set_pixels(ian_handle* h, int format) {
  const char* fn = "ian_sessions_set_pixels";
  if (int rc = session_need(h, fn, SESS_BASE)) return rc;
  if (format < PIXELS_PLANAR || format > PIXELS_BGRA)
    return fail(h, -7, "%s: format %d outside 0..3 (0 planar, 1 rgb, 2 rgba, 3 bgra)", fn, format);
  h->sess.pixels = format;
  return 0;
}
int sessions_pixels(ian_handle* h) {
  if (int rc = session_need(h, "ian_sessions_pixels", SESS_BASE)) return rc;
  return h->sess.pixels;
}

int sessions_set_blend(ian_handle* h, const double* gauss_half, int radius) {
  if (!h) return -1;
  if (!gauss_half) return fail(h, -1, "null pointer passed to ian_sessions_set_blend");
  if (radius < 0 || radius > 7) return fail(h, -7, "ian_sessions_set_blend: radius %d outside 0..7", radius);
  if (is_device_ptr(gauss_half)) return fail(h, -7, "ian_sessions_set_blend: gauss_half must be a host array");
  for (int i = 0; i < 8; ++i) h->sess.w[i] = i <= radius ? gauss_half[i] : 0.0;
  h->sess.radius = radius;
  return 0;
}

int sessions_reserve_local(ian_handle* h, int on) {
  const char* fn = "ian_sessions_reserve_local";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (on != 0 && on != 1) return fail(h, -7, "%s: on = %d (0 frees, 1 allocates)", fn, on);
  if (sess_has(S.arr, SESS_HISTORY) && (on != 0) != sess_has(S.arr, SESS_LOCAL))   // the saved states would lose or lack their UMASK rows
    return fail(h, -6, "%s: the pool has a history reservation made %s the local one: free the history first (ian_sessions_reserve_history(0))",
                fn, on ? "without" : "with");
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that are freed
  h->last_pending = false;
  if (!on) {
    sess_free_group(S, SESS_LOCAL);
    return 0;
  }
  if (sess_has(S.arr, SESS_LOCAL)) return 0;
  SessionArrays N = S.arr;
  if ((rc = sess_add_group(h, fn, N, SESS_LOCAL))) return rc;
  S.falloff_set = false;
  S.local_flags.assign((size_t)S.capacity, 0);
  return 0;
}

int sessions_set_local(ian_handle* h, const double* falloff64, double dampen_thresh) {
  const char* fn = "ian_sessions_set_local";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  if (!falloff64) return fail(h, -1, "null pointer passed to %s", fn);
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_LOCAL))) return rc;
  if (is_device_ptr(falloff64)) return fail(h, -7, "%s: falloff64 must be a host array", fn);
  if (!(falloff64[0] == 1.0)) return fail(h, -7, "%s: falloff64[0] = %g, not 1.0 (the footprint is 1 inside the brush rectangle)", fn, falloff64[0]);
  for (int i = 0; i < 64; ++i)
    if (!(falloff64[i] >= 0.0 && falloff64[i] <= 1.0)) return fail(h, -7, "%s: falloff64[%d] = %g outside [0,1]", fn, i, falloff64[i]);
  if (!std::isfinite(dampen_thresh)) return fail(h, -7, "%s: dampen_thresh %g is not finite", fn, dampen_thresh);
  HIPCHK(h, hipDeviceSynchronize());   // a pending blend may still read the old table
  h->last_pending = false;
  HIPCHK(h, hipMemcpy(S.d_falloff, falloff64, 64 * sizeof(double), hipMemcpyHostToDevice));
  S.dampen_thresh = dampen_thresh;
  S.falloff_set = true;
  return 0;
}

// ian_session_brush / ian_session_set_latent(as_sample = 0) on a pool with the local reservation: a session whose LOCAL flags are not
// 0 needs the table.  Checked with everything else, before anything is enqueued.
int session_local_check(ian_handle* h, const char* fn, int n, const int32_t* ids, int stride) {
  auto& S = h->sess;
  if (!S.arr.pool.umask || S.falloff_set) return 0;
  for (int i = 0; i < n; ++i) {
    const int id = ids[(size_t)i * stride];
    if (S.local_flags[id])
      return fail(h, -6, "%s: item %d: session %d has local flags %d, but the falloff table is not set (call ian_sessions_set_local first)",
                  fn, i, id, (int)S.local_flags[id]);
  }
  return 0;
}

// A call that only reads or writes pool rows (ian_session_local, _render, _read): the decoder's activations and the residency of
// ian_session_brush survive it.  Enter: the stream hand-over; leave: a device result leaves the stream pending, a host result is
// synchronised.
int session_rows_enter(ian_handle* h, hipStream_t st) {
  if (h->last_pending && h->last_stream != st) HIPCHK(h, hipStreamSynchronize(h->last_stream));
  return 0;
}
int session_rows_leave(ian_handle* h, hipStream_t st, bool device_result) {
  if (device_result) {
    h->last_stream = st;
    h->last_pending = true;
  } else {
    HIPCHK(h, hipStreamSynchronize(st));
    if (h->last_stream == st) h->last_pending = false;
  }
  return 0;
}

// one session id: in the pool and, where the call needs it, opened; item < 0: the call names one session only
int session_check_one(ian_handle* h, const char* fn, int item, int id, bool need_opened) {
  const bool outside = id < 0 || id >= h->sess.capacity;
  if (!outside && (!need_opened || h->sess.opened[id])) return 0;   // the common case formats nothing
  char where[32] = "";
  if (item >= 0) snprintf(where, sizeof where, "item %d: ", item);
  if (outside) return fail(h, -7, "%s: %ssession %d outside the pool (capacity %d)", fn, where, id, h->sess.capacity);
  return fail(h, -7, "%s: %ssession %d has not been opened", fn, where, id);
}
// what every session call checks first: the model, the pool, n; then per item its id (ids[i * stride]).  Nothing is enqueued or
// written before all of it passed.
int session_check(ian_handle* h, const char* fn, int n, const int32_t* ids, int stride, bool need_opened, bool need_blend) {
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (n < 1 || n > BATCH_MAX) return fail(h, -7, "%s: n = %d outside 1..%d", fn, n, BATCH_MAX);
  if (!ids) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(ids)) return fail(h, -7, "%s: the session ids / events must be a host array", fn);
  if (need_blend && S.radius < 0) return fail(h, -6, "%s: the photo blend's Gaussian is not set (call ian_sessions_set_blend first)", fn);
  std::map<int, int> first;
  for (int i = 0; i < n; ++i) {
    const int id = ids[(size_t)i * stride];
    if ((rc = session_check_one(h, fn, i, id, need_opened))) return rc;
    auto ins = first.emplace(id, i);
    if (!ins.second) return fail(h, -7, "%s: item %d: session %d already appears as item %d of this call", fn, i, id, ins.first->second);
  }
  return 0;
}

// The undo history's side of every other call, host only, where the call bumps S.version or has rewritten what a saved state is
// measured against: `clear` for a call that rewrites RECON / ERROR / GIM or zeroes UMASK (the saved states no longer belong to the
// picture), otherwise `edited` (the latent was written: the redo tail goes).
void session_history_note(decltype(ian_handle::sess)& S, int id, bool clear) {
  if (!S.arr.rings.depth) return;
  if (clear)
    session_history_clear(S.hist[id]);
  else
    session_history_edited(S.hist[id], S.arr.rings.depth);
}
// a call wrote session id's latent: a new version (what the residency of ian_session_brush is keyed by) and the history's note of it
void session_latent_written(decltype(ian_handle::sess)& S, int id, bool clear) {
  ++S.version[id];
  session_history_note(S, id, clear);
}

int session_local(ian_handle* h, int n, const int32_t* ids, const int32_t* flags, void* stream) {
  const char* fn = "ian_session_local";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if (S.capacity > 0 && (rc = session_need(h, fn, SESS_LOCAL))) return rc;
  if ((rc = session_check(h, fn, n, ids, 1, true, false))) return rc;
  if (!flags) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(flags)) return fail(h, -7, "%s: the flags must be a host array", fn);
  for (int i = 0; i < n; ++i)
    if (flags[i] < 0 || flags[i] > 3) return fail(h, -7, "%s: item %d: flags %d outside 0..3 (bit 0 = local, bit 1 = dampen)", fn, i, flags[i]);
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  S.ltab_shadow.resize((size_t)2 * n);
  memcpy(S.ltab_shadow.data(), ids, (size_t)n * sizeof(int32_t));
  memcpy(S.ltab_shadow.data() + n, flags, (size_t)n * sizeof(int32_t));
  HIPCHK(h, hipMemcpyAsync(S.d_ltab, S.ltab_shadow.data(), (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_session_local_set(S.arr.pool, S.d_ltab, S.d_ltab + n, n, st));
  for (int i = 0; i < n; ++i) {
    S.local_flags[ids[i]] = (char)flags[i];
    session_history_note(S, ids[i], true);
  }
  return session_rows_leave(h, st, true);
}

// start of the enqueueing part of a session call: stream hand-over, the other paths' caches (as batch_common)
void session_enter(ian_handle* h, hipStream_t st) {
  enter_stream(h, st);
  h->dec_cache_valid = false;   // the batch-1 activations are overwritten
  h->pin_img_valid = false;
}

int session_upload_ids(ian_handle* h, int n, const int32_t* ids, hipStream_t st) {
  auto& S = h->sess;
  S.tab_shadow.assign(ids, ids + n);
  HIPCHK(h, hipMemcpyAsync(S.d_tab, S.tab_shadow.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  return 0;
}

// Where a result array of a call goes.  dev: what the kernels write -- the caller's array when it is device memory, else a staging
// buffer; nullptr: the call has no such result.  host: the copy down that the end of the call owes; nullptr: none.
struct ResultTarget { unsigned char* dev; uint8_t* host; };
// the canvas images: staged in d_shown; need_dev: the kernel (the blend) writes them whether the caller wants them or not
ResultTarget shown_target(ian_handle* h, uint8_t* shown, bool need_dev) {
  if (shown && is_device_ptr(shown)) return {shown, nullptr};
  return {shown || need_dev ? h->sess.d_shown : nullptr, shown};
}
// end of a call: the canvas images (and, for ian_session_brush_view / ian_canvas_brush, the rendered windows with their byte count)
// to the caller; one synchronisation when host memory was read or written
int session_finish(ian_handle* h, int n, const ResultTarget& shown, bool host_in, hipStream_t st, const ResultTarget& win = {},
                   size_t win_bytes = 0) {
  if (shown.host) HIPCHK(h, hipMemcpyAsync(shown.host, shown.dev, (size_t)n * SESS_IMG, hipMemcpyDeviceToHost, st));
  if (win.host) HIPCHK(h, hipMemcpyAsync(win.host, win.dev, win_bytes, hipMemcpyDeviceToHost, st));
  if (shown.host || host_in || win.host) {
    HIPCHK(h, hipStreamSynchronize(st));
    h->last_pending = false;
  }
  return 0;
}

// what ian_session_render and ian_session_brush_view check about the windows, before anything is enqueued: the reservation, n, and
// per item the session (in the pool, opened, holding a photo; ev given: the session of event i) and the window.  The same session may
// appear several times (tiles of one picture).  zoom: vw x vh is the size of a view at 1/zoom (DESIGN.md 4.14), whose source window
// (x, y, zoom * vw, zoom * vh) is the one that must lie inside the picture; 1: the window itself.
constexpr int ZOOM_LIMIT = 16;
int zoom_check(ian_handle* h, const char* fn, int zoom) {
  return zoom < 1 || zoom > ZOOM_LIMIT ? fail(h, -7, "%s: zoom %d outside 1..%d", fn, zoom, ZOOM_LIMIT) : 0;
}
// "x > limit - zoom * size" of one axis without overflow
bool zoom_outside(int at, int size, int zoom, int limit) { return at < 0 || (long long)at + (long long)zoom * size > limit; }
int session_view_check(ian_handle* h, const char* fn, int n, const ian_session_view* views, int vw, int vh, const uint8_t* out,
                       const ian_session_event* ev, int zoom = 1) {
  static_assert(sizeof(ian_session_view) == 3 * sizeof(int32_t), "ian_session_view is 3 words");
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_HIRES)) || (rc = zoom_check(h, fn, zoom))) return rc;
  if (n < 1 || n > BATCH_MAX) return fail(h, -7, "%s: n = %d outside 1..%d", fn, n, BATCH_MAX);
  if (!views || !out) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(views)) return fail(h, -7, "%s: the views must be a host array", fn);
  const int Sz = 64 * S.arr.pool.scale;
  if (vw < 1 || vh < 1) return fail(h, -7, "%s: window %d x %d: both sizes must be at least 1", fn, vw, vh);
  if (vw & 3) return fail(h, -7, "%s: window width %d is not a multiple of 4", fn, vw);
  for (int i = 0; i < n; ++i) {
    const ian_session_view& v = views[i];
    if ((rc = session_check_one(h, fn, i, v.session, false))) return rc;
    if (ev && ev[i].session != v.session)
      return fail(h, -7, "%s: item %d: the view names session %d, the event session %d", fn, i, v.session, ev[i].session);
    if (!S.opened[v.session]) return fail(h, -7, "%s: item %d: session %d has not been opened", fn, i, v.session);
    if (!S.has_src[v.session])
      return fail(h, -7, "%s: item %d: session %d has no full-resolution source (open it with ian_session_open_hires)", fn, i, v.session);
    if (v.x & 3) return fail(h, -7, "%s: item %d: window x %d is not a multiple of 4", fn, i, v.x);
    if (zoom == 1 && (v.x < 0 || v.y < 0 || v.x > Sz - vw || v.y > Sz - vh))
      return fail(h, -7, "%s: item %d: window (%d,%d) + %d x %d outside the %d x %d picture", fn, i, v.x, v.y, vw, vh, Sz, Sz);
    if (zoom_outside(v.x, vw, zoom, Sz) || zoom_outside(v.y, vh, zoom, Sz))
      return fail(h, -7, "%s: item %d: window (%d,%d) + %d x %d at zoom %d outside the %d x %d picture", fn, i, v.x, v.y, vw, vh, zoom, Sz, Sz);
  }
  return 0;
}

// the windows of n views into d_out (device, u8[n,3,vh,vw]; packed under S.pixels), or, d_out == nullptr, the whole picture over each
// session's own SRC, planar whatever the pool's format.
// zoom > 1: the views at 1/zoom.  S.d_guide (ian_sessions_reserve_guide): the field's taps weighted by the photo; nullptr: plain
int session_render_enqueue(ian_handle* h, int n, const ian_session_view* views, int vw, int vh, unsigned char* d_out, hipStream_t st,
                           int zoom = 1) {
  auto& S = h->sess;
  S.views_shadow.resize((size_t)3 * n);
  memcpy(S.views_shadow.data(), views, (size_t)n * sizeof(ian_session_view));
  HIPCHK(h, hipMemcpyAsync(S.d_views, S.views_shadow.data(), (size_t)n * sizeof(ian_session_view), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_session_render(S.arr.pool, S.d_guide, S.d_views, vw, vh, zoom, d_out, n, d_out ? S.pixels : PIXELS_PLANAR, st));
  return 0;
}

// the device buffer a call renders into: the caller's, or the staging buffer grown to the call's size
int session_render_target(ian_handle* h, uint8_t* out, size_t bytes, ResultTarget* t) {
  auto& S = h->sess;
  const bool dev = is_device_ptr(out);
  int rc = dev ? 0 : grow_dev(h, &S.d_out, &S.out_cap, bytes);
  *t = dev ? ResultTarget{out, nullptr} : ResultTarget{S.d_out, out};
  return rc;
}

// A call that renders n windows and nothing else (ian_session_render, ian_canvas_compose), after its checks: the render target,
// session_rows_enter, the caller's enqueue(d_out, st), the copy down for a host array, session_rows_leave.
template <typename Enqueue>
int window_call(ian_handle* h, int n, int vw, int vh, uint8_t* out, void* stream, Enqueue enqueue) {
  const size_t bytes = (size_t)n * pixels_bpp(h->sess.pixels) * (size_t)vh * (size_t)vw;
  ResultTarget t = {};
  int rc = session_render_target(h, out, bytes, &t);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  if ((rc = enqueue(t.dev, st))) return rc;
  if (t.host) HIPCHK(h, hipMemcpyAsync(t.host, t.dev, bytes, hipMemcpyDeviceToHost, st));
  return session_rows_leave(h, st, !t.host);
}

int session_open_finish(ian_handle* h, int n, const int32_t* ids, uint8_t* shown, bool host_in, int has_src, hipStream_t st);
int session_open(ian_handle* h, int n, const int32_t* ids, const uint8_t* photos, int source, uint8_t* shown, void* stream, bool hires) {
  const char* fn = hires ? "ian_session_open_hires" : "ian_session_open";
  int rc = session_check(h, fn, n, ids, 1, photos == nullptr, false);
  if (rc) return rc;
  if (!photos && source != 0 && source != 1) return fail(h, -7, "%s: source %d (0 = from GIM, 1 = GIM := IM first)", fn, source);
  auto& S = h->sess;
  if (hires && (rc = session_need(h, fn, SESS_HIRES))) return rc;
  if (hires && !photos) return fail(h, -1, "null pointer passed to %s", fn);
  for (int i = 0; !photos && source == 1 && i < n; ++i)
    if (canvas_is_placed(h, ids[i]))   // GIM := IM would bake the unfeathered 64x64 blend into the session
      return fail(h, -7, "%s: item %d: session %d is placed on a canvas: commit the canvas instead (ian_canvas_commit)", fn, i, ids[i]);
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);
  TotalTimer tt(h, st);
  if ((rc = session_upload_ids(h, n, ids, st))) return rc;
  for (int i = 0; photos && i < n; ++i) canvas_unplace(h, ids[i]);   // a new photo: the session leaves its canvas
  if (photos && (rc = canvas_table_flush(h, st))) return rc;
  const unsigned char* d_photos = photos;
  const bool host_in = photos && !is_device_ptr(photos);
  if (host_in && hires) {   // straight into the sessions' SRC rows: no staging of n * 3 * S * S bytes
    const size_t row = sess_src_bytes(S.arr.pool.scale);
    for (int i = 0; i < n; ++i)
      HIPCHK(h, hipMemcpyAsync(S.arr.pool.src + (size_t)ids[i] * row, photos + (size_t)i * row, row, hipMemcpyHostToDevice, st));
    d_photos = nullptr;
  } else if (host_in) {
    if (!S.d_photo) HIPCHK(h, hipMalloc((void**)&S.d_photo, (size_t)BATCH_MAX * SESS_IMG));
    HIPCHK(h, hipMemcpyAsync(S.d_photo, photos, (size_t)n * SESS_IMG, hipMemcpyHostToDevice, st));
    d_photos = S.d_photo;
  }
  if (!photos && source == 1 && S.arr.pool.scale > 0) {   // commit: what is displayed becomes the full-resolution photo as well
    std::vector<ian_session_view> whole;
    for (int i = 0; i < n; ++i)
      if (S.has_src[ids[i]]) whole.push_back(ian_session_view{ids[i], 0, 0});
    const int Sz = 64 * S.arr.pool.scale;
    if (!whole.empty() && (rc = session_render_enqueue(h, (int)whole.size(), whole.data(), Sz, Sz, nullptr, st))) return rc;
  }
  Slot& xs = h->slots[h->desc.x_slot];
  if ((rc = ensure_slot(h, h->desc.x_slot, n))) return rc;
  if (hires)
    HIPCHK(h, launch_session_hires_open(d_photos, S.arr.pool, S.d_tab, S.d_tanh, xs.d, n, st));
  else
    HIPCHK(h, launch_session_open_in(d_photos, S.arr.pool, S.d_tab, source, S.d_tanh, xs.d, n, st));
  return session_open_finish(h, n, ids, shown, host_in, photos ? (hires ? 1 : 0) : -1, st);
}

// Every open from here on: the input kernel has written GIM, IM and the encoder's input rows of sessions `ids` (device: S.d_tab[0..n));
// encode, decode, store, the UMASK clear, what the host keeps per session, shown down.  has_src: 1 / 0 sets the sessions' "SRC
// holds a photo" flag, -1 leaves it.
int session_open_finish(ian_handle* h, int n, const int32_t* ids, uint8_t* shown, bool host_in, int has_src, hipStream_t st) {
  auto& S = h->sess;
  int rc = 0;
  Slot& zs = h->slots[h->desc.z_slot];
  Slot& out = h->slots[h->desc.out_slot];
  h->slot_stale[h->desc.x_slot] = 0;
  // the very segments ian_encode and ian_decode_u8 run at this batch: Z and RECON are theirs bit for bit
  if ((rc = run_segment(h, IAN_SEG_ENC, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_IAF, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;
  h->slot_stale[h->desc.out_slot] = 0;
  const ResultTarget sh = shown_target(h, shown, false);
  HIPCHK(h, launch_session_store(out.d, zs.d, zs.cs, S.arr.pool, S.d_tab, 0, 0, sh.dev, n, st));
  if (S.arr.pool.umask) HIPCHK(h, launch_session_local_set(S.arr.pool, S.d_tab, nullptr, n, st));   // USER_MASK *= 0 (NPE.py:267, :337); LOCAL stays
  for (int i = 0; i < n; ++i) {
    S.opened[ids[i]] = 1;
    session_latent_written(S, ids[i], true);
    if (has_src >= 0) S.has_src[ids[i]] = (char)has_src;   // a 64x64 photo leaves nothing at full resolution to edit
  }
  return session_finish(h, n, sh, host_in, st);
}

// the blend of `ids` (device) after the decoder ran at their latents: items == nullptr is paint_latents, store != 0 a brush event
SessionBlendArgs session_blend_args(ian_handle* h, const int* ids, const int* items, unsigned char* shown, int store) {
  const auto& S = h->sess;
  const Slot& zs = h->slots[h->desc.z_slot];
  SessionBlendArgs a;
  memset(&a, 0, sizeof a);
  a.xhat = h->slots[h->desc.out_slot].d; a.zslot = zs.d; a.zs = zs.cs; a.P = S.arr.pool; a.ids = ids; a.items = items;
  a.shown = shown;
  a.store = store;
  for (int i = 0; i < 8; ++i) a.w[i] = S.w[i];
  a.radius = S.radius;
  a.falloff = S.d_falloff; a.thresh = S.dampen_thresh;
  return a;
}

int session_set_latent(ian_handle* h, int n, const int32_t* ids, const float* z, int as_sample, uint8_t* shown, void* stream) {
  const char* fn = "ian_session_set_latent";
  int rc = session_check(h, fn, n, ids, 1, true, as_sample == 0);
  if (rc) return rc;
  if (!z) return fail(h, -1, "null pointer passed to %s", fn);
  if (as_sample != 0 && as_sample != 1) return fail(h, -7, "%s: as_sample %d (0 = paint_latents, 1 = sample)", fn, as_sample);
  if (as_sample == 0 && (rc = session_local_check(h, fn, n, ids, 1))) return rc;
  auto& S = h->sess;
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);
  TotalTimer tt(h, st);
  if ((rc = session_upload_ids(h, n, ids, st))) return rc;
  const bool host_in = !is_device_ptr(z);
  Slot& zs = h->slots[h->desc.z_slot];
  Slot& out = h->slots[h->desc.out_slot];
  if ((rc = set_latent_input(h, h->desc.z_slot, z, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;   // sample_at(z) at this batch, as ian_decode / ian_decode_u8 run it
  h->slot_stale[h->desc.out_slot] = 0;
  const ResultTarget sh = shown_target(h, shown, as_sample == 0);
  if (as_sample) {
    HIPCHK(h, launch_session_store(out.d, zs.d, zs.cs, S.arr.pool, S.d_tab, 1, 1, sh.dev, n, st));
  } else {
    HIPCHK(h, launch_session_blend(session_blend_args(h, S.d_tab, nullptr, sh.dev, 0), n, st));
  }
  for (int i = 0; i < n; ++i) session_latent_written(S, ids[i], as_sample != 0);
  return session_finish(h, n, sh, host_in, st);
}

int sessions_reserve_history(ian_handle* h, int depth) {
  const char* fn = "ian_sessions_reserve_history";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (depth < 0 || depth > SESSION_HISTORY_MAX_DEPTH) return fail(h, -7, "%s: depth %d outside 0..%d", fn, depth, SESSION_HISTORY_MAX_DEPTH);
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that are freed
  h->last_pending = false;
  if (depth == S.arr.rings.depth) return 0;
  if (depth == 0) {
    sess_free_group(S, SESS_HISTORY);
    return 0;
  }
  // another depth: new rings (a slot's place depends on the depth), every history starts empty
  SessionArrays N = S.arr;
  N.rings.depth = depth;
  N.rings.hist_z = nullptr;
  N.rings.hist_umask = nullptr;
  if ((rc = sess_add_group(h, fn, N, SESS_HISTORY))) return rc;
  S.hist.assign((size_t)S.capacity, SessionHistory{});
  return 0;
}

// ian_session_mark / ian_session_undo: the reservation, then what every session call checks
int session_history_check(ian_handle* h, const char* fn, int n, const int32_t* ids, bool need_blend) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if (h->sess.capacity > 0 && (rc = session_need(h, fn, SESS_HISTORY))) return rc;
  return session_check(h, fn, n, ids, 1, true, need_blend);
}

int session_mark(ian_handle* h, int n, const int32_t* ids, void* stream) {
  const char* fn = "ian_session_mark";
  int rc = session_history_check(h, fn, n, ids, false);
  if (rc) return rc;
  auto& S = h->sess;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  std::vector<SessionHistory> next((size_t)n);   // the counters move only after the enqueue succeeded
  S.htab_shadow.resize((size_t)2 * n);
  for (int i = 0; i < n; ++i) {
    next[i] = S.hist[ids[i]];
    S.htab_shadow[i] = ids[i];
    S.htab_shadow[(size_t)n + i] = session_history_mark(next[i], S.arr.rings.depth);
  }
  HIPCHK(h, hipMemcpyAsync(S.d_htab, S.htab_shadow.data(), (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_session_history_save(S.arr.pool, S.arr.rings, S.d_htab, S.d_htab + n, n, st));
  for (int i = 0; i < n; ++i) S.hist[ids[i]] = next[i];
  return session_rows_leave(h, st, true);
}

// steps[i] > 0 undoes, < 0 redoes (nullptr: one undo each).  One submission: the slot table up, the move kernel (tip save where
// needed, the saved state into the decoder's latent slot and the UMASK row), the decoder at batch n as ian_session_set_latent runs it,
// the blend of set_latent(as_sample = 0) but stored (IM := shown := blend, FIELD the edit field; sample mode: shown = uint8(from_tanh(x)),
// FIELD := x), shown down.
int session_undo(ian_handle* h, int n, const int32_t* ids, const int32_t* steps, uint8_t* shown, void* stream) {
  const char* fn = "ian_session_undo";
  int rc = session_history_check(h, fn, n, ids, true);
  if (rc) return rc;
  if ((rc = session_local_check(h, fn, n, ids, 1))) return rc;
  if (steps && is_device_ptr(steps)) return fail(h, -7, "%s: the steps must be a host array", fn);
  auto& S = h->sess;
  for (int i = 0; i < n; ++i) {
    const int k = steps ? steps[i] : 1;
    const SessionHistory& H = S.hist[ids[i]];
    if (k == 0) return fail(h, -7, "%s: item %d: steps 0 (> 0 undoes, < 0 redoes)", fn, i);
    if (k > 0 && k > session_history_undoable(H))
      return fail(h, -7, "%s: item %d: %d undo steps asked, session %d has %d", fn, i, k, ids[i], session_history_undoable(H));
    if (k < 0 && (k < -SESSION_HISTORY_MAX_DEPTH || -k > session_history_redoable(H)))
      return fail(h, -7, "%s: item %d: %lld redo steps asked, session %d has %d", fn, i, -(long long)k, ids[i], session_history_redoable(H));
  }
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);   // the residency of ian_session_brush ends: the activations belong to the latents that are replaced
  TotalTimer tt(h, st);
  std::vector<SessionHistory> next((size_t)n);   // the counters move only after every enqueue succeeded
  S.htab_shadow.resize((size_t)3 * n);
  for (int i = 0; i < n; ++i) {
    const int k = steps ? steps[i] : 1;
    int save = -1;
    next[i] = S.hist[ids[i]];
    const int load = k > 0 ? session_history_undo(next[i], S.arr.rings.depth, k, &save) : session_history_redo(next[i], S.arr.rings.depth, -k);
    S.htab_shadow[i] = ids[i];
    S.htab_shadow[(size_t)n + i] = save;
    S.htab_shadow[(size_t)2 * n + i] = load;
  }
  HIPCHK(h, hipMemcpyAsync(S.d_htab, S.htab_shadow.data(), (size_t)3 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  Slot& zs = h->slots[h->desc.z_slot];
  if ((rc = ensure_slot(h, h->desc.z_slot, n))) return rc;
  HIPCHK(h, launch_session_history_move(S.arr.pool, S.arr.rings, S.d_htab, S.d_htab + n, S.d_htab + (size_t)2 * n, zs.d, zs.cs, n, st));
  if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;   // sample_at(z) at this batch, as ian_session_set_latent runs it
  h->slot_stale[h->desc.out_slot] = 0;
  const ResultTarget sh = shown_target(h, shown, true);
  HIPCHK(h, launch_session_blend(session_blend_args(h, S.d_htab, nullptr, sh.dev, 1), n, st));
  for (int i = 0; i < n; ++i) ++S.version[ids[i]];
  if ((rc = session_finish(h, n, sh, false, st))) return rc;
  for (int i = 0; i < n; ++i) S.hist[ids[i]] = next[i];   // not `edited`: this call is what moves the cursor
  return 0;
}

int session_history(ian_handle* h, int id, int32_t* out) {
  const char* fn = "ian_session_history";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if (S.capacity > 0 && (rc = session_need(h, fn, SESS_HISTORY))) return rc;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (!out) return fail(h, -1, "null pointer passed to %s", fn);
  if ((rc = session_check_one(h, fn, -1, id, true))) return rc;
  out[0] = S.arr.rings.depth;
  out[1] = session_history_undoable(S.hist[id]);
  out[2] = session_history_redoable(S.hist[id]);
  return 0;
}

// ---- brush tips (DESIGN.md 4.12) ---------------------------------------------------------------------------------------------------
// A setting of the handle like the guide: one device array beside the pool, [count] slots of 64 x 64 floats.  A new count is a new
// array and every tip starts unset; the same count changes nothing.
int sessions_reserve_tips(ian_handle* h, int count) {
  const char* fn = "ian_sessions_reserve_tips";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (count < 0 || count > TIP_MAX_COUNT) return fail(h, -7, "%s: count %d outside 0..%d", fn, count, TIP_MAX_COUNT);
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read the tips that are freed
  h->last_pending = false;
  if (count == S.tip_count) return 0;
  sess_free_group(S, SESS_TIPS);
  if (count == 0) return 0;
  const size_t bytes = (size_t)count * TIP_SLOT * sizeof(float), sbytes = (size_t)count * TIP_SLOT * sizeof(double);
  float* d = nullptr;
  double* ds = nullptr;   // the shapes beside the weights: a tip never set has neither
  hipError_t e = hipMalloc((void**)&d, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&ds, sbytes);
  if (e == hipSuccess && (e = hipMemset(d, 0, bytes)) == hipSuccess && (e = hipMemset(ds, 0, sbytes)) == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    if (ds) (void)hipFree(ds);
    (void)hipGetLastError();
    return fail(h, -2, "%s: %s for %d tips of %zu bytes", fn, hipGetErrorString(e), count, TIP_SLOT * (sizeof(float) + sizeof(double)));
  }
  S.d_tips = d;
  S.d_tip_shape = ds;
  S.tip_count = count;
  S.tip_wh.assign((size_t)2 * count, 0);
  return 0;
}
// the tip index of ian_sessions_set_tip / ian_sessions_tip
int session_tip_index(ian_handle* h, const char* fn, int tip) {
  const int count = h->sess.tip_count;
  return tip >= 0 && tip < count ? 0 : fail(h, -7, "%s: tip %d outside the reservation (0..%d)", fn, tip, count - 1);
}
int sessions_set_tip(ian_handle* h, int tip, int tw, int th, const float* wn) {
  const char* fn = "ian_sessions_set_tip";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  if (!wn) return fail(h, -1, "null pointer passed to %s", fn);
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_TIPS))) return rc;
  if ((rc = session_tip_index(h, fn, tip))) return rc;
  if (tip_check_size(tw, th) != TIP_OK) return fail(h, -7, "%s: tip %d: size %d x %d, both sides must be 1..%d", fn, tip, tw, th, TIP_MAX_SIDE);
  if (is_device_ptr(wn)) return fail(h, -7, "%s: wn must be a host array", fn);
  int at = 0;
  if (tip_check_weights(wn, tw, th, &at) != TIP_OK)
    return fail(h, -7, "%s: tip %d: weight [%d][%d] = %g is not a finite number >= 0", fn, tip, at / tw, at % tw, (double)wn[at]);
  HIPCHK(h, hipDeviceSynchronize());   // no event in flight sees the tip change
  h->last_pending = false;
  std::vector<float> slot((size_t)TIP_SLOT);
  tip_to_slot(wn, tw, th, slot.data());
  S.tip_wh[2 * tip] = S.tip_wh[2 * tip + 1] = 0;   // a failed copy leaves the tip unset, not half written
  HIPCHK(h, hipMemcpy(S.d_tips + (size_t)tip * TIP_SLOT, slot.data(), TIP_SLOT * sizeof(float), hipMemcpyHostToDevice));
  std::vector<double> shape((size_t)TIP_SLOT);
  tip_shape_slot(wn, tw, th, shape.data());
  HIPCHK(h, hipMemcpy(S.d_tip_shape + (size_t)tip * TIP_SLOT, shape.data(), TIP_SLOT * sizeof(double), hipMemcpyHostToDevice));
  S.tip_wh[2 * tip] = tw;
  S.tip_wh[2 * tip + 1] = th;
  return 0;
}
int sessions_tip(ian_handle* h, int tip, int32_t* wh, float* wn_out) {
  const char* fn = "ian_sessions_tip";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  if (!wh) return fail(h, -1, "null pointer passed to %s", fn);
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_TIPS))) return rc;
  if ((rc = session_tip_index(h, fn, tip))) return rc;
  const int tw = S.tip_wh[2 * tip], th = S.tip_wh[2 * tip + 1];
  if (tw < 1) return fail(h, -7, "%s: tip %d has never been set (ian_sessions_set_tip)", fn, tip);
  if (wn_out) {
    if (is_device_ptr(wn_out)) return fail(h, -7, "%s: wn_out must be a host array", fn);
    std::vector<float> slot((size_t)TIP_SLOT);
    HIPCHK(h, hipMemcpy(slot.data(), S.d_tips + (size_t)tip * TIP_SLOT, TIP_SLOT * sizeof(float), hipMemcpyDeviceToHost));
    tip_from_slot(slot.data(), tw, th, wn_out);
  }
  wh[0] = tw;
  wh[1] = th;
  return 0;
}
// The tip-shaped footprint (DESIGN.md 4.18) is a setting of the handle like the pixel format, and host state only: the enqueue of the
// next call reads it.  It goes with the tips (sess_free_group).  Records, history and ian_session_read know nothing of it; in a pool
// without the local reservation it is kept and changes nothing.
int sessions_set_tip_footprint(ian_handle* h, int on) {
  const char* fn = "ian_sessions_set_soft_mask";
  int rc = session_ready(h, fn);
  if (rc) return rc;
  if ((rc = session_need(h, fn, SESS_BASE)) || (rc = session_need(h, fn, SESS_TIPS))) return rc;
  if (on != 0 && on != 1) return fail(h, -7, "%s: on = %d (0 = the rectangle's footprint, 1 = the tip's)", fn, on);
  HIPCHK(h, hipDeviceSynchronize());   // no event in flight sees the setting change
  h->last_pending = false;
  h->sess.tip_footprint = on != 0;
  return 0;
}
int sessions_tip_footprint(ian_handle* h, int32_t* on) {
  const char* fn = "ian_sessions_soft_mask";
  if (int rc = session_need(h, fn, SESS_BASE)) return rc;
  if (!on) return fail(h, -1, "null pointer passed to %s", fn);
  *on = h->sess.tip_footprint ? 1 : 0;
  return 0;
}
// What ian_session_brush_tip / ian_session_path_tip / ian_session_stamp_soft check about the tips array itself, after the checks of the plain call
int session_tips_arg(ian_handle* h, const char* fn, const int32_t* tips) {
  if (!tips) return fail(h, -7, "%s: null tips array (one tip index per item, -1 for none)", fn);
  if (is_device_ptr(tips)) return fail(h, -7, "%s: the tips must be a host array", fn);
  return session_need(h, fn, SESS_TIPS);
}
// ... and about one rectangle against its item's tip; point < 0: the item has one rectangle only
int session_tip_rect(ian_handle* h, const char* fn, int item, int point, int tip, int c1, int r1, int c2, int r2) {
  const auto& S = h->sess;
  const TipRefusal r = tip_check_event(tip, S.tip_count, S.tip_wh.data(), c1, r1, c2, r2);
  if (r == TIP_OK) return 0;
  char where[48];
  if (point >= 0) snprintf(where, sizeof where, "item %d: point %d", item, point);
  else snprintf(where, sizeof where, "item %d", item);
  if (r == TIP_OUTSIDE) return fail(h, -7, "%s: %s: tip %d outside -1..%d", fn, where, tip, S.tip_count - 1);
  if (r == TIP_NEVER_SET) return fail(h, -7, "%s: %s: tip %d has never been set (ian_sessions_set_tip)", fn, where, tip);
  return fail(h, -7, "%s: %s: patch (%d,%d,%d,%d) is not the %d x %d of tip %d", fn, where, c1, r1, c2, r2, S.tip_wh[2 * tip], S.tip_wh[2 * tip + 1], tip);
}

// The table of a brush, clone, stroke or fit call (EditTable, ian_edit_plan.h) starts here: d_stab holds L.words (it only grows, from
// the EDIT_TABLE_FLOOR it is reserved with: only a stroke of many points ever allocates), *t is its zeroed shadow with the tip indices in
// place.  The caller fills ids, seed words and item rows and, after session_enter, copies L.words up from the shadow.
int edit_table_begin(ian_handle* h, const EditTable& L, int n, const int32_t* tips, int32_t** t) {
  auto& S = h->sess;
  int rc = grow_dev(h, &S.d_stab, &S.stab_cap, L.words);
  if (rc) return rc;
  S.stab_shadow.assign(L.words, 0);
  *t = S.stab_shadow.data();
  if (L.has_tips) memcpy(*t + L.tips, tips, (size_t)n * sizeof(int32_t));
  return 0;
}
// one item row: ian_brush_item's layout
void edit_row(int32_t* row, int c1, int r1, int c2, int r2, int kind, float coef, float gscale) {
  row[0] = c1; row[1] = r1; row[2] = c2; row[3] = r2; row[4] = kind;
  memcpy(row + 5, &coef, sizeof(float));
  memcpy(row + 6, &gscale, sizeof(float));
}
// The residency of ian_session_brush / ian_session_stroke: the decoder's activations belong to sessions ids[i * stride], in that order, at
// their current latent versions.  hit: a call on exactly these may skip its gather and forward (IAN_NO_DEC_CACHE switches that off);
// arm: what a call that left them so records at its end (session_enter ended the residency at its start).
bool session_residency_hit(const decltype(ian_handle::sess)& S, int n, const int32_t* ids, int stride) {
  bool hit = S.res_valid && (int)S.res_ids.size() == n && getenv("IAN_NO_DEC_CACHE") == nullptr;
  for (int i = 0; hit && i < n; ++i) {
    const int id = ids[(size_t)i * stride];
    hit = S.res_ids[i] == id && S.res_ver[i] == S.version[id];
  }
  return hit;
}
void session_residency_arm(decltype(ian_handle::sess)& S, int n, const int32_t* ids, int stride) {
  S.res_ids.resize(n);
  S.res_ver.resize(n);
  for (int i = 0; i < n; ++i) {
    S.res_ids[i] = ids[(size_t)i * stride];
    S.res_ver[i] = S.version[S.res_ids[i]];
  }
  S.res_valid = true;
}
// What a brush renders after the events, in the same submission, one synchronisation for both results: nothing (ian_session_brush),
// window i of session views[i].session == ev[i].session (ian_session_brush_view: count == n) or canvas windows (ian_canvas_brush) -> out
struct BrushWindows {
  enum Kind { NONE, VIEWS, CANVAS } kind;
  const ian_session_view* views;       // VIEWS: [count]
  const ian_canvas_window* windows;    // CANVAS: [count]
  int count, vw, vh;
  uint8_t* out;
  int zoom = 1;               // vw x vh is the size at 1/zoom (DESIGN.md 4.14)
  const char* fn = nullptr;   // the entry's name in messages; nullptr: the one session_brush derives from kind
};
// A brush, clone or stroke call after its checks, its table filled in the shadow (edit_table_begin): everything it enqueues.
struct EditCall {
  const int32_t* ids; int stride;   // the sessions, ids[i * stride]
  EditPlan plan;
  EditTable tab;
  bool clone;                   // the seed words are SEED_CLONE's (source id, field selector, shift), not colours
  const int32_t* modes;         // strokes: modes[i * stride], the footprints of all their points go into UMASK first; nullptr: the blend's one will do
  const SessionHistory* next;   // strokes with bit 0 of flags: the histories after the mark; nullptr: no mark
  BrushWindows W;               // brushes only
};
EditCall edit_call(const int32_t* ids, int stride, const EditPlan& plan, bool tips, bool clone = false, const int32_t* modes = nullptr,
                   const SessionHistory* next = nullptr, const BrushWindows& W = BrushWindows{}) {
  return EditCall{ids, stride, plan, edit_table(plan, next != nullptr, tips), clone, modes, next, W};
}
// The pass loop of DESIGN.md 4.2.  Per pass of at most opt.brush_pass items: gather Z and one forward (neither when the residency hits),
// [the footprints,] and per step the shared middle -- seed, backward, update, forward at z_new, which IS the next step's forward while
// the same items go on -- then the stored blend of the items that end here (an earlier blend would be overwritten) and, when some are
// left, the forward again at their batch: per-event calls would miss their residency there, and the decoder's kernels may differ with it.
int edit_passes(ian_handle* h, const EditCall& C, uint8_t* shown, void* stream) {
  auto& S = h->sess;
  const EditPlan& P = C.plan; const EditTable& L = C.tab; const BrushWindows& W = C.W;
  const int n = P.n, pass = h->opt.brush_pass;
  int rc;
  ResultTarget win = {};
  const size_t win_bytes = (size_t)W.count * pixels_bpp(S.pixels) * (size_t)W.vh * (size_t)W.vw;
  if (W.kind != W.NONE && (rc = session_render_target(h, W.out, win_bytes, &win))) return rc;
  const bool hit = n <= pass && session_residency_hit(S, n, C.ids, C.stride);
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);   // also ends the residency: re-armed below
  TotalTimer tt(h, st);
  HIPCHK(h, hipMemcpyAsync(S.d_stab, S.stab_shadow.data(), L.words * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int* d = S.d_stab;
  if (C.next) HIPCHK(h, launch_session_history_save(S.arr.pool, S.arr.rings, d + L.ids, d + L.save, n, st));
  BrushSeedSrc seed0;   // what every step's seed has in common
  if (C.clone) { seed0.gim = S.arr.pool.gim; seed0.im = S.arr.pool.im; seed0.recon = S.arr.pool.recon; seed0.tanh_tab = S.d_tanh; }
  if (L.has_tips) seed0.tips = S.d_tips;
  Slot& zs = h->slots[h->desc.z_slot];
  const ResultTarget sh = shown_target(h, shown, true);
  // ian_sessions_set_soft_mask: an item with a tip leaves the tip's footprint, launch_session_tip_umask's, not its rectangle's
  const int* foot_tips = (S.tip_footprint && L.has_tips && S.arr.pool.umask) ? d + L.tips : nullptr;
  auto tip_of = [&](int i) { return foot_tips ? S.stab_shadow[L.tips + (size_t)i] : -1; };
  // what either footprint kernel would find on the device for item i, as far as the host knows it: the mode flag it does not
  auto paints_local = [&](int i) {
    return S.stab_shadow[L.items + (size_t)EDIT_ROW_WORDS * i + 4] == 1 && (S.local_flags[C.ids[(size_t)i * C.stride]] & 1);
  };
  for (int off = 0; off < n; off += pass) {
    const int nc = std::min(pass, n - off);
    if (!hit) {
      if ((rc = ensure_slot(h, h->desc.z_slot, nc))) return rc;
      HIPCHK(h, launch_session_gather_z(S.arr.pool, d + L.ids + off, zs.d, zs.cs, nc, st));
      if ((rc = batch_forward(h, nullptr, nc, st))) return rc;
    }
    bool footprints = false;   // what the kernel would find on the device, as far as the host knows it: the mode flag it does not
    for (int i = off; C.modes && S.arr.pool.umask && !footprints && i < off + nc; ++i)
      footprints = C.modes[(size_t)i * C.stride] == 1 && (S.local_flags[C.ids[(size_t)i * C.stride]] & 1) && tip_of(i) < 0;
    if (footprints)
      HIPCHK(h, launch_session_stroke_umask(S.arr.pool, d + L.ids, d + L.items, d + L.rows, P.count(off), off, S.d_falloff, foot_tips, nc, st));
    bool tip_footprints = false;
    for (int i = off; foot_tips && !tip_footprints && i < off + nc; ++i) tip_footprints = tip_of(i) >= 0 && paints_local(i);
    if (tip_footprints)
      HIPCHK(h, launch_session_tip_umask(S.arr.pool, d + L.ids, d + L.items, P.own_rows ? d + L.rows : nullptr, P.own_rows ? P.count(off) : 1, off,
                                         S.d_falloff, foot_tips, S.d_tip_shape, nc, st));
    rc = edit_pass_steps(P, off, nc, [&](const EditStep& s) -> int {
      BrushSeedSrc seed = seed0;
      seed.table = d + L.items + (size_t)EDIT_ROW_WORDS * s.row;
      const int* words = d + L.seed + (size_t)3 * off;
      if (C.clone) seed.clone = words;
      else seed.colour = reinterpret_cast<const float*>(words);
      if (L.has_tips) seed.tipsel = d + L.tips + off;   // the items of a step are a prefix of the pass: so are their tips
      if (int e = brush_pass_middle(h, s.act, seed, true, st)) return e;
      if (s.keep == s.act) return 0;   // the same items go on: the activations at z_new are the next step's
      SessionBlendArgs a = session_blend_args(h, d + L.ids + off + s.keep, seed.table + (size_t)EDIT_ROW_WORDS * s.keep,
                                              sh.dev + (size_t)(off + s.keep) * SESS_IMG, 1);
      a.xhat += (size_t)s.keep * SESS_IMG; a.zslot += (size_t)s.keep * zs.cs;
      if (foot_tips) a.tips = foot_tips + off + s.keep;
      HIPCHK(h, launch_session_blend(a, s.act - s.keep, st));
      return s.keep > 0 ? batch_forward(h, nullptr, s.keep, st) : 0;
    });
    if (rc) return rc;
  }
  h->slot_stale[h->desc.out_slot] = 0;
  // One note per session where per-event calls make one per step: the version is only ever compared for equality, and
  // session_history_edited is idempotent (DESIGN.md 4.9).  The marked histories move only now, after every enqueue succeeded.
  for (int i = 0; i < n; ++i) {
    const int id = C.ids[(size_t)i * C.stride];
    if (C.next) S.hist[id] = C.next[i];
    session_latent_written(S, id, false);
  }
  if (W.kind == W.VIEWS && (rc = session_render_enqueue(h, W.count, W.views, W.vw, W.vh, win.dev, st, W.zoom))) return rc;
  if (W.kind == W.CANVAS && (rc = canvas_compose_enqueue(h, W.count, W.windows, W.vw, W.vh, win.dev, st, W.zoom))) return rc;
  if ((rc = session_finish(h, n, sh, false, st, win, win_bytes))) return rc;
  if (edit_plan_resident(P, pass)) session_residency_arm(S, n, C.ids, C.stride);
  return 0;
}

// ian_session_brush and its forms: a stroke whose counts are all 1.  tipped: ian_session_brush_tip, one tip index per event (tips)
int session_brush(ian_handle* h, int n, const ian_session_event* ev, uint8_t* shown, void* stream, const BrushWindows& W,
                  bool tipped = false, const int32_t* tips = nullptr) {
  const char* fn = W.fn ? W.fn : tipped ? "ian_session_brush_tip"
                          : (W.kind == W.CANVAS ? "ian_canvas_brush" : (W.kind == W.VIEWS ? "ian_session_brush_view" : "ian_session_brush"));
  static_assert(sizeof(ian_session_event) == 11 * sizeof(int32_t), "ian_session_event is 11 words");
  int rc = session_check(h, fn, n, ev ? &ev->session : nullptr, 11, true, true);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    const ian_session_event& e = ev[i];
    if (e.mode != 0 && e.mode != 1) return fail(h, -7, "%s: item %d has mode %d (0 = imgrad, 1 = imgradRGB toward rgb)", fn, i, e.mode);
    if ((rc = check_rect(h, fn, i, e.c1, e.r1, e.c2, e.r2, "patch"))) return rc;
  }
  if ((rc = session_local_check(h, fn, n, &ev->session, 11))) return rc;
  if (tipped && (rc = session_tips_arg(h, fn, tips))) return rc;
  for (int i = 0; tipped && i < n; ++i)
    if ((rc = session_tip_rect(h, fn, i, -1, tips[i], ev[i].c1, ev[i].r1, ev[i].c2, ev[i].r2))) return rc;
  if (W.kind == W.VIEWS && (rc = session_view_check(h, fn, W.count, W.views, W.vw, W.vh, W.out, ev, W.zoom))) return rc;
  if (W.kind == W.CANVAS && (rc = canvas_window_check(h, fn, W.count, W.windows, W.vw, W.vh, W.out, W.zoom))) return rc;
  static const int32_t one = 1;
  const EditCall C = edit_call(&ev->session, 11, edit_plan(n, &one, 0, false), tipped, false, nullptr, nullptr, W);
  const EditTable& L = C.tab;
  int32_t* t;
  if ((rc = edit_table_begin(h, L, n, tips, &t))) return rc;
  for (int i = 0; i < n; ++i) {
    t[L.ids + i] = ev[i].session;
    memcpy(t + L.seed + (size_t)3 * i, ev[i].rgb, 3 * sizeof(float));
    memcpy(t + L.items + (size_t)EDIT_ROW_WORDS * i, &ev[i].c1, EDIT_ROW_WORDS * sizeof(int32_t));   // c1 .. gscale: ian_brush_item's layout
  }
  return edit_passes(h, C, shown, stream);
}

// ian_session_clone (DESIGN.md 4.10): a paint event towards a rectangle of another picture of the pool, `steps` gradient steps: a stroke
// whose items all have `steps` points on one row.  Seed words: source id, field selector (0 GIM, 1 IM, 2 RECON), shift dr * 64 + dc.
// tipped: ian_session_stamp_soft, one tip index per event (tips): the seed is SEED_CLONE_TIP's (DESIGN.md 4.18)
int session_clone(ian_handle* h, int n, const ian_session_clone_event* ev, int steps, uint8_t* shown, void* stream, bool tipped = false,
                  const int32_t* tips = nullptr) {
  const char* fn = tipped ? "ian_session_stamp_soft" : "ian_session_clone";
  static_assert(sizeof(ian_session_clone_event) == 11 * sizeof(int32_t), "ian_session_clone_event is 11 words");
  int rc = session_check(h, fn, n, ev ? &ev->session : nullptr, 11, true, true);
  if (rc) return rc;
  if (steps < 1 || steps > IAN_CLONE_MAX_STEPS) return fail(h, -7, "%s: steps = %d outside 1..%d", fn, steps, IAN_CLONE_MAX_STEPS);
  auto& S = h->sess;
  std::map<int, int> dest;
  for (int i = 0; i < n; ++i) dest.emplace(ev[i].session, i);
  auto selector = [](int field) { return field == IAN_SESSION_GIM ? 0 : (field == IAN_SESSION_IM ? 1 : (field == IAN_SESSION_RECON ? 2 : -1)); };
  auto inside = [](const ian_session_clone_event& e) { return e.c1 < e.c2 && e.r1 < e.r2; };   // the rectangle has elements: only then is the source read
  for (int i = 0; i < n; ++i) {
    const ian_session_clone_event& e = ev[i];
    if ((rc = check_rect(h, fn, i, e.c1, e.r1, e.c2, e.r2, "patch"))) return rc;
    if (e.source < 0 || e.source >= S.capacity) return fail(h, -7, "%s: item %d: source session %d outside the pool (capacity %d)", fn, i, e.source, S.capacity);
    if (!S.opened[e.source]) return fail(h, -7, "%s: item %d: source session %d has not been opened", fn, i, e.source);
    if (selector(e.field) < 0)
      return fail(h, -7, "%s: item %d: field %d (IAN_SESSION_GIM, IAN_SESSION_IM or IAN_SESSION_RECON of the source)", fn, i, e.field);
    if (inside(e) && ((long long)e.c1 + e.dc < 0 || (long long)e.c2 + e.dc > 64 || (long long)e.r1 + e.dr < 0 || (long long)e.r2 + e.dr > 64))
      return fail(h, -7, "%s: item %d: patch (%d,%d,%d,%d) shifted by (%d,%d) leaves the 64x64 image", fn, i, e.c1, e.r1, e.c2, e.r2, e.dc, e.dr);
    if (e.field == IAN_SESSION_IM && dest.count(e.source))
      return fail(h, -7, "%s: item %d: source session %d is read from IM, which item %d of this call writes", fn, i, e.source, dest[e.source]);
  }
  if ((rc = session_local_check(h, fn, n, &ev->session, 11))) return rc;
  if (tipped && (rc = session_tips_arg(h, fn, tips))) return rc;
  for (int i = 0; tipped && i < n; ++i)
    if ((rc = session_tip_rect(h, fn, i, -1, tips[i], ev[i].c1, ev[i].r1, ev[i].c2, ev[i].r2))) return rc;
  const int32_t count = steps;
  const EditCall C = edit_call(&ev->session, 11, edit_plan(n, &count, 0, false), tipped, true);
  const EditTable& L = C.tab;
  int32_t* t;
  if ((rc = edit_table_begin(h, L, n, tips, &t))) return rc;
  for (int i = 0; i < n; ++i) {
    const ian_session_clone_event& e = ev[i];
    t[L.ids + i] = e.session;
    int32_t* src = t + L.seed + (size_t)3 * i;
    src[0] = e.source; src[1] = selector(e.field); src[2] = inside(e) ? e.dr * 64 + e.dc : 0;
    edit_row(t + L.items + (size_t)EDIT_ROW_WORDS * i, e.c1, e.r1, e.c2, e.r2, 1, e.coef, e.gscale);   // loss kind 1: the blend sees a paint event
  }
  return edit_passes(h, C, shown, stream);
}

// ian_session_stroke (DESIGN.md 4.9): per session a path of rectangles, every step of it in one submission.  The meaning is the loop
// of ian_session_brush calls in include/ian.h; what is left out is what nobody would look at between the steps.  Step k has its own
// item rows (EditPlan, own_rows).  tipped: ian_session_path_tip, the same call with one tip index per stroke (tips)
int session_stroke(ian_handle* h, int n, const ian_session_stroke_item* sk, int nboxes, const ian_stroke_box* boxes, int flags,
                   uint8_t* shown, void* stream, bool tipped = false, const int32_t* tips = nullptr) {
  const char* fn = tipped ? "ian_session_path_tip" : "ian_session_stroke";
  static_assert(sizeof(ian_session_stroke_item) == 8 * sizeof(int32_t), "ian_session_stroke_item is 8 words");
  static_assert(sizeof(ian_stroke_box) == 5 * sizeof(int32_t), "ian_stroke_box is 5 words");
  static_assert(IAN_STROKE_MAX_POINTS == STROKE_MAX_POINTS, "the kernel's LDS holds one rectangle per point");
  int rc = session_check(h, fn, n, sk ? &sk->session : nullptr, 8, true, true);
  if (rc) return rc;
  if (flags & ~1) return fail(h, -7, "%s: flags %d: only bit 0 (mark first) is defined", fn, flags);
  const bool mark = (flags & 1) != 0;
  if (mark && (rc = session_need(h, fn, SESS_HISTORY))) return rc;
  if (!boxes) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(boxes)) return fail(h, -7, "%s: the boxes must be a host array", fn);
  if (nboxes < 1) return fail(h, -7, "%s: nboxes = %d: a stroke has at least one rectangle", fn, nboxes);
  for (int i = 0; i < n; ++i) {
    const ian_session_stroke_item& s = sk[i];
    if (s.mode != 0 && s.mode != 1) return fail(h, -7, "%s: item %d has mode %d (0 = imgrad, 1 = imgradRGB toward rgb)", fn, i, s.mode);
    if (s.count < 1 || s.count > IAN_STROKE_MAX_POINTS)
      return fail(h, -7, "%s: item %d: count %d outside 1..%d", fn, i, s.count, IAN_STROKE_MAX_POINTS);
    if (s.first < 0 || (long long)s.first + s.count > nboxes)
      return fail(h, -7, "%s: item %d: rectangles %d..%lld outside the %d boxes", fn, i, s.first, (long long)s.first + s.count - 1, nboxes);
    if (i > 0 && s.count > sk[i - 1].count)
      return fail(h, -7, "%s: item %d: count %d after item %d's %d (the strokes must come with non-increasing count)", fn, i, s.count, i - 1,
                  sk[i - 1].count);
    for (int k = 0; k < s.count; ++k) {
      const ian_stroke_box& b = boxes[s.first + k];
      if (b.c1 < 0 || b.r1 < 0 || b.c2 > 64 || b.r2 > 64)
        return fail(h, -7, "%s: item %d: point %d: patch (%d,%d,%d,%d) outside the 64x64 image", fn, i, k, b.c1, b.r1, b.c2, b.r2);
    }
  }
  if ((rc = session_local_check(h, fn, n, &sk->session, 8))) return rc;
  auto& S = h->sess;
  if (tipped && (rc = session_tips_arg(h, fn, tips))) return rc;
  for (int i = 0; tipped && i < n; ++i)
    for (int k = 0; k < sk[i].count; ++k) {
      const ian_stroke_box& b = boxes[sk[i].first + k];
      if ((rc = session_tip_rect(h, fn, i, k, tips[i], b.c1, b.r1, b.c2, b.r2))) return rc;
    }
  std::vector<SessionHistory> next((size_t)(mark ? n : 0));   // bit 0: the histories after the mark
  const EditCall C = edit_call(&sk->session, 8, edit_plan(n, &sk->count, 8, true), tipped, false, &sk->mode, mark ? next.data() : nullptr);
  const EditPlan& P = C.plan; const EditTable& L = C.tab;
  int32_t* t;
  if ((rc = edit_table_begin(h, L, n, tips, &t))) return rc;
  for (int i = 0; i < n; ++i) {
    t[L.ids + i] = sk[i].session;
    if (mark) {
      next[i] = S.hist[sk[i].session];
      t[L.save + i] = session_history_mark(next[i], S.arr.rings.depth);
    }
    memcpy(t + L.seed + (size_t)3 * i, sk[i].rgb, 3 * sizeof(float));
  }
  memcpy(t + L.rows, P.rows, ((size_t)P.steps + 1) * sizeof(int32_t));
  for (int k = 0; k < P.steps; ++k)
    for (int i = 0; i < P.rows[k + 1] - P.rows[k]; ++i) {
      const ian_stroke_box& b = boxes[sk[i].first + k];
      edit_row(t + L.items + (size_t)EDIT_ROW_WORDS * (P.rows[k] + i), b.c1, b.r1, b.c2, b.r2, sk[i].mode, sk[i].coef, b.gscale);
    }
  return edit_passes(h, C, shown, stream);
}

// ian_session_fit (DESIGN.md 4.8): the sessions' latents fitted to their own photos, `steps` Adam steps in one submission.  Per pass
// of at most opt.brush_pass items every step is: the decoder forward with kept activations, [the loss read-out,] the batched backward
// sweep seeded from the pool's GIM rows (SEED_PHOTO, no update fused into the GEMV), the Adam kernel on the latent slot.  Then the
// decoder as ian_decode_u8 runs it, [the last loss,] and the store kernel of an open: the call ends like Reset at the fitted latent.
constexpr int SESS_FIT_MAX_STEPS = 512;
int session_fit(ian_handle* h, int n, const ian_session_fit_item* items, int steps, float lr, double* loss, uint8_t* shown, void* stream) {
  const char* fn = "ian_session_fit";
  static_assert(sizeof(ian_session_fit_item) == 5 * sizeof(int32_t), "ian_session_fit_item is 5 words");
  int rc = session_check(h, fn, n, items ? &items->session : nullptr, 5, true, false);
  if (rc) return rc;
  Slot& out = h->slots[h->desc.out_slot];
  for (int i = 0; i < n; ++i)
    if ((rc = check_rect(h, fn, i, items[i].c1, items[i].r1, items[i].c2, items[i].r2, "rectangle"))) return rc;
  if (steps < 1 || steps > SESS_FIT_MAX_STEPS) return fail(h, -7, "%s: steps = %d outside 1..%d", fn, steps, SESS_FIT_MAX_STEPS);
  if (!std::isfinite(lr) || !(lr > 0.f)) return fail(h, -7, "%s: lr = %g is not a finite positive number", fn, (double)lr);
  auto& S = h->sess;
  const int zl = h->desc.num_latents;
  const int lstride = steps + 1;
  const bool loss_dev = loss && is_device_ptr(loss);
  if (!S.d_fit) HIPCHK(h, hipMalloc((void**)&S.d_fit, (size_t)2 * BATCH_MAX * zl * sizeof(float)));
  if (loss && !loss_dev && !S.d_fit_loss)
    HIPCHK(h, hipMalloc((void**)&S.d_fit_loss, (size_t)BATCH_MAX * (SESS_FIT_MAX_STEPS + 1) * sizeof(double)));
  // the bias corrections of every step, in double, rounded once (npe_ops.fit_adam_consts)
  std::vector<float> c1((size_t)steps + 1), c2((size_t)steps + 1);
  for (int t = 1; t <= steps; ++t) {
    c1[t] = (float)(1.0 / (1.0 - std::pow(0.9, (double)t)));
    c2[t] = (float)(1.0 / (1.0 - std::pow(0.999, (double)t)));
  }
  // the brush calls' table: one row per item (the rectangle, loss kind 1; coef and gscale unused), the seed words left zero
  static const int32_t one = 1;
  const EditTable L = edit_table(edit_plan(n, &one, 0, false), false, false);
  int32_t* t;
  if ((rc = edit_table_begin(h, L, n, nullptr, &t))) return rc;
  for (int i = 0; i < n; ++i) {
    t[L.ids + i] = items[i].session;
    edit_row(t + L.items + (size_t)EDIT_ROW_WORDS * i, items[i].c1, items[i].r1, items[i].c2, items[i].r2, 1, 0.f, 0.f);
  }
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);   // also ends the residency of ian_session_brush: not re-armed, the last forward keeps no activations
  TotalTimer tt(h, st);
  HIPCHK(h, hipMemcpyAsync(S.d_stab, t, L.words * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int* d_ids = S.d_stab + L.ids;
  HIPCHK(h, launch_session_fit_begin(S.arr.pool, d_ids, n, st));   // IM := GIM (NPE.py:332)
  Slot& zs = h->slots[h->desc.z_slot];
  double* d_loss = loss ? (loss_dev ? loss : S.d_fit_loss) : nullptr;
  const ResultTarget sh = shown_target(h, shown, false);
  const int pass = h->opt.brush_pass;
  for (int off = 0; off < n; off += pass) {
    const int nc = std::min(pass, n - off);
    if ((rc = ensure_slot(h, h->desc.z_slot, nc))) return rc;
    HIPCHK(h, launch_session_gather_z(S.arr.pool, d_ids + off, zs.d, zs.cs, nc, st));
    float* m = S.d_fit;
    float* v = S.d_fit + (size_t)nc * zl;
    HIPCHK(h, hipMemsetAsync(S.d_fit, 0, (size_t)2 * nc * zl * sizeof(float), st));   // the moments start at zero on every call
    BrushSeedSrc seed;
    seed.table = S.d_stab + L.items + (size_t)EDIT_ROW_WORDS * off;
    seed.gim = S.arr.pool.gim;
    seed.ids = d_ids + off;
    seed.tanh_tab = S.d_tanh;
    auto read_loss = [&](int t) -> hipError_t {
      return launch_session_fit_loss(out.d, S.arr.pool, seed.ids, seed.table, S.d_tanh, d_loss + (size_t)off * lstride + t, lstride, nc, st);
    };
    for (int t = 1; t <= steps; ++t) {
      if ((rc = batch_forward(h, nullptr, nc, st))) return rc;   // sample_at(Z_{t-1}), every activation kept
      if (d_loss) HIPCHK(h, read_loss(t - 1));
      if ((rc = brush_pass_middle(h, nc, seed, false, st))) return rc;   // g -> the z slot's gradient rows
      HIPCHK(h, launch_session_fit_adam(zs.d, zs.g, zs.cs, m, v, nc, zl, lr, c1[t], c2[t], st));
    }
    if ((rc = run_segment(h, IAN_SEG_DEC, nc, st))) return rc;   // sample_at(Z_steps) at this batch, as ian_decode_u8 runs it
    if (d_loss) HIPCHK(h, read_loss(steps));
    HIPCHK(h, launch_session_store(out.d, zs.d, zs.cs, S.arr.pool, seed.ids, 0, 1, sh.dev ? sh.dev + (size_t)off * SESS_IMG : nullptr, nc, st));
  }
  h->slot_stale[h->desc.out_slot] = 0;
  if (S.arr.pool.umask) HIPCHK(h, launch_session_local_set(S.arr.pool, d_ids, nullptr, n, st));   // USER_MASK *= 0 (NPE.py:337); LOCAL stays
  for (int i = 0; i < n; ++i) session_latent_written(S, items[i].session, true);   // the saved states no longer belong to the picture
  const bool loss_host = loss && !loss_dev;
  if (loss_host) HIPCHK(h, hipMemcpyAsync(loss, S.d_fit_loss, (size_t)n * lstride * sizeof(double), hipMemcpyDeviceToHost, st));
  return session_finish(h, n, sh, loss_host, st);
}

int session_render(ian_handle* h, const char* fn, int n, const ian_session_view* views, int vw, int vh, int zoom, uint8_t* out, void* stream) {
  if (int rc = session_view_check(h, fn, n, views, vw, vh, out, nullptr, zoom)) return rc;
  return window_call(h, n, vw, vh, out, stream,
                     [&](unsigned char* d, hipStream_t st) { return session_render_enqueue(h, n, views, vw, vh, d, st, zoom); });
}

int session_read(ian_handle* h, int id, int what, void* out, void* stream) {
  const char* fn = "ian_session_read";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  if (!out) return fail(h, -1, "null pointer passed to %s", fn);
  if ((rc = session_check_one(h, fn, -1, id, true))) return rc;
  const SessColumn* col = nullptr;
  for (const SessColumn& c : SESS_COLUMNS)
    if (c.field >= 0 && c.field == what) col = &c;
  if (col && col->group != SESS_BASE && (rc = session_need(h, fn, col->group))) return rc;
  if (what == IAN_SESSION_SOURCE && !S.has_src[id])
    return fail(h, -7, "%s: session %d has no full-resolution source (open it with ian_session_open_hires)", fn, id);
  if (!col) return fail(h, -7, "%s: field %d (enum ian_session_field)", fn, what);
  const size_t bytes = col->row_bytes(S.arr);
  const char* src = (const char*)slot_get(&S.arr, col->at) + (size_t)id * bytes;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  const bool dev = is_device_ptr(out);
  HIPCHK(h, hipMemcpyAsync(out, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  return session_rows_leave(h, st, dev);
}

// ---- saved sessions (DESIGN.md 4.6) ----------------------------------------------------------------------------------------------
// the layout of this pool's records
SessionRecordLayout session_record_layout(const decltype(ian_handle::sess)& S, const SessionRecordCols& T) {
  SessionRecordLayout L;
  L.num_latents = S.arr.pool.zl;
  L.scale = S.arr.pool.scale;
  L.local = S.arr.pool.umask ? 1 : 0;
  L.depth = S.arr.rings.depth;
  L.body_bytes = (long long)T.body_bytes;
  return L;
}
ian_session_meta session_record_meta(const SessionRecordLayout& L) {
  ian_session_meta m;
  memset(&m, 0, sizeof m);
  m.magic = IAN_SESSION_RECORD_MAGIC;
  m.format = IAN_SESSION_RECORD_FORMAT;
  m.num_latents = L.num_latents; m.scale = L.scale; m.local = L.local; m.depth = L.depth;
  m.body_bytes = L.body_bytes;
  return m;
}

int session_record_info(ian_handle* h, ian_session_meta* layout, int64_t* offsets, int32_t* ncols) {
  const char* fn = "ian_session_record_info";
  static_assert(sizeof(ian_session_meta) == 64, "ian_session_meta is 64 bytes");
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if ((rc = session_need(h, fn, SESS_BASE))) return rc;
  SessionRecordCols T;
  if (!sess_record_cols(S.arr, T)) return fail(h, -7, "%s: a record of this pool is larger than 2 GB", fn);
  if (layout) *layout = session_record_meta(session_record_layout(S, T));
  for (int k = 0; offsets && k < T.ncols; ++k) offsets[k] = T.col[k].off;
  if (ncols) *ncols = T.ncols;
  return 0;
}

// what ian_session_save and ian_session_load check beside the ids, before anything is enqueued
int session_record_check_args(ian_handle* h, const char* fn, const void* meta, const void* body, SessionRecordCols& T) {
  if (!meta || !body) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(meta)) return fail(h, -7, "%s: meta must be a host array", fn);
  if (reinterpret_cast<uintptr_t>(body) & 15) return fail(h, -7, "%s: body %p is not 16-byte aligned", fn, body);
  if (!sess_record_cols(h->sess.arr, T)) return fail(h, -7, "%s: a record of this pool is larger than 2 GB", fn);
  return 0;
}
// the per-item table (4 words per item: id, has_source, ring base, history length) up, in the one copy the call makes
int session_record_upload(ian_handle* h, int n, hipStream_t st) {
  auto& S = h->sess;
  if (!S.d_rtab) HIPCHK(h, hipMalloc((void**)&S.d_rtab, (size_t)BATCH_MAX * 4 * sizeof(int32_t)));
  HIPCHK(h, hipMemcpyAsync(S.d_rtab, S.rtab_shadow.data(), (size_t)4 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  return 0;
}
// records per pass through the staging buffer of a host body: what opt.session_stage_bytes holds, at least one; the buffer is there
int session_record_stage(ian_handle* h, int n, size_t body_bytes, int* per_pass) {
  auto& S = h->sess;
  const size_t fit = (size_t)h->opt.session_stage_bytes / body_bytes;
  *per_pass = (int)std::min<size_t>((size_t)n, std::max<size_t>(fit, 1));
  return grow_dev(h, &S.d_stage, &S.stage_cap, (size_t)*per_pass * body_bytes);
}

int session_save(ian_handle* h, int n, const int32_t* ids, ian_session_meta* meta, void* body, void* stream) {
  const char* fn = "ian_session_save";
  int rc = session_check(h, fn, n, ids, 1, true, false);
  if (rc) return rc;
  SessionRecordCols T;
  if ((rc = session_record_check_args(h, fn, meta, body, T))) return rc;
  auto& S = h->sess;
  const int depth = S.arr.rings.depth;
  const size_t bb = T.body_bytes;
  const bool dev = is_device_ptr(body);
  int per_pass = n;
  if (!dev && (rc = session_record_stage(h, n, bb, &per_pass))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  S.rtab_shadow.resize((size_t)4 * n);
  for (int i = 0; i < n; ++i) {
    const SessionHistory H = depth ? S.hist[ids[i]] : SessionHistory{};
    int32_t* t = S.rtab_shadow.data() + (size_t)4 * i;
    t[0] = ids[i]; t[1] = S.has_src[ids[i]] ? 1 : 0; t[2] = session_record_ring_slot(H.base, depth, 0); t[3] = H.len;
  }
  if ((rc = session_record_upload(h, n, st))) return rc;
  for (int off = 0; off < n; off += per_pass) {
    const int nc = std::min(per_pass, n - off);
    unsigned char* out = (unsigned char*)body + (size_t)off * bb;
    HIPCHK(h, launch_session_pack(S.arr.pool, S.arr.rings, T, S.d_rtab + (size_t)4 * off, dev ? out : S.d_stage, nc, st));
    if (!dev) HIPCHK(h, hipMemcpyAsync(out, S.d_stage, (size_t)nc * bb, hipMemcpyDeviceToHost, st));
  }
  const ian_session_meta layout = session_record_meta(session_record_layout(S, T));
  for (int i = 0; i < n; ++i) {
    const int32_t* t = S.rtab_shadow.data() + (size_t)4 * i;
    meta[i] = layout;
    meta[i].has_source = t[1];
    meta[i].local_flags = S.local_flags[ids[i]];
    meta[i].hist_len = t[3];
    meta[i].hist_cur = depth ? S.hist[ids[i]].cur : 0;
  }
  return session_rows_leave(h, st, dev);
}

int session_load(ian_handle* h, int n, const int32_t* ids, const ian_session_meta* meta, const void* body, void* stream) {
  const char* fn = "ian_session_load";
  int rc = session_check(h, fn, n, ids, 1, false, false);
  if (rc) return rc;
  SessionRecordCols T;
  if ((rc = session_record_check_args(h, fn, meta, body, T))) return rc;
  auto& S = h->sess;
  const SessionRecordLayout L = session_record_layout(S, T);
  for (int i = 0; i < n; ++i) {
    const SessionRecordRefusal r = session_record_check(meta[i], L);
    if (r.field) return fail(h, -7, "%s: item %d: %s = %lld (this pool: %lld): %s", fn, i, r.field, r.got, r.want, r.why);
  }
  const size_t bb = T.body_bytes;
  const bool dev = is_device_ptr(body);
  int per_pass = n;
  if (!dev && (rc = session_record_stage(h, n, bb, &per_pass))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = session_rows_enter(h, st))) return rc;
  for (int i = 0; i < n; ++i) canvas_unplace(h, ids[i]);   // another session's state: not where this id was placed
  if ((rc = canvas_table_flush(h, st))) return rc;
  S.rtab_shadow.resize((size_t)4 * n);
  for (int i = 0; i < n; ++i) {
    int32_t* t = S.rtab_shadow.data() + (size_t)4 * i;
    t[0] = ids[i]; t[1] = meta[i].has_source; t[2] = 0; t[3] = meta[i].hist_len;   // the ring restarts at slot 0
  }
  if ((rc = session_record_upload(h, n, st))) return rc;
  for (int off = 0; off < n; off += per_pass) {
    const int nc = std::min(per_pass, n - off);
    const unsigned char* in = (const unsigned char*)body + (size_t)off * bb;
    if (!dev) HIPCHK(h, hipMemcpyAsync(S.d_stage, in, (size_t)nc * bb, hipMemcpyHostToDevice, st));
    HIPCHK(h, launch_session_unpack(S.arr.pool, S.arr.rings, T, S.d_rtab + (size_t)4 * off, dev ? in : S.d_stage, nc, st));
  }
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    S.opened[id] = 1;
    ++S.version[id];   // a forward left resident for this id belongs to the latent that was just replaced
    S.has_src[id] = (char)meta[i].has_source;
    S.local_flags[id] = (char)meta[i].local_flags;
    S.hist[id] = SessionHistory{0, meta[i].hist_len, meta[i].hist_cur};
  }
  return session_rows_leave(h, st, dev);
}

}  // namespace

extern "C" {

int ian_sessions_reserve(ian_handle* h, int32_t capacity) {
  return h ? sessions_reserve(h, capacity) : -1;
}
int ian_sessions_set_blend(ian_handle* h, const double* gauss_half, int32_t radius) { return sessions_set_blend(h, gauss_half, radius); }
int ian_session_open(ian_handle* h, int32_t n, const int32_t* ids, const uint8_t* photos, int32_t source, uint8_t* shown, void* stream) {
  return h ? session_open(h, n, ids, photos, source, shown, stream, false) : -1;
}
int ian_sessions_reserve_hires(ian_handle* h, int32_t scale) {
  return h ? sessions_reserve_hires(h, scale) : -1;
}
int ian_sessions_set_pixels(ian_handle* h, int32_t format) { return h ? sessions_set_pixels(h, format) : -1; }
int ian_sessions_pixels(ian_handle* h) { return h ? sessions_pixels(h) : -1; }
int ian_sessions_reserve_guide(ian_handle* h, const float* table, int32_t count) {
  return h ? sessions_reserve_guide(h, table, count) : -1;
}
int ian_sessions_guide(ian_handle* h, float* table_out) {
  return h ? sessions_guide(h, table_out) : -1;
}
int ian_session_open_hires(ian_handle* h, int32_t n, const int32_t* ids, const uint8_t* photos, uint8_t* shown, void* stream) {
  return h ? session_open(h, n, ids, photos, 0, shown, stream, true) : -1;
}
int ian_session_render(ian_handle* h, int32_t n, const ian_session_view* views, int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  return h ? session_render(h, "ian_session_render", n, views, vw, vh, 1, out, stream) : -1;
}
int ian_session_zoom(ian_handle* h, int32_t n, const ian_session_view* views, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out,
                            void* stream) {
  return h ? session_render(h, "ian_session_zoom", n, views, vw, vh, zoom, out, stream) : -1;
}
int ian_session_brush_zoom(ian_handle* h, int32_t n, const ian_session_event* events, const int32_t* tips, uint8_t* shown,
                                const ian_session_view* views, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out, void* stream) {
  if (!h) return -1;
  if (!views) return fail(h, -1, "null pointer passed to ian_session_brush_zoom");
  const BrushWindows W = {BrushWindows::VIEWS, views, nullptr, n, vw, vh, out, zoom, "ian_session_brush_zoom"};
  return session_brush(h, n, events, shown, stream, W, tips != nullptr, tips);
}
int ian_session_brush_view(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, const ian_session_view* views,
                           int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  return h ? session_brush(h, n, events, shown, stream, BrushWindows{BrushWindows::VIEWS, views, nullptr, n, vw, vh, out}) : -1;
}
int ian_session_set_latent(ian_handle* h, int32_t n, const int32_t* ids, const float* z, int32_t as_sample, uint8_t* shown, void* stream) {
  return h ? session_set_latent(h, n, ids, z, as_sample, shown, stream) : -1;
}
int ian_session_brush(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, void* stream) {
  return h ? session_brush(h, n, events, shown, stream, BrushWindows{}) : -1;
}
int ian_sessions_reserve_tips(ian_handle* h, int32_t count) {
  return h ? sessions_reserve_tips(h, count) : -1;
}
int ian_sessions_set_tip(ian_handle* h, int32_t tip, int32_t tw, int32_t th, const float* wn) {
  return h ? sessions_set_tip(h, tip, tw, th, wn) : -1;
}
int ian_sessions_set_soft_mask(ian_handle* h, int32_t on) { return h ? sessions_set_tip_footprint(h, on) : -1; }
int ian_sessions_soft_mask(ian_handle* h, int32_t* on) { return h ? sessions_tip_footprint(h, on) : -1; }
int ian_sessions_tip(ian_handle* h, int32_t tip, int32_t wh[2], float* wn_out) {
  return h ? sessions_tip(h, tip, wh, wn_out) : -1;
}
int ian_session_brush_tip(ian_handle* h, int32_t n, const ian_session_event* events, const int32_t* tips, uint8_t* shown,
                          const ian_session_view* views, int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  if (!h) return -1;
  const BrushWindows W = views ? BrushWindows{BrushWindows::VIEWS, views, nullptr, n, vw, vh, out} : BrushWindows{};
  return session_brush(h, n, events, shown, stream, W, true, tips);
}
int ian_session_read(ian_handle* h, int32_t id, int32_t what, void* out, void* stream) {
  return h ? session_read(h, id, what, out, stream) : -1;
}
int ian_sessions_reserve_local(ian_handle* h, int32_t on) {
  return h ? sessions_reserve_local(h, on) : -1;
}
int ian_sessions_set_local(ian_handle* h, const double* falloff64, double dampen_thresh) {
  return h ? sessions_set_local(h, falloff64, dampen_thresh) : -1;
}
int ian_session_local(ian_handle* h, int32_t n, const int32_t* ids, const int32_t* flags, void* stream) {
  return h ? session_local(h, n, ids, flags, stream) : -1;
}
int ian_sessions_reserve_history(ian_handle* h, int32_t depth) {
  return h ? sessions_reserve_history(h, depth) : -1;
}
int ian_session_mark(ian_handle* h, int32_t n, const int32_t* ids, void* stream) {
  return h ? session_mark(h, n, ids, stream) : -1;
}
int ian_session_undo(ian_handle* h, int32_t n, const int32_t* ids, const int32_t* steps, uint8_t* shown, void* stream) {
  return h ? session_undo(h, n, ids, steps, shown, stream) : -1;
}
int ian_session_history(ian_handle* h, int32_t id, int32_t out[3]) {
  return h ? session_history(h, id, out) : -1;
}
int ian_session_fit(ian_handle* h, int32_t n, const ian_session_fit_item* items, int32_t steps, float lr, double* loss, uint8_t* shown,
                    void* stream) {
  return h ? session_fit(h, n, items, steps, lr, loss, shown, stream) : -1;
}
int ian_session_clone(ian_handle* h, int32_t n, const ian_session_clone_event* events, int32_t steps, uint8_t* shown, void* stream) {
  return h ? session_clone(h, n, events, steps, shown, stream) : -1;
}
int ian_session_stamp_soft(ian_handle* h, int32_t n, const ian_session_clone_event* events, const int32_t* tips, int32_t steps,
                          uint8_t* shown, void* stream) {
  return h ? session_clone(h, n, events, steps, shown, stream, true, tips) : -1;
}
int ian_session_record_info(ian_handle* h, ian_session_meta* layout, int64_t* offsets, int32_t* ncols) {
  return h ? session_record_info(h, layout, offsets, ncols) : -1;
}
int ian_session_save(ian_handle* h, int32_t n, const int32_t* ids, ian_session_meta* meta, void* body, void* stream) {
  return h ? session_save(h, n, ids, meta, body, stream) : -1;
}
int ian_session_load(ian_handle* h, int32_t n, const int32_t* ids, const ian_session_meta* meta, const void* body, void* stream) {
  return h ? session_load(h, n, ids, meta, body, stream) : -1;
}
void ian_session_tanh_table(float* out256) {
  if (out256) session_tanh_table(out256);
}

}  // extern "C"
