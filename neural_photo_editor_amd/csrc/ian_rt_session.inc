// ian_rt_session.inc -- device-resident edit sessions: the pool, open / set_latent / brush / read by session id.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
//
// What NPE.py keeps in host globals per editor (GIM, IM, RECON, ERROR, Z, SAMPLE_FLAG) is one row per session id in each array of
// h->sess.pool.  A call names sessions by id; per brush call the only host -> device traffic is the event table (11 words per
// event) and the only device -> host traffic the canvas images.  The host keeps, per session, whether it was opened and a
// counter of its latent's versions (the residency key of ian_session_brush is n ids + n counters, not the latents' bytes).
//
// Full-resolution sessions (ian_sessions_reserve_hires, DESIGN.md 4.3) add three arrays: SRC (the photo at S x S, S = 64 * scale), FIELD
// and FIELD_KIND (what the last call displayed, as something ian_session_render can apply to SRC), and a per-session host flag
// "SRC holds a photo".  Without that reservation pool.src / field / kind are null and no kernel touches them.
//
// Local edits (ian_sessions_reserve_local, DESIGN.md 4.4) add UMASK (where the user has brushed) and the LOCAL flags per session, and
// per handle the falloff table of the brush footprint.  Without that reservation pool.umask / local are null, launch_session_blend
// runs session_blend_kernel, and no other kernel is launched.
namespace {

constexpr size_t SESS_IMG = 3 * 64 * 64;
constexpr int SESS_MAX_CAPACITY = 1 << 20;

// np.asarray([to_tanh(IM)], dtype=np.float32) per uint8 level: float64 2.0*(v/255.0)-1.0, then one rounding to float32
void session_tanh_table(float* out) {
  for (int v = 0; v < 256; ++v) {
    volatile double q = (double)v / 255.0;
    volatile double t = 2.0 * q;
    out[v] = (float)(t - 1.0);
  }
}

void sessions_free(ian_handle* h) {
  auto& S = h->sess;
  SessionPool& P = S.pool;
  for (void* p : {(void*)P.gim, (void*)P.im, (void*)P.recon, (void*)P.error, (void*)P.z, (void*)P.mode, (void*)S.d_tab, (void*)S.d_tanh,
                  (void*)S.d_photo, (void*)S.d_shown, (void*)P.src, (void*)P.field, (void*)P.kind, (void*)S.d_views, (void*)S.d_out,
                  (void*)P.umask, (void*)P.local, (void*)S.d_falloff, (void*)S.d_ltab})
    if (p) (void)hipFree(p);
  P = SessionPool{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  S.d_falloff = nullptr;
  S.d_ltab = nullptr;
  S.falloff_set = false;
  S.local_flags.clear();
  S.d_tab = nullptr;
  S.d_tanh = nullptr;
  S.d_photo = S.d_shown = nullptr;
  S.d_views = nullptr;
  S.d_out = nullptr;
  S.out_cap = 0;
  S.capacity = 0;
  S.opened.clear();
  S.version.clear();
  S.has_src.clear();
  S.res_valid = false;
}

size_t sess_src_bytes(int scale) { return 3 * (size_t)(64 * scale) * (size_t)(64 * scale); }
constexpr size_t SESS_UMASK = 64 * 64 * sizeof(double);

// session calls need the 3x64x64 image on both ends (the pool rows, the blend and the open kernels are written for it)
int session_model_check(ian_handle* h, const char* fn) {
  const Slot& os = h->slots[h->desc.out_slot];
  const Slot& xs = h->slots[h->desc.x_slot];
  if (os.h != 64 || os.w != 64 || os.c != 3 || !os.nchw || xs.h != 64 || xs.w != 64 || xs.c != 3 || !xs.nchw)
    return fail(h, -7, "%s: edit sessions need a model with a 3x64x64 image", fn);
  return 0;
}

int sessions_reserve(ian_handle* h, int capacity) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if ((rc = session_model_check(h, "ian_sessions_reserve"))) return rc;
  if (capacity < 0 || capacity > SESS_MAX_CAPACITY) return fail(h, -7, "ian_sessions_reserve: capacity %d outside 0..%d", capacity, SESS_MAX_CAPACITY);
  auto& S = h->sess;
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that move
  h->last_pending = false;
  S.res_valid = false;
  if (capacity == 0) {
    sessions_free(h);
    return 0;
  }
  const int zl = h->desc.num_latents;
  if (capacity != S.capacity) {
    SessionPool N{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, zl};
    N.scale = S.pool.scale;
    const size_t c = (size_t)capacity, keep = (size_t)std::min(capacity, S.capacity);
    auto grow = [&](void** dst, const void* src, size_t row_bytes) -> hipError_t {
      hipError_t e = hipMalloc(dst, c * row_bytes);
      if (e == hipSuccess && keep) e = hipMemcpy(*dst, src, keep * row_bytes, hipMemcpyDeviceToDevice);
      return e;
    };
    hipError_t e = grow((void**)&N.gim, S.pool.gim, SESS_IMG);
    if (e == hipSuccess) e = grow((void**)&N.im, S.pool.im, SESS_IMG);
    if (e == hipSuccess) e = grow((void**)&N.recon, S.pool.recon, SESS_IMG);
    if (e == hipSuccess) e = grow((void**)&N.error, S.pool.error, SESS_IMG * sizeof(float));
    if (e == hipSuccess) e = grow((void**)&N.z, S.pool.z, (size_t)zl * sizeof(float));
    if (e == hipSuccess) e = grow((void**)&N.mode, S.pool.mode, sizeof(int));
    if (N.scale) {   // a full-resolution pool: its three arrays follow the capacity
      if (e == hipSuccess) e = grow((void**)&N.src, S.pool.src, sess_src_bytes(N.scale));
      if (e == hipSuccess) e = grow((void**)&N.field, S.pool.field, SESS_IMG * sizeof(float));
      if (e == hipSuccess) e = grow((void**)&N.kind, S.pool.kind, sizeof(int));
    }
    if (S.pool.umask) {   // a pool with the local reservation: UMASK and LOCAL follow the capacity, new rows are zero
      auto grow0 = [&](void** dst, const void* src, size_t row_bytes) -> hipError_t {
        hipError_t g = grow(dst, src, row_bytes);
        if (g == hipSuccess && c > keep) g = hipMemset((char*)*dst + keep * row_bytes, 0, (c - keep) * row_bytes);
        return g;
      };
      if (e == hipSuccess) e = grow0((void**)&N.umask, S.pool.umask, SESS_UMASK);
      if (e == hipSuccess) e = grow0((void**)&N.local, S.pool.local, sizeof(int));
      if (e == hipSuccess) e = hipDeviceSynchronize();   // the zeros are there before any stream reads them
    }
    if (e != hipSuccess) {   // the old pool stays as it was
      for (void* p : {(void*)N.gim, (void*)N.im, (void*)N.recon, (void*)N.error, (void*)N.z, (void*)N.mode, (void*)N.src, (void*)N.field,
                      (void*)N.kind, (void*)N.umask, (void*)N.local})
        if (p) (void)hipFree(p);
      (void)hipGetLastError();
      return fail(h, -2, "ian_sessions_reserve: %s for %d sessions of %zu bytes", hipGetErrorString(e), capacity,
                  3 * SESS_IMG + SESS_IMG * sizeof(float) + (size_t)zl * sizeof(float) + sizeof(int) +
                      (N.scale ? sess_src_bytes(N.scale) + SESS_IMG * sizeof(float) + sizeof(int) : 0) +
                      (S.pool.umask ? SESS_UMASK + sizeof(int) : 0));
    }
    for (void* p : {(void*)S.pool.gim, (void*)S.pool.im, (void*)S.pool.recon, (void*)S.pool.error, (void*)S.pool.z, (void*)S.pool.mode,
                    (void*)S.pool.src, (void*)S.pool.field, (void*)S.pool.kind, (void*)S.pool.umask, (void*)S.pool.local})
      if (p) (void)hipFree(p);
    S.pool = N;
    S.capacity = capacity;
    S.opened.resize(c, 0);
    S.version.resize(c, 0);
    S.has_src.resize(c, 0);
    S.local_flags.resize(c, 0);
  }
  if (!S.d_tab) HIPCHK(h, hipMalloc((void**)&S.d_tab, (size_t)BATCH_MAX * 11 * sizeof(int32_t)));
  if (!S.d_shown) HIPCHK(h, hipMalloc((void**)&S.d_shown, (size_t)BATCH_MAX * SESS_IMG));
  if (!S.d_tanh) {
    float tab[256];
    session_tanh_table(tab);
    HIPCHK(h, hipMalloc((void**)&S.d_tanh, sizeof tab));
    HIPCHK(h, hipMemcpy(S.d_tanh, tab, sizeof tab, hipMemcpyHostToDevice));
  }
  return 0;
}

int sessions_reserve_hires(ian_handle* h, int scale) {
  const char* fn = "ian_sessions_reserve_hires";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if ((rc = session_model_check(h, fn))) return rc;
  auto& S = h->sess;
  if (S.capacity <= 0) return fail(h, -6, "%s: no session pool (call ian_sessions_reserve first)", fn);
  if (scale < 0 || scale > 16) return fail(h, -7, "%s: scale %d outside 0..16", fn, scale);
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that are freed
  h->last_pending = false;
  if (scale == S.pool.scale) return 0;
  SessionPool& P = S.pool;
  if (scale == 0) {
    for (void* p : {(void*)P.src, (void*)P.field, (void*)P.kind, (void*)S.d_views, (void*)S.d_out})
      if (p) (void)hipFree(p);
    P.src = nullptr;
    P.field = nullptr;
    P.kind = nullptr;
    P.scale = 0;
    S.d_views = nullptr;
    S.d_out = nullptr;
    S.out_cap = 0;
    std::fill(S.has_src.begin(), S.has_src.end(), 0);
    return 0;
  }
  // a new scale: a new SRC array (no photo survives, its size differs); FIELD and FIELD_KIND are allocated once, zeroed so that a
  // session opened before this call reads as "nothing edited"
  const size_t c = (size_t)S.capacity;
  unsigned char* src = nullptr;
  float* field = P.field;
  int* kind = P.kind;
  int* views = S.d_views;
  hipError_t e = hipMalloc((void**)&src, c * sess_src_bytes(scale));
  if (e == hipSuccess && !field) {
    e = hipMalloc((void**)&field, c * SESS_IMG * sizeof(float));
    if (e == hipSuccess) e = hipMemset(field, 0, c * SESS_IMG * sizeof(float));
  }
  if (e == hipSuccess && !kind) {
    e = hipMalloc((void**)&kind, c * sizeof(int));
    if (e == hipSuccess) e = hipMemset(kind, 0, c * sizeof(int));
  }
  if (e == hipSuccess && !views) e = hipMalloc((void**)&views, (size_t)BATCH_MAX * 3 * sizeof(int32_t));
  if (e != hipSuccess) {   // the old pool stays as it was
    if (src) (void)hipFree(src);
    if (field && field != P.field) (void)hipFree(field);
    if (kind && kind != P.kind) (void)hipFree(kind);
    if (views && views != S.d_views) (void)hipFree(views);
    (void)hipGetLastError();
    return fail(h, -2, "%s: %s for %d sessions of %zu bytes", fn, hipGetErrorString(e), S.capacity,
                sess_src_bytes(scale) + SESS_IMG * sizeof(float) + sizeof(int));
  }
  if (P.src) (void)hipFree(P.src);
  P.src = src;
  P.field = field;
  P.kind = kind;
  P.scale = scale;
  S.d_views = views;
  std::fill(S.has_src.begin(), S.has_src.end(), 0);
  return 0;
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

int session_check(ian_handle* h, const char* fn, int n, const int32_t* ids, int stride, bool need_opened, bool need_blend);

int sessions_reserve_local(ian_handle* h, int on) {
  const char* fn = "ian_sessions_reserve_local";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if ((rc = session_model_check(h, fn))) return rc;
  auto& S = h->sess;
  if (S.capacity <= 0) return fail(h, -6, "%s: no session pool (call ian_sessions_reserve first)", fn);
  if (on != 0 && on != 1) return fail(h, -7, "%s: on = %d (0 frees, 1 allocates)", fn, on);
  HIPCHK(h, hipDeviceSynchronize());   // pending work may still read or write the rows that are freed
  h->last_pending = false;
  SessionPool& P = S.pool;
  if (!on) {   // everything of the feature goes, the table too: a later reservation starts from nothing
    for (void* p : {(void*)P.umask, (void*)P.local, (void*)S.d_falloff, (void*)S.d_ltab})
      if (p) (void)hipFree(p);
    P.umask = nullptr;
    P.local = nullptr;
    S.d_falloff = nullptr;
    S.d_ltab = nullptr;
    S.falloff_set = false;
    std::fill(S.local_flags.begin(), S.local_flags.end(), 0);
    return 0;
  }
  if (P.umask) return 0;
  const size_t c = (size_t)S.capacity;
  double* umask = nullptr;
  int* local = nullptr;
  double* falloff = nullptr;
  int* ltab = nullptr;
  hipError_t e = hipMalloc((void**)&umask, c * SESS_UMASK);
  if (e == hipSuccess) e = hipMemset(umask, 0, c * SESS_UMASK);
  if (e == hipSuccess) e = hipMalloc((void**)&local, c * sizeof(int));
  if (e == hipSuccess) e = hipMemset(local, 0, c * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&falloff, 64 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&ltab, (size_t)BATCH_MAX * 2 * sizeof(int32_t));
  if (e == hipSuccess) e = hipDeviceSynchronize();   // the zeros are there before any stream reads them
  if (e != hipSuccess) {   // the old pool stays as it was
    for (void* p : {(void*)umask, (void*)local, (void*)falloff, (void*)ltab})
      if (p) (void)hipFree(p);
    (void)hipGetLastError();
    return fail(h, -2, "%s: %s for %d sessions of %zu bytes", fn, hipGetErrorString(e), S.capacity, SESS_UMASK + sizeof(int));
  }
  P.umask = umask;
  P.local = local;
  S.d_falloff = falloff;
  S.d_ltab = ltab;
  S.falloff_set = false;
  S.local_flags.assign(c, 0);
  return 0;
}

int sessions_set_local(ian_handle* h, const double* falloff64, double dampen_thresh) {
  const char* fn = "ian_sessions_set_local";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if ((rc = session_model_check(h, fn))) return rc;
  if (!falloff64) return fail(h, -1, "null pointer passed to %s", fn);
  auto& S = h->sess;
  if (!S.pool.umask) return fail(h, -6, "%s: no local reservation (call ian_sessions_reserve_local first)", fn);
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
  if (!S.pool.umask || S.falloff_set) return 0;
  for (int i = 0; i < n; ++i) {
    const int id = ids[(size_t)i * stride];
    if (S.local_flags[id])
      return fail(h, -6, "%s: item %d: session %d has local flags %d, but the falloff table is not set (call ian_sessions_set_local first)",
                  fn, i, id, (int)S.local_flags[id]);
  }
  return 0;
}

int session_local(ian_handle* h, int n, const int32_t* ids, const int32_t* flags, void* stream) {
  const char* fn = "ian_session_local";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if (S.capacity > 0 && !S.pool.umask) return fail(h, -6, "%s: no local reservation (call ian_sessions_reserve_local first)", fn);
  if ((rc = session_check(h, fn, n, ids, 1, true, false))) return rc;
  if (!flags) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(flags)) return fail(h, -7, "%s: the flags must be a host array", fn);
  for (int i = 0; i < n; ++i)
    if (flags[i] < 0 || flags[i] > 3) return fail(h, -7, "%s: item %d: flags %d outside 0..3 (bit 0 = local, bit 1 = dampen)", fn, i, flags[i]);
  // writes pool rows only, as ian_session_read reads them: the decoder's activations and the residency of ian_session_brush survive it
  hipStream_t st = (hipStream_t)stream;
  if (h->last_pending && h->last_stream != st) HIPCHK(h, hipStreamSynchronize(h->last_stream));
  S.ltab_shadow.resize((size_t)2 * n);
  memcpy(S.ltab_shadow.data(), ids, (size_t)n * sizeof(int32_t));
  memcpy(S.ltab_shadow.data() + n, flags, (size_t)n * sizeof(int32_t));
  HIPCHK(h, hipMemcpyAsync(S.d_ltab, S.ltab_shadow.data(), (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_session_local_set(S.pool, S.d_ltab, S.d_ltab + n, n, st));
  for (int i = 0; i < n; ++i) S.local_flags[ids[i]] = (char)flags[i];
  h->last_stream = st;
  h->last_pending = true;
  return 0;
}

// what every session call checks first: the model, the pool, n; then per item its id (ids[i * stride]).  Nothing is enqueued or
// written before all of it passed.
int session_check(ian_handle* h, const char* fn, int n, const int32_t* ids, int stride, bool need_opened, bool need_blend) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if ((rc = session_model_check(h, fn))) return rc;
  auto& S = h->sess;
  if (S.capacity <= 0) return fail(h, -6, "%s: no session pool (call ian_sessions_reserve first)", fn);
  if (n < 1 || n > BATCH_MAX) return fail(h, -7, "%s: n = %d outside 1..%d", fn, n, BATCH_MAX);
  if (!ids) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(ids)) return fail(h, -7, "%s: the session ids / events must be a host array", fn);
  if (need_blend && S.radius < 0) return fail(h, -6, "%s: the photo blend's Gaussian is not set (call ian_sessions_set_blend first)", fn);
  std::map<int, int> first;
  for (int i = 0; i < n; ++i) {
    const int id = ids[(size_t)i * stride];
    if (id < 0 || id >= S.capacity) return fail(h, -7, "%s: item %d: session %d outside the pool (capacity %d)", fn, i, id, S.capacity);
    if (need_opened && !S.opened[id]) return fail(h, -7, "%s: item %d: session %d has not been opened", fn, i, id);
    auto ins = first.emplace(id, i);
    if (!ins.second) return fail(h, -7, "%s: item %d: session %d already appears as item %d of this call", fn, i, id, ins.first->second);
  }
  return 0;
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

// end of a call: the canvas images (and, for ian_session_brush_view, the windows rendered into the staging buffer: out_host with
// its byte count) to the caller; one synchronisation when host memory was read or written
int session_finish(ian_handle* h, int n, uint8_t* shown, bool shown_dev, bool host_in, hipStream_t st, uint8_t* out_host = nullptr,
                   size_t out_bytes = 0) {
  if (shown && !shown_dev) HIPCHK(h, hipMemcpyAsync(shown, h->sess.d_shown, (size_t)n * SESS_IMG, hipMemcpyDeviceToHost, st));
  if (out_host) HIPCHK(h, hipMemcpyAsync(out_host, h->sess.d_out, out_bytes, hipMemcpyDeviceToHost, st));
  if ((shown && !shown_dev) || host_in || out_host) {
    HIPCHK(h, hipStreamSynchronize(st));
    h->last_pending = false;
  }
  return 0;
}

// what ian_session_render and ian_session_brush_view check about the windows, before anything is enqueued: the reservation, n, and
// per item the session (in the pool, opened, holding a photo; ev given: the session of event i) and the window.  The same session may
// appear several times (tiles of one picture).
int session_view_check(ian_handle* h, const char* fn, int n, const ian_session_view* views, int vw, int vh, const uint8_t* out,
                       const ian_session_event* ev) {
  static_assert(sizeof(ian_session_view) == 3 * sizeof(int32_t), "ian_session_view is 3 words");
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if (S.capacity <= 0) return fail(h, -6, "%s: no session pool (call ian_sessions_reserve first)", fn);
  if (S.pool.scale <= 0) return fail(h, -6, "%s: no full-resolution reservation (call ian_sessions_reserve_hires first)", fn);
  if (n < 1 || n > BATCH_MAX) return fail(h, -7, "%s: n = %d outside 1..%d", fn, n, BATCH_MAX);
  if (!views || !out) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(views)) return fail(h, -7, "%s: the views must be a host array", fn);
  const int Sz = 64 * S.pool.scale;
  if (vw < 1 || vh < 1) return fail(h, -7, "%s: window %d x %d: both sizes must be at least 1", fn, vw, vh);
  if (vw & 3) return fail(h, -7, "%s: window width %d is not a multiple of 4", fn, vw);
  for (int i = 0; i < n; ++i) {
    const ian_session_view& v = views[i];
    if (v.session < 0 || v.session >= S.capacity)
      return fail(h, -7, "%s: item %d: session %d outside the pool (capacity %d)", fn, i, v.session, S.capacity);
    if (ev && ev[i].session != v.session)
      return fail(h, -7, "%s: item %d: the view names session %d, the event session %d", fn, i, v.session, ev[i].session);
    if (!S.opened[v.session]) return fail(h, -7, "%s: item %d: session %d has not been opened", fn, i, v.session);
    if (!S.has_src[v.session])
      return fail(h, -7, "%s: item %d: session %d has no full-resolution source (open it with ian_session_open_hires)", fn, i, v.session);
    if (v.x & 3) return fail(h, -7, "%s: item %d: window x %d is not a multiple of 4", fn, i, v.x);
    if (v.x < 0 || v.y < 0 || v.x > Sz - vw || v.y > Sz - vh)
      return fail(h, -7, "%s: item %d: window (%d,%d) + %d x %d outside the %d x %d picture", fn, i, v.x, v.y, vw, vh, Sz, Sz);
  }
  return 0;
}

// the windows of n views into d_out (device, u8[n,3,vh,vw]), or, d_out == nullptr, the whole picture over each session's own SRC
int session_render_enqueue(ian_handle* h, int n, const ian_session_view* views, int vw, int vh, unsigned char* d_out, hipStream_t st) {
  auto& S = h->sess;
  S.views_shadow.resize((size_t)3 * n);
  memcpy(S.views_shadow.data(), views, (size_t)n * sizeof(ian_session_view));
  HIPCHK(h, hipMemcpyAsync(S.d_views, S.views_shadow.data(), (size_t)n * sizeof(ian_session_view), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_session_render(S.pool, S.d_views, vw, vh, d_out, n, st));
  return 0;
}

// the device buffer a call renders into: the caller's, or the staging buffer grown to the call's size
int session_render_target(ian_handle* h, uint8_t* out, size_t bytes, unsigned char** d_out, bool* out_dev) {
  auto& S = h->sess;
  *out_dev = is_device_ptr(out);
  if (*out_dev) {
    *d_out = out;
    return 0;
  }
  int rc = grow_dev(h, &S.d_out, &S.out_cap, bytes);
  *d_out = S.d_out;
  return rc;
}

int session_open(ian_handle* h, int n, const int32_t* ids, const uint8_t* photos, int source, uint8_t* shown, void* stream, bool hires) {
  const char* fn = hires ? "ian_session_open_hires" : "ian_session_open";
  int rc = session_check(h, fn, n, ids, 1, photos == nullptr, false);
  if (rc) return rc;
  if (!photos && source != 0 && source != 1) return fail(h, -7, "%s: source %d (0 = from GIM, 1 = GIM := IM first)", fn, source);
  auto& S = h->sess;
  if (hires && S.pool.scale <= 0) return fail(h, -6, "%s: no full-resolution reservation (call ian_sessions_reserve_hires first)", fn);
  if (hires && !photos) return fail(h, -1, "null pointer passed to %s", fn);
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);
  TotalTimer tt(h, st);
  if ((rc = session_upload_ids(h, n, ids, st))) return rc;
  const unsigned char* d_photos = photos;
  const bool host_in = photos && !is_device_ptr(photos);
  if (host_in && hires) {   // straight into the sessions' SRC rows: no staging of n * 3 * S * S bytes
    const size_t row = sess_src_bytes(S.pool.scale);
    for (int i = 0; i < n; ++i)
      HIPCHK(h, hipMemcpyAsync(S.pool.src + (size_t)ids[i] * row, photos + (size_t)i * row, row, hipMemcpyHostToDevice, st));
    d_photos = nullptr;
  } else if (host_in) {
    if (!S.d_photo) HIPCHK(h, hipMalloc((void**)&S.d_photo, (size_t)BATCH_MAX * SESS_IMG));
    HIPCHK(h, hipMemcpyAsync(S.d_photo, photos, (size_t)n * SESS_IMG, hipMemcpyHostToDevice, st));
    d_photos = S.d_photo;
  }
  if (!photos && source == 1 && S.pool.scale > 0) {   // commit: what is displayed becomes the full-resolution photo as well
    std::vector<ian_session_view> whole;
    for (int i = 0; i < n; ++i)
      if (S.has_src[ids[i]]) whole.push_back(ian_session_view{ids[i], 0, 0});
    const int Sz = 64 * S.pool.scale;
    if (!whole.empty() && (rc = session_render_enqueue(h, (int)whole.size(), whole.data(), Sz, Sz, nullptr, st))) return rc;
  }
  Slot& xs = h->slots[h->desc.x_slot];
  Slot& zs = h->slots[h->desc.z_slot];
  Slot& out = h->slots[h->desc.out_slot];
  if ((rc = ensure_slot(h, h->desc.x_slot, n))) return rc;
  if (hires)
    HIPCHK(h, launch_session_hires_open(d_photos, S.pool, S.d_tab, S.d_tanh, xs.d, n, st));
  else
    HIPCHK(h, launch_session_open_in(d_photos, S.pool, S.d_tab, source, S.d_tanh, xs.d, n, st));
  h->slot_stale[h->desc.x_slot] = 0;
  // the very segments ian_encode and ian_decode_u8 run at this batch: Z and RECON are theirs bit for bit
  if ((rc = run_segment(h, IAN_SEG_ENC, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_IAF, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;
  h->slot_stale[h->desc.out_slot] = 0;
  const bool shown_dev = shown && is_device_ptr(shown);
  HIPCHK(h, launch_session_store(out.d, zs.d, zs.cs, S.pool, S.d_tab, 0, 0, shown ? (shown_dev ? shown : S.d_shown) : nullptr, n, st));
  if (S.pool.umask) HIPCHK(h, launch_session_local_set(S.pool, S.d_tab, nullptr, n, st));   // USER_MASK *= 0 (NPE.py:267, :337); LOCAL stays
  for (int i = 0; i < n; ++i) {
    S.opened[ids[i]] = 1;
    ++S.version[ids[i]];
    if (photos) S.has_src[ids[i]] = hires ? 1 : 0;   // a 64x64 photo leaves nothing at full resolution to edit
  }
  return session_finish(h, n, shown, shown_dev, host_in, st);
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
  const bool shown_dev = shown && is_device_ptr(shown);
  if (as_sample) {
    HIPCHK(h, launch_session_store(out.d, zs.d, zs.cs, S.pool, S.d_tab, 1, 1, shown ? (shown_dev ? shown : S.d_shown) : nullptr, n, st));
  } else {
    SessionBlendArgs a;
    memset(&a, 0, sizeof a);
    a.xhat = out.d; a.zslot = zs.d; a.zs = zs.cs; a.P = S.pool; a.ids = S.d_tab;
    a.shown = shown_dev ? shown : S.d_shown;
    a.store = 0;
    for (int i = 0; i < 8; ++i) a.w[i] = S.w[i];
    a.radius = S.radius;
    a.falloff = S.d_falloff; a.thresh = S.dampen_thresh;
    HIPCHK(h, launch_session_blend(a, n, st));
  }
  for (int i = 0; i < n; ++i) ++S.version[ids[i]];
  return session_finish(h, n, shown, shown_dev, host_in, st);
}

// with_view: ian_session_brush_view: after the brush, in the same submission, window i of session views[i].session (== ev[i].session)
// -> out, and one synchronisation for both results.
int session_brush(ian_handle* h, int n, const ian_session_event* ev, uint8_t* shown, void* stream, bool with_view = false,
                  const ian_session_view* views = nullptr, int vw = 0, int vh = 0, uint8_t* win = nullptr) {
  const char* fn = with_view ? "ian_session_brush_view" : "ian_session_brush";
  static_assert(sizeof(ian_session_event) == 11 * sizeof(int32_t), "ian_session_event is 11 words");
  int rc = session_check(h, fn, n, ev ? &ev->session : nullptr, 11, true, true);
  if (rc) return rc;
  Slot& out = h->slots[h->desc.out_slot];
  for (int i = 0; i < n; ++i) {
    const ian_session_event& e = ev[i];
    if (e.mode != 0 && e.mode != 1) return fail(h, -7, "%s: item %d has mode %d (0 = imgrad, 1 = imgradRGB toward rgb)", fn, i, e.mode);
    if (e.c1 < 0 || e.r1 < 0 || e.c2 > out.w || e.r2 > out.h)
      return fail(h, -7, "%s: item %d: patch (%d,%d,%d,%d) outside the %dx%d image", fn, i, e.c1, e.r1, e.c2, e.r2, out.w, out.h);
  }
  if ((rc = session_local_check(h, fn, n, &ev->session, 11))) return rc;
  auto& S = h->sess;
  unsigned char* d_out = nullptr;
  bool out_dev = false;
  const size_t out_bytes = (size_t)n * 3 * (size_t)(vh > 0 ? vh : 0) * (size_t)(vw > 0 ? vw : 0);
  if (with_view) {
    if ((rc = session_view_check(h, fn, n, views, vw, vh, win, ev))) return rc;
    if ((rc = session_render_target(h, win, out_bytes, &d_out, &out_dev))) return rc;
  }
  const int pass = h->opt.brush_pass;
  bool hit = n <= pass && S.res_valid && (int)S.res_ids.size() == n && getenv("IAN_NO_DEC_CACHE") == nullptr;
  for (int i = 0; hit && i < n; ++i) hit = S.res_ids[i] == ev[i].session && S.res_ver[i] == S.version[ev[i].session];
  hipStream_t st = (hipStream_t)stream;
  session_enter(h, st);   // also ends the residency: re-armed below
  TotalTimer tt(h, st);
  // the event table, rearranged for the kernels: n ian_brush_item records (the shared middle reads them), n ids, n colours
  S.tab_shadow.resize((size_t)11 * n);
  int32_t* t_items = S.tab_shadow.data();
  int32_t* t_ids = t_items + (size_t)7 * n;
  int32_t* t_col = t_ids + n;
  for (int i = 0; i < n; ++i) {
    memcpy(t_items + (size_t)7 * i, &ev[i].c1, 7 * sizeof(int32_t));   // c1 r1 c2 r2 mode coef gscale: ian_brush_item's layout
    t_ids[i] = ev[i].session;
    memcpy(t_col + (size_t)3 * i, ev[i].rgb, 3 * sizeof(float));
  }
  HIPCHK(h, hipMemcpyAsync(S.d_tab, S.tab_shadow.data(), (size_t)11 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int* d_items = S.d_tab;
  const int* d_ids = S.d_tab + (size_t)7 * n;
  const float* d_col = reinterpret_cast<const float*>(S.d_tab + (size_t)8 * n);
  Slot& zs = h->slots[h->desc.z_slot];
  const bool shown_dev = shown && is_device_ptr(shown);
  unsigned char* d_shown = shown_dev ? shown : S.d_shown;
  for (int off = 0; off < n; off += pass) {
    const int nc = std::min(pass, n - off);
    if (!hit) {
      if ((rc = ensure_slot(h, h->desc.z_slot, nc))) return rc;
      HIPCHK(h, launch_session_gather_z(S.pool, d_ids + off, zs.d, zs.cs, nc, st));
      if ((rc = batch_forward(h, nullptr, nc, st))) return rc;
    }
    if ((rc = brush_pass_middle(h, nc, d_items + (size_t)7 * off, nullptr, d_col + (size_t)3 * off, true, st))) return rc;
    SessionBlendArgs a;
    memset(&a, 0, sizeof a);
    a.xhat = out.d; a.zslot = zs.d; a.zs = zs.cs; a.P = S.pool; a.ids = d_ids + off; a.items = d_items + (size_t)7 * off;
    a.shown = d_shown + (size_t)off * SESS_IMG;
    a.store = 1;
    for (int i = 0; i < 8; ++i) a.w[i] = S.w[i];
    a.radius = S.radius;
    a.falloff = S.d_falloff; a.thresh = S.dampen_thresh;
    HIPCHK(h, launch_session_blend(a, nc, st));
  }
  h->slot_stale[h->desc.out_slot] = 0;
  for (int i = 0; i < n; ++i) ++S.version[ev[i].session];
  if (with_view && (rc = session_render_enqueue(h, n, views, vw, vh, d_out, st))) return rc;
  if ((rc = session_finish(h, n, shown, shown_dev, false, st, with_view && !out_dev ? win : nullptr, out_bytes))) return rc;
  if (n <= pass) {   // one pass: the resident activations belong to these sessions' new latents
    S.res_ids.resize(n);
    S.res_ver.resize(n);
    for (int i = 0; i < n; ++i) {
      S.res_ids[i] = ev[i].session;
      S.res_ver[i] = S.version[ev[i].session];
    }
    S.res_valid = true;
  }
  return 0;
}

int session_render(ian_handle* h, int n, const ian_session_view* views, int vw, int vh, uint8_t* out, void* stream) {
  const char* fn = "ian_session_render";
  int rc = session_view_check(h, fn, n, views, vw, vh, out, nullptr);
  if (rc) return rc;
  auto& S = h->sess;
  unsigned char* d_out = nullptr;
  bool out_dev = false;
  const size_t bytes = (size_t)n * 3 * (size_t)vh * (size_t)vw;
  if ((rc = session_render_target(h, out, bytes, &d_out, &out_dev))) return rc;
  // reads pool rows only, as ian_session_read: the decoder's activations and the residency of ian_session_brush survive it
  hipStream_t st = (hipStream_t)stream;
  if (h->last_pending && h->last_stream != st) HIPCHK(h, hipStreamSynchronize(h->last_stream));
  if ((rc = session_render_enqueue(h, n, views, vw, vh, d_out, st))) return rc;
  if (out_dev) {
    h->last_stream = st;
    h->last_pending = true;
  } else {
    HIPCHK(h, hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (h->last_stream == st) h->last_pending = false;
  }
  return 0;
}

int session_read(ian_handle* h, int id, int what, void* out, void* stream) {
  const char* fn = "ian_session_read";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  auto& S = h->sess;
  if (S.capacity <= 0) return fail(h, -6, "%s: no session pool (call ian_sessions_reserve first)", fn);
  if (!out) return fail(h, -1, "null pointer passed to %s", fn);
  if (id < 0 || id >= S.capacity) return fail(h, -7, "%s: session %d outside the pool (capacity %d)", fn, id, S.capacity);
  if (!S.opened[id]) return fail(h, -7, "%s: session %d has not been opened", fn, id);
  if (what >= IAN_SESSION_FIELD && what <= IAN_SESSION_SOURCE) {
    if (S.pool.scale <= 0) return fail(h, -6, "%s: no full-resolution reservation (call ian_sessions_reserve_hires first)", fn);
    if (what == IAN_SESSION_SOURCE && !S.has_src[id])
      return fail(h, -7, "%s: session %d has no full-resolution source (open it with ian_session_open_hires)", fn, id);
  }
  if ((what == IAN_SESSION_UMASK || what == IAN_SESSION_LOCAL) && !S.pool.umask)
    return fail(h, -6, "%s: no local reservation (call ian_sessions_reserve_local first)", fn);
  const void* src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case IAN_SESSION_Z: src = S.pool.z + (size_t)id * S.pool.zl; bytes = (size_t)S.pool.zl * sizeof(float); break;
    case IAN_SESSION_RECON: src = S.pool.recon + (size_t)id * SESS_IMG; bytes = SESS_IMG; break;
    case IAN_SESSION_ERROR: src = S.pool.error + (size_t)id * SESS_IMG; bytes = SESS_IMG * sizeof(float); break;
    case IAN_SESSION_IM: src = S.pool.im + (size_t)id * SESS_IMG; bytes = SESS_IMG; break;
    case IAN_SESSION_GIM: src = S.pool.gim + (size_t)id * SESS_IMG; bytes = SESS_IMG; break;
    case IAN_SESSION_MODE: src = S.pool.mode + id; bytes = sizeof(int32_t); break;
    case IAN_SESSION_FIELD: src = S.pool.field + (size_t)id * SESS_IMG; bytes = SESS_IMG * sizeof(float); break;
    case IAN_SESSION_FIELD_KIND: src = S.pool.kind + id; bytes = sizeof(int32_t); break;
    case IAN_SESSION_SOURCE: bytes = sess_src_bytes(S.pool.scale); src = S.pool.src + (size_t)id * bytes; break;
    case IAN_SESSION_UMASK: src = S.pool.umask + (size_t)id * (64 * 64); bytes = SESS_UMASK; break;
    case IAN_SESSION_LOCAL: src = S.pool.local + id; bytes = sizeof(int32_t); break;
    default: return fail(h, -7, "%s: field %d (enum ian_session_field)", fn, what);
  }
  // a plain copy of pool rows: the decoder's activations are not touched, so the residency of ian_session_brush survives it
  hipStream_t st = (hipStream_t)stream;
  if (h->last_pending && h->last_stream != st) HIPCHK(h, hipStreamSynchronize(h->last_stream));
  const bool dev = is_device_ptr(out);
  HIPCHK(h, hipMemcpyAsync(out, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (dev) {
    h->last_stream = st;
    h->last_pending = true;
  } else {
    HIPCHK(h, hipStreamSynchronize(st));
    if (h->last_stream == st) h->last_pending = false;
  }
  return 0;
}

}  // namespace

extern "C" {

int ian_sessions_reserve(ian_handle* h, int32_t capacity) {
  if (!h) return -1;
  return sessions_reserve(h, capacity);
}
int ian_sessions_set_blend(ian_handle* h, const double* gauss_half, int32_t radius) { return sessions_set_blend(h, gauss_half, radius); }
int ian_session_open(ian_handle* h, int32_t n, const int32_t* ids, const uint8_t* photos, int32_t source, uint8_t* shown, void* stream) {
  if (!h) return -1;
  return session_open(h, n, ids, photos, source, shown, stream, false);
}
int ian_sessions_reserve_hires(ian_handle* h, int32_t scale) {
  if (!h) return -1;
  return sessions_reserve_hires(h, scale);
}
int ian_session_open_hires(ian_handle* h, int32_t n, const int32_t* ids, const uint8_t* photos, uint8_t* shown, void* stream) {
  if (!h) return -1;
  return session_open(h, n, ids, photos, 0, shown, stream, true);
}
int ian_session_render(ian_handle* h, int32_t n, const ian_session_view* views, int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  if (!h) return -1;
  return session_render(h, n, views, vw, vh, out, stream);
}
int ian_session_brush_view(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, const ian_session_view* views,
                           int32_t vw, int32_t vh, uint8_t* out, void* stream) {
  if (!h) return -1;
  return session_brush(h, n, events, shown, stream, true, views, vw, vh, out);
}
int ian_session_set_latent(ian_handle* h, int32_t n, const int32_t* ids, const float* z, int32_t as_sample, uint8_t* shown, void* stream) {
  if (!h) return -1;
  return session_set_latent(h, n, ids, z, as_sample, shown, stream);
}
int ian_session_brush(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, void* stream) {
  if (!h) return -1;
  return session_brush(h, n, events, shown, stream);
}
int ian_session_read(ian_handle* h, int32_t id, int32_t what, void* out, void* stream) {
  if (!h) return -1;
  return session_read(h, id, what, out, stream);
}
int ian_sessions_reserve_local(ian_handle* h, int32_t on) {
  if (!h) return -1;
  return sessions_reserve_local(h, on);
}
int ian_sessions_set_local(ian_handle* h, const double* falloff64, double dampen_thresh) {
  if (!h) return -1;
  return sessions_set_local(h, falloff64, dampen_thresh);
}
int ian_session_local(ian_handle* h, int32_t n, const int32_t* ids, const int32_t* flags, void* stream) {
  if (!h) return -1;
  return session_local(h, n, ids, flags, stream);
}
void ian_session_tanh_table(float* out256) {
  if (out256) session_tanh_table(out256);
}

}  // extern "C"
