// ian_rt_edit.inc -- stream hand-over, captured graphs of the interactive loop, decoder cache, photo blend.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
namespace {

// ----- stream hand-over between calls ------------------------------------------------------------------------
// The handle's buffers are shared by every call; a call that returns without synchronising (device output pointers)
// leaves work pending on its stream.  When the next call runs on ANOTHER stream, wait for that work first.
constexpr int PIN_WARM_FLAG = 256 + 3 * 64 * 64 + 7;   // int slot of the pinned block the keep-warm kernel polls (behind the 7 brush words)
void warm_release(ian_handle* h) {
  if (!h->warm_armed) return;
  reinterpret_cast<volatile int*>(h->pin)[PIN_WARM_FLAG] = 1;   // mapped + coherent: the spinning wave sees it and exits
  h->warm_armed = false;
}
void enter_stream(ian_handle* h, hipStream_t st) {
  warm_release(h);     // whatever comes next must not queue behind the keep-warm kernel
  h->batch.cache_valid = false;   // the batched calls' resident activations survive only until the next call
  h->sess.res_valid = false;      // ... and so do those of ian_session_brush
  if (h->last_pending && h->last_stream != st) (void)hipStreamSynchronize(h->last_stream);
  h->last_stream = st;
  h->last_pending = true;   // cleared by callers that synchronise before returning
}

// ----- captured graphs for the interactive loop ----------------------------------------------------------------
constexpr int PIN_Z = 0, PIN_DZ = 128, PIN_IMG = 256, PIN_BRUSH = 256 + 3 * 64 * 64, PIN_FLOATS = PIN_BRUSH + 8;
// The single event's brush words, in the pinned block and in h->d_patch, are one row of the batched calls' table: the seed kernels
// read the rectangle and loss kind from it, the latent update (coef, gscale) at words 5 and 6.
static_assert(sizeof(ian_brush_item) == 7 * sizeof(int32_t) && PIN_WARM_FLAG == PIN_BRUSH + 7, "brush words: one ian_brush_item, then the keep-warm flag");
ian_brush_item* pin_brush_item(ian_handle* h) { return reinterpret_cast<ian_brush_item*>(h->pin + PIN_BRUSH); }
constexpr int BRUSH_CG = 5;   // word of coef in an ian_brush_item row; gscale follows

bool edit_graph_eligible(const ian_handle* h, void* stream, std::initializer_list<const void*> host_ptrs) {
  if (!h->opt.edit_graph || h->prof || stream != nullptr || h->graph_failed || h->desc.num_latents > 128) return false;
  const Slot& os = h->slots[h->desc.out_slot];
  if (os.per_image() > 3 * 64 * 64) return false;
  for (const void* p : host_ptrs)
    if (p && is_device_ptr(p)) return false;
  return true;
}

// End of an interactive call: the host needs the results NOW.  hipStreamSynchronize may park the thread on an interrupt (the
// wake-up is what costs); the calls of the edit loop last 0.1-0.2 ms, so poll the stream for at most ~2 ms first.
hipError_t wait_edit_stream(ian_handle* h, hipStream_t st) {
  if (h->opt.edit_spin) {
    for (int i = 0; i < 20000; ++i) {
      const hipError_t e = hipStreamQuery(st);
      if (e == hipSuccess) return hipSuccess;
      if (e != hipErrorNotReady) break;
    }
    (void)hipGetLastError();
  }
  return hipStreamSynchronize(st);
}

bool zero_copy(const ian_handle* h) { return h->pin_dev != nullptr && h->opt.edit_zero_copy != 0; }

int edit_ctx(ian_handle* h) {
  if (h->edit_stream) return 0;
  HIPCHK(h, hipStreamCreateWithFlags(&h->edit_stream, hipStreamNonBlocking));
  // mapped + coherent: kernels of the captured graphs address the block directly (zero-copy); when the runtime refuses the
  // flags or the device pointer, fall back to a plain pinned block and keep the copy nodes
  if (hipHostMalloc((void**)&h->pin, PIN_FLOATS * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, h->pin, 0) == hipSuccess && dp) h->pin_dev = (float*)dp;
    else (void)hipGetLastError();
  } else {
    (void)hipGetLastError();
    HIPCHK(h, hipHostMalloc((void**)&h->pin, PIN_FLOATS * sizeof(float), hipHostMallocDefault));
  }
  memset(h->pin, 0, PIN_FLOATS * sizeof(float));
  HIPCHK(h, hipMalloc((void**)&h->d_patch, 8 * sizeof(int)));   // brush rectangle + (coef, gscale) of ian_brush_step
  if (128 > h->stage_in_cap) {
    if (h->d_stage_in) HIPCHK(h, hipFree(h->d_stage_in));
    HIPCHK(h, hipMalloc((void**)&h->d_stage_in, 128 * sizeof(float)));
    h->stage_in_cap = 128;
  }
  if (128 > h->stage_out_cap) {
    if (h->d_stage_out) HIPCHK(h, hipFree(h->d_stage_out));
    HIPCHK(h, hipMalloc((void**)&h->d_stage_out, 128 * sizeof(float)));
    h->stage_out_cap = 128;
  }
  ++h->alloc_epoch;
  return 0;
}

// Run `body` (a fixed sequence of launches / async copies on h->edit_stream): eagerly the first times (allocations,
// schedule uploads, function attributes happen there), then captured once, then replayed.
template <typename F>
int run_or_replay(ian_handle* h, ian_handle::EditGraph& G, F&& body) {
  hipStream_t st = h->edit_stream;
  if (G.exec && G.epoch == h->alloc_epoch) {
    HIPCHK(h, hipGraphLaunch(G.exec, st));
    return 0;
  }
  if (G.exec) {
    (void)hipGraphExecDestroy(G.exec);
    G.exec = nullptr;
    G.warm = 0;
  }
  if (G.warm < 1 || G.warm_epoch != h->alloc_epoch || h->graph_failed) {
    // a capture must replay exactly what an eager pass has already done once: first launches set function attributes,
    // build and upload schedules, allocate -- none of which may happen inside a capture.  An option change or a
    // (re)allocation between the eager pass and the capture (alloc_epoch moved) therefore asks for another eager pass.
    const long long e0 = h->alloc_epoch;
    const int rc = body();
    G.warm = (h->alloc_epoch == e0) ? 1 : 0;
    G.warm_epoch = h->alloc_epoch;
    return rc;
  }
  const long long e0 = h->alloc_epoch;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    h->graph_failed = true;
    return body();
  }
  const int rc = body();
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(st, &g);
  if (rc || e != hipSuccess || !g || h->alloc_epoch != e0) {   // never replay a graph whose capture hit an error or an allocation
    (void)hipGetLastError();
    if (g) (void)hipGraphDestroy(g);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {   // an invalidated capture may still hold the stream
      hipGraph_t g2 = nullptr;
      (void)hipStreamEndCapture(st, &g2);
      if (g2) (void)hipGraphDestroy(g2);
    }
    (void)hipGetLastError();
    h->graph_failed = true;
    h->err.clear();
    return body();
  }
  const hipError_t ei = hipGraphInstantiate(&G.exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess) {
    (void)hipGetLastError();
    G.exec = nullptr;
    h->graph_failed = true;
    return body();
  }
  G.epoch = h->alloc_epoch;
  HIPCHK(h, hipGraphLaunch(G.exec, st));
  return 0;
}

bool dec_cache_hit(const ian_handle* h, const float* z) {
  return h->dec_cache_valid && !is_device_ptr(z) && getenv("IAN_NO_DEC_CACHE") == nullptr &&
         memcmp(h->dec_cache_z.data(), z, sizeof(float) * h->desc.num_latents) == 0;
}

// batch-1 decoder forward for the HOST latent z on the internal stream (graph replay), unless the resident activations
// already belong to it
int decode_one_graph(ian_handle* h, const float* z) {
  if (dec_cache_hit(h, z)) return 0;
  h->dec_cache_valid = false;
  int rc;
  if ((rc = ensure_slot(h, h->desc.z_slot, 1))) return rc;
  const int zl = h->desc.num_latents;
  memcpy(h->pin + PIN_Z, z, zl * sizeof(float));
  hipStream_t st = h->edit_stream;
  h->pin_img_valid = false;
  rc = run_or_replay(h, h->g_fwd, [&]() -> int {
    Slot& zs = h->slots[h->desc.z_slot];
    // one row: straight into the slot (its channel padding beyond num_latents stays zero), no staging kernel
    HIPCHK(h, hipMemcpyAsync(zs.d, h->pin + PIN_Z, zl * sizeof(float), hipMemcpyHostToDevice, st));
    h->out_mirror = zero_copy(h) ? h->pin_dev + PIN_IMG : nullptr;   // the image kernel also writes the pinned image (no copy node)
    const int r = run_segment(h, IAN_SEG_DEC, 1, st);
    h->out_mirror = nullptr;
    h->g_fwd.mirrors = h->pin_img_valid;    // set by the image kernel's launch site when it took the mirror
    return r;
  });
  if (rc) return rc;
  h->pin_img_valid = h->g_fwd.mirrors;      // also on a replay, which does not run the body
  h->dec_cache_z.assign(z, z + zl);
  h->dec_cache_valid = true;
  return 0;
}

// batch-1 decoder forward for latent z unless the resident activations already belong to it (NPE.py:205,218:
// imgradRGB(z) right after sample_at(z), the blend right after the brush step)
int decode_one_cached(ian_handle* h, const float* z, hipStream_t st) {
  int rc;
  const bool host_z = !is_device_ptr(z);
  if (!dec_cache_hit(h, z)) {
    h->dec_cache_valid = false;
    if ((rc = set_latent_input(h, h->desc.z_slot, z, 1, st))) return rc;
    if ((rc = run_segment(h, IAN_SEG_DEC, 1, st))) return rc;
    if (host_z) {
      h->dec_cache_z.assign(z, z + h->desc.num_latents);
      h->dec_cache_valid = true;
    }
  }
  return 0;
}

int upload_rgb_if_changed(ian_handle* h, const float* rgb, hipStream_t st, const float** d_rgb) {
  Slot& out = h->slots[h->desc.out_slot];
  const size_t cnt = out.per_image();
  if (is_device_ptr(rgb)) {
    *d_rgb = rgb;
    return 0;
  }
  if (!h->d_rgb) {
    HIPCHK(h, hipMalloc((void**)&h->d_rgb, cnt * sizeof(float)));
    ++h->alloc_epoch;
  }
  // the brush colour image rarely changes between motion events (NPE.py:205 passes the same myRGB): re-upload only when
  // the host bytes differ from the last upload
  if (h->rgb_cache.size() != cnt || memcmp(h->rgb_cache.data(), rgb, cnt * sizeof(float)) != 0) {
    h->rgb_cache.assign(rgb, rgb + cnt);   // the shadow copy is the upload source: it outlives the caller's buffer
    HIPCHK(h, hipMemcpyAsync(h->d_rgb, h->rgb_cache.data(), cnt * sizeof(float), hipMemcpyHostToDevice, st));
  }
  *d_rgb = h->d_rgb;
  return 0;
}

int grad_common(ian_handle* h, int mode, int c1, int r1, int c2, int r2, const float* rgb, const float* z, float* dz,
                void* stream) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if (!z || !dz) return fail(h, -1, "null pointer passed to ian_grad_*");
  Slot& zs = h->slots[h->desc.z_slot];
  if (edit_graph_eligible(h, stream, {z, dz, rgb})) {
    if ((rc = check_rect(h, nullptr, 0, c1, r1, c2, r2, "patch"))) return rc;
    if ((rc = edit_ctx(h))) return rc;
    hipStream_t st = h->edit_stream;
    enter_stream(h, st);
    if ((rc = decode_one_graph(h, z))) return rc;
    const float* d_rgb = nullptr;
    if (mode == 1 && (rc = upload_rgb_if_changed(h, rgb, st, &d_rgb))) return rc;
    if ((rc = ensure_slot(h, h->desc.z_slot, 1, true))) return rc;
    ian_brush_item* item = pin_brush_item(h);
    item->c1 = c1; item->r1 = r1; item->c2 = c2; item->r2 = r2; item->mode = mode;
    rc = run_or_replay(h, h->g_bwd[mode], [&]() -> int {
      BrushBackward rq;
      rq.seed.rgb = d_rgb;
      if (zero_copy(h)) rq.seed.table = reinterpret_cast<const int*>(h->pin_dev + PIN_BRUSH);   // read in place: no copy node
      else {
        HIPCHK(h, hipMemcpyAsync(h->d_patch, item, 5 * sizeof(int), hipMemcpyHostToDevice, st));
        rq.seed.table = h->d_patch;
      }
      int r = run_decoder_backward(h, rq, st);
      if (r) return r;
      HIPCHK(h, hipMemcpyAsync(h->pin + PIN_DZ, zs.g, zs.c * sizeof(float), hipMemcpyDeviceToHost, st));
      return 0;
    });
    if (rc) return rc;
    HIPCHK(h, wait_edit_stream(h, st));
    h->last_pending = false;
    memcpy(dz, h->pin + PIN_DZ, zs.c * sizeof(float));
    return 0;
  }
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  TotalTimer tt(h, st);
  if ((rc = decode_one_cached(h, z, st))) return rc;
  const float* d_rgb = nullptr;
  if (mode == 1 && (rc = upload_rgb_if_changed(h, rgb, st, &d_rgb))) return rc;
  BrushBackward rq;   // no table: the rectangle travels in the launch
  rq.seed.c1 = c1; rq.seed.r1 = r1; rq.seed.c2 = c2; rq.seed.r2 = r2; rq.seed.mode = mode;
  rq.seed.rgb = d_rgb;
  if ((rc = run_decoder_backward(h, rq, st))) return rc;
  // result sits in the gradient buffer of the z slot
  if (is_device_ptr(dz)) {
    HIPCHK(h, launch_rows_copy(zs.g, zs.cs, dz, zs.c, 1, zs.c, st));
  } else {
    if ((size_t)zs.c > h->stage_out_cap) {
      if (h->d_stage_out) HIPCHK(h, hipFree(h->d_stage_out));
      HIPCHK(h, hipMalloc((void**)&h->d_stage_out, zs.c * sizeof(float)));
      h->stage_out_cap = zs.c;
      ++h->alloc_epoch;
    }
    HIPCHK(h, launch_rows_copy(zs.g, zs.cs, h->d_stage_out, zs.c, 1, zs.c, st));
    HIPCHK(h, hipMemcpyAsync(dz, h->d_stage_out, zs.c * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->last_pending = false;
  }
  return 0;
}

// NPE.py:218-231 for the image resident in the output slot: (cached) uploads of RECON / ERROR, the blend kernel, copies
// back.  *pending = a host copy was enqueued (the caller synchronises).
int enqueue_photo_blend(ian_handle* h, const uint8_t* recon, const float* error, const double* gauss_half, int radius, uint8_t* im,
                        double* mask, hipStream_t st, bool* pending) {
  if (!recon || !error || !gauss_half || !im) return fail(h, -1, "null pointer passed to the photo blend");
  if (radius < 0 || radius > 7) return fail(h, -7, "photo blend: radius %d outside 0..7", radius);
  Slot& os = h->slots[h->desc.out_slot];
  if (os.h != 64 || os.w != 64 || os.c != 3) return fail(h, -7, "the photo blend needs a 3x64x64 image");
  const size_t cnt = 3 * 64 * 64;
  PhotoBlendArgs a;
  memset(&a, 0, sizeof a);
  a.xhat = os.d;
  if (is_device_ptr(recon)) a.recon = recon;
  else {
    if (!h->d_recon) HIPCHK(h, hipMalloc((void**)&h->d_recon, cnt));
    if (h->recon_cache.size() != cnt || memcmp(h->recon_cache.data(), recon, cnt) != 0) {   // changes on infer / Reset only
      h->recon_cache.assign(recon, recon + cnt);
      HIPCHK(h, hipMemcpyAsync(h->d_recon, h->recon_cache.data(), cnt, hipMemcpyHostToDevice, st));
    }
    a.recon = h->d_recon;
  }
  if (is_device_ptr(error)) a.error = error;
  else {
    if (!h->d_error) HIPCHK(h, hipMalloc((void**)&h->d_error, cnt * sizeof(float)));
    if (h->error_cache.size() != cnt || memcmp(h->error_cache.data(), error, cnt * sizeof(float)) != 0) {
      h->error_cache.assign(error, error + cnt);
      HIPCHK(h, hipMemcpyAsync(h->d_error, h->error_cache.data(), cnt * sizeof(float), hipMemcpyHostToDevice, st));
    }
    a.error = h->d_error;
  }
  const bool im_dev = is_device_ptr(im), mask_dev = mask && is_device_ptr(mask);
  if (!im_dev && !h->d_im) HIPCHK(h, hipMalloc((void**)&h->d_im, cnt));
  if (mask && !mask_dev && !h->d_mask) HIPCHK(h, hipMalloc((void**)&h->d_mask, 64 * 64 * sizeof(double)));
  a.im = im_dev ? im : h->d_im;
  a.mask = mask ? (mask_dev ? mask : h->d_mask) : nullptr;
  for (int i = 0; i <= radius; ++i) a.w[i] = gauss_half[i];
  a.radius = radius;
  HIPCHK(h, launch_photo_blend(a, st));
  if (!im_dev) HIPCHK(h, hipMemcpyAsync(im, h->d_im, cnt, hipMemcpyDeviceToHost, st));
  if (mask && !mask_dev) HIPCHK(h, hipMemcpyAsync(mask, h->d_mask, 64 * 64 * sizeof(double), hipMemcpyDeviceToHost, st));
  *pending = !im_dev || (mask && !mask_dev);
  return 0;
}

// ----- several editors: n brush events in one submission (ian_grad_batch / ian_brush_step_batch) ----------------------------
// buffers of the batched calls only: no captured batch-1 graph references them, so growing one does not move alloc_epoch
template <typename T>
int grow_dev(ian_handle* h, T** p, size_t* cap, size_t need, bool* grew = nullptr) {
  if (grew) *grew = false;
  if (need <= *cap) return 0;
  if (*p) HIPCHK(h, hipFree(*p));
  *p = nullptr;
  *cap = 0;
  HIPCHK(h, hipMalloc((void**)p, need * sizeof(T)));
  *cap = need;
  if (grew) *grew = true;
  return 0;
}

// a host input goes up only when its bytes differ from the last upload (the shadow copy is the upload source); device inputs are
// used in place
template <typename T>
int upload_batch_cached(ian_handle* h, const T* src, size_t cnt, T** d, size_t* cap, std::vector<T>& shadow, hipStream_t st,
                        const T** out) {
  if (is_device_ptr(src)) {
    *out = src;
    return 0;
  }
  bool grew = false;
  int rc = grow_dev(h, d, cap, cnt, &grew);
  if (rc) return rc;
  if (grew || shadow.size() != cnt || memcmp(shadow.data(), src, cnt * sizeof(T)) != 0) {
    shadow.assign(src, src + cnt);
    HIPCHK(h, hipMemcpyAsync(*d, shadow.data(), cnt * sizeof(T), hipMemcpyHostToDevice, st));
  }
  *out = *d;
  return 0;
}

constexpr int BATCH_MAX = 256;

// The decoder's forward at batch nc with every layer's activation kept (the backward sweep reads them), its output written.
int batch_forward(ian_handle* h, const float* z, int nc, hipStream_t st) {
  int rc;
  if (z && (rc = set_latent_input(h, h->desc.z_slot, z, nc, st))) return rc;
  h->keep_layer_acts = true;
  rc = run_segment(h, IAN_SEG_DEC, nc, st);
  h->keep_layer_acts = false;
  if (rc) return rc;
  for (auto& op : h->ops) {   // every activation the backward sweep may read holds nc images (no kernel may run past a buffer)
    if (op.d.segment != IAN_SEG_DEC) continue;
    for (int sl : {op.d.src, op.d.src2, op.d.src3, op.d.dst}) {
      if (sl < 0) continue;
      const Slot& s = h->slots[sl];
      if (!s.d || s.cap < s.per_image() * (size_t)nc) return fail(h, -9, "batched brush: activation of slot %d was not materialised", sl);
    }
  }
  return 0;
}

// What every batched brush call runs between "the latent slot holds nc latents and the decoder's activations belong to them" and its
// outputs: the batched seed + backward sweep (seed: the nc rows of the item table and where their targets come from -- rgb: [nc,3,H,W]
// colour images, colour: [nc][3] constant colours, or gim / ids / tanh_tab: the sessions' own photos) and, for a step, the brush
// update (fused into the latent's GEMV where that form is taken) and the forward at z_new.  Without a step the latents' gradient
// rows are left in the z slot's gradient buffer.  Shared by batch_common and the session calls (ian_rt_session.inc).
int brush_pass_middle(ian_handle* h, int nc, const BrushSeedSrc& seed, bool step, hipStream_t st) {
  int rc;
  Slot& zs = h->slots[h->desc.z_slot];
  if ((rc = ensure_slot(h, h->desc.z_slot, nc, true))) return rc;
  const int* d_it = seed.table;
  BrushBackward rq;
  rq.seed = seed;
  rq.n = nc;
  rq.batch = true;
  rq.update = step ? BrushBackward::PER_ITEM : BrushBackward::NONE;
  if ((rc = run_decoder_backward(h, rq, st))) return rc;
  if (step) {
    if (!rq.updated) HIPCHK(h, launch_latent_update_batch(zs.d, zs.g, zs.cs, d_it, nc, h->desc.num_latents, st));
    if ((rc = batch_forward(h, nullptr, nc, st))) return rc;   // sample_at(z_new)
  }
  return 0;
}

// Item i is one single-image call on (z[i], items[i], rgb[i]).  Per pass of at most opt.brush_pass items: the decoder forward (skipped when
// the activations the previous ian_brush_step_batch left resident belong to these very latents), the batched seed + backward sweep,
// [the brush update fused into the latent's GEMV and the forward at z_new,] [the batched photo blend].  Then the outputs, with one
// synchronisation when any of them is host memory.  All launches on the caller's stream.
int batch_common(ian_handle* h, int n, const ian_brush_item* items, const float* rgb, const float* z, float* z_new, float* dz, float* x,
                 const ian_photo_batch_args* photo, void* stream, bool step) {
  const char* fn = step ? "ian_brush_step_batch" : "ian_grad_batch";
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if (n < 1 || n > BATCH_MAX) return fail(h, -7, "%s: n = %d outside 1..%d", fn, n, BATCH_MAX);
  if (!items || !z || (step ? !z_new : !dz)) return fail(h, -1, "null pointer passed to %s", fn);
  if (is_device_ptr(items)) return fail(h, -7, "%s: items must be a host array", fn);
  Slot& out = h->slots[h->desc.out_slot];
  bool any_rgb = false;
  for (int i = 0; i < n; ++i) {   // everything is checked before anything is enqueued or written
    const ian_brush_item& it = items[i];
    if (it.mode != 0 && it.mode != 1) return fail(h, -7, "%s: item %d has mode %d (0 = imgrad, 1 = imgradRGB)", fn, i, it.mode);
    if (it.mode == 1 && !rgb) return fail(h, -1, "%s: item %d has mode 1 (imgradRGB) but rgb is NULL", fn, i);
    if ((rc = check_rect(h, fn, i, it.c1, it.r1, it.c2, it.r2, "patch"))) return rc;
    any_rgb = any_rgb || it.mode == 1;
  }
  if (photo) {
    if (!photo->recon || !photo->error || !photo->gauss_half || !photo->im) return fail(h, -1, "null pointer passed to the photo blend of %s", fn);
    if (photo->radius < 0 || photo->radius > 7) return fail(h, -7, "%s: photo blend radius %d outside 0..7", fn, photo->radius);
    if (out.h != 64 || out.w != 64 || out.c != 3) return fail(h, -7, "%s: the photo blend needs a 3x64x64 image", fn);
  }
  if (photo && is_device_ptr(photo->gauss_half)) return fail(h, -7, "%s: gauss_half must be a host array", fn);
  const int pass = h->opt.brush_pass;   // items per forward / backward / forward pass
  const int zl = h->desc.num_latents;
  Slot& zs = h->slots[h->desc.z_slot];
  const size_t img = out.per_image();
  auto& B = h->batch;
  const bool hit = n <= pass && !is_device_ptr(z) && B.cache_valid && B.cache_n == n && getenv("IAN_NO_DEC_CACHE") == nullptr &&
                   memcmp(B.cache_z.data(), z, (size_t)n * zl * sizeof(float)) == 0;
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);   // also ends the resident-activation cache: re-armed below when this call leaves z_new resident
  TotalTimer tt(h, st);
  h->dec_cache_valid = false;   // the batch-1 activations are overwritten
  h->pin_img_valid = false;
  size_t items_cap = B.d_items ? (size_t)BATCH_MAX * 7 : 0;
  if ((rc = grow_dev(h, &B.d_items, &items_cap, (size_t)BATCH_MAX * 7))) return rc;
  B.items_shadow.assign(reinterpret_cast<const int32_t*>(items), reinterpret_cast<const int32_t*>(items) + (size_t)7 * n);
  HIPCHK(h, hipMemcpyAsync(B.d_items, B.items_shadow.data(), (size_t)7 * n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const float* d_rgb = nullptr;
  if (any_rgb && (rc = upload_batch_cached(h, rgb, (size_t)n * img, &B.d_rgb, &B.rgb_cap, B.rgb_cache, st, &d_rgb))) return rc;
  PhotoBlendArgs pa;
  memset(&pa, 0, sizeof pa);
  const bool im_dev = photo && is_device_ptr(photo->im), mask_dev = photo && photo->mask && is_device_ptr(photo->mask);
  if (photo) {
    if ((rc = upload_batch_cached(h, photo->recon, (size_t)n * img, &B.d_recon, &B.recon_cap, B.recon_cache, st, &pa.recon))) return rc;
    if ((rc = upload_batch_cached(h, photo->error, (size_t)n * img, &B.d_error, &B.error_cap, B.error_cache, st, &pa.error))) return rc;
    if (!im_dev && (rc = grow_dev(h, &B.d_im, &B.im_cap, (size_t)BATCH_MAX * img))) return rc;
    if (photo->mask && !mask_dev && (rc = grow_dev(h, &B.d_mask, &B.mask_cap, (size_t)BATCH_MAX * 64 * 64))) return rc;
    for (int i = 0; i <= photo->radius; ++i) pa.w[i] = photo->gauss_half[i];
    pa.radius = photo->radius;
  }
  if ((rc = grow_dev(h, &B.d_out, &B.out_cap, (size_t)2 * BATCH_MAX * zl))) return rc;
  float* st_z = B.d_out;                           // staging of host outputs: z_new rows | dz rows
  float* st_g = B.d_out + (size_t)BATCH_MAX * zl;
  const bool z_new_dev = step && is_device_ptr(z_new), dz_dev = dz && is_device_ptr(dz), x_dev = x && is_device_ptr(x);
  for (int off = 0; off < n; off += pass) {
    const int nc = std::min(pass, n - off);
    const size_t zo = (size_t)off * zl, io = (size_t)off * img;
    if (!hit && (rc = batch_forward(h, z + zo, nc, st))) return rc;
    const int* d_it = B.d_items + (size_t)7 * off;
    BrushSeedSrc seed;
    seed.table = d_it;
    seed.rgb = d_rgb ? d_rgb + io : nullptr;
    if ((rc = brush_pass_middle(h, nc, seed, step, st))) return rc;
    if (step) {
      HIPCHK(h, launch_rows_copy(zs.d, zs.cs, z_new_dev ? z_new + zo : st_z + zo, zl, nc, zl, st));
    }
    if (dz) HIPCHK(h, launch_rows_copy(zs.g, zs.cs, dz_dev ? dz + zo : st_g + zo, zl, nc, zl, st));
    if (x) HIPCHK(h, hipMemcpyAsync(x + io, out.d, (size_t)nc * img * sizeof(float), x_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (photo) {
      PhotoBlendArgs a = pa;
      a.xhat = out.d;
      a.recon += io;
      a.error += io;
      a.im = (im_dev ? photo->im : B.d_im) + io;
      a.mask = photo->mask ? (mask_dev ? photo->mask : B.d_mask) + (size_t)off * 64 * 64 : nullptr;
      HIPCHK(h, launch_photo_blend_batch(a, nc, st));
    }
  }
  h->slot_stale[h->desc.out_slot] = 0;
  bool host_out = x && !x_dev;
  if (step && !z_new_dev) HIPCHK(h, hipMemcpyAsync(z_new, st_z, (size_t)n * zl * sizeof(float), hipMemcpyDeviceToHost, st));
  if (dz && !dz_dev) HIPCHK(h, hipMemcpyAsync(dz, st_g, (size_t)n * zl * sizeof(float), hipMemcpyDeviceToHost, st));
  host_out = host_out || (step && !z_new_dev) || (dz && !dz_dev);
  if (photo) {
    if (!im_dev) HIPCHK(h, hipMemcpyAsync(photo->im, B.d_im, (size_t)n * img, hipMemcpyDeviceToHost, st));
    if (photo->mask && !mask_dev)
      HIPCHK(h, hipMemcpyAsync(photo->mask, B.d_mask, (size_t)n * 64 * 64 * sizeof(double), hipMemcpyDeviceToHost, st));
    host_out = host_out || !im_dev || (photo->mask && !mask_dev);
  }
  if (host_out) {
    HIPCHK(h, hipStreamSynchronize(st));
    h->last_pending = false;
  }
  if (step && n <= pass && !z_new_dev) {   // one pass: the resident activations belong to z_new, the next event skips its forward
    B.cache_z.assign(z_new, z_new + (size_t)n * zl);
    B.cache_n = n;
    B.cache_valid = true;
  }
  return 0;
}
}  // namespace
