// ian_rt_api.inc -- C ABI of include/ian.h.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
// =========================================== C ABI ====================================================
extern "C" {

const char* ian_version(void) {
#ifdef IAN_ABLATION
  return "libian 0.2 (gfx950, ablation: negative-result variants compiled in -- NOT the product library)";
#else
  return "libian 0.2 (gfx950)";
#endif
}

int ian_box_probe(int32_t iters, int32_t launches, double* tflops, double* us_per_launch, void* stream) {
  if (iters <= 0 || launches <= 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = 512;                       // 2 workgroups x 4 waves per CU on 256 CUs
  const size_t n = (size_t)blocks * 256;
  std::vector<float> hbuf(n * 4);
  unsigned lcg = 12345u;
  for (auto& v : hbuf) {
    lcg = lcg * 1664525u + 1013904223u;
    v = ((float)(lcg >> 8) / 16777216.f) * 0.02f - 0.01f;
  }
  float *din = nullptr, *dout = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  int rc = 0;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && !rc) rc = -(int)e - 1000; return e == hipSuccess; };
  if (chk(hipMalloc(&din, n * 4 * sizeof(float))) && chk(hipMalloc(&dout, n * sizeof(float))) &&
      chk(hipMemcpyAsync(din, hbuf.data(), n * 4 * sizeof(float), hipMemcpyHostToDevice, st)) && chk(hipEventCreate(&a)) &&
      chk(hipEventCreate(&b))) {
    for (int w = 0; w < 3 && !rc; ++w) chk(ian::launch_box_probe(din, dout, blocks, iters, st));   // warm-up
    chk(hipEventRecord(a, st));
    for (int r = 0; r < launches && !rc; ++r) chk(ian::launch_box_probe(din, dout, blocks, iters, st));
    chk(hipEventRecord(b, st));
    chk(hipEventSynchronize(b));
    float ms = 0;
    if (!rc && chk(hipEventElapsedTime(&ms, a, b)) && ms > 0) {
      const double flops = (double)blocks * 4.0 /*waves*/ * 4.0 /*MFMAs per iteration*/ * (double)iters * 4096.0 * (double)launches;
      if (tflops) *tflops = flops / (ms * 1e-3) / 1e12;
      if (us_per_launch) *us_per_launch = ms * 1e3 / launches;
    }
  }
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return rc;
}

const char* ian_last_error(ian_handle* h) { return h ? h->err.c_str() : "null handle"; }

int ian_create(const ian_model_desc* desc, ian_handle** out) {
  if (!desc || !out) return -1;
  std::unique_ptr<ian_handle> h(new ian_handle());
  apply_env_options(h->opt);
  h->desc = *desc;
  h->strings.reserve((size_t)desc->n_ops * 2 + 4);
  h->ops.resize(desc->n_ops);
  for (int i = 0; i < desc->n_ops; ++i) {
    OpPlan& op = h->ops[i];
    op.d = desc->ops[i];
    op.name = op.d.name ? op.d.name : "";
    op.bn_name = op.d.bn_name ? op.d.bn_name : "";
    op.d.name = nullptr;
    op.d.bn_name = nullptr;
    if (op.d.n_scales < 0 || op.d.n_scales > IAN_MAX_SCALES) return -1;
    auto bad = [&](int s) { return s < -1 || s >= desc->n_slots; };
    if (bad(op.d.src) || bad(op.d.src2) || bad(op.d.src3) || bad(op.d.dst) || op.d.src < 0 || op.d.dst < 0) return -1;
  }
  h->slots.resize(desc->n_slots);
  for (int i = 0; i < desc->n_slots; ++i) {
    Slot& s = h->slots[i];
    s.h = desc->slots[i].h; s.w = desc->slots[i].w; s.c = desc->slots[i].c;
    s.cs = round_up(s.c, 32);
    s.nchw = (i == desc->x_slot || i == desc->out_slot);
  }
  h->desc.ops = nullptr;
  h->desc.slots = nullptr;
  *out = h.release();
  return 0;
}

int ian_load_param(ian_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
  if (!h || !name || !data || ndim < 0 || ndim > 8) return fail(h, -1, "bad argument to ian_load_param");
  if (h->finalized) return fail(h, -6, "model already finalized");
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  const int64_t n = t.numel();
  t.data.assign(data, data + n);
  h->params[name] = std::move(t);
  return 0;
}

int ian_set_made_masks(ian_handle* h, const float* m0, const float* m1, const float* md, int32_t n) {
  if (!h || !m0 || !m1 || !md || n <= 0) return fail(h, -1, "bad argument to ian_set_made_masks");
  const float* src[3] = {m0, m1, md};
  for (int k = 0; k < 3; ++k) {
    h->made_masks[k].assign(src[k], src[k] + (size_t)n * n);
    for (float v : h->made_masks[k])
      if (v != 0.f && v != 1.f) return fail(h, -3, "MADE mask %d is not 0/1 valued", k);
  }
  h->made_n = n;
  return 0;
}

int ian_finalize(ian_handle* h) {
  if (!h) return -1;
  if (h->finalized) return fail(h, -6, "model already finalized");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(h, -10, "no HIP device available: libian has no CPU fallback");
  }
  for (auto& op : h->ops) {
    int rc = 0;
    std::vector<int> out_perm;
    bool has_out_perm = false;
    switch (op.d.kind) {
      case IAN_OP_CONV5S2:
        if ((rc = pack_conv_fwd(h, op))) return rc;
        if ((rc = build_affine(h, op, op.d.cout, nullptr))) return rc;
        break;
      case IAN_OP_DECONV5S2:
        if ((rc = pack_deconv(h, op))) return rc;
        if ((rc = build_affine(h, op, op.d.cout, nullptr))) return rc;
        break;
      case IAN_OP_MDC3:
        if ((rc = pack_mdc(h, op))) return rc;
        if ((rc = build_affine(h, op, op.d.cout, nullptr))) return rc;
        break;
      case IAN_OP_DENSE:
        if ((rc = pack_dense(h, op, out_perm, has_out_perm))) return rc;
        if ((rc = build_affine(h, op, op.d.cout, has_out_perm ? &out_perm : nullptr))) return rc;
        break;
      case IAN_OP_AFFINE:
        if ((rc = build_affine(h, op, op.d.cout, nullptr))) return rc;
        break;
      case IAN_OP_MADE_IAF:
        if ((rc = pack_made(h, op))) return rc;
        break;
      case IAN_OP_BETA:
      case IAN_OP_CONCAT:
        break;
      default:
        return fail(h, -5, "unknown op kind %d", op.d.kind);
    }
    if ((rc = upload_layer(h, op.fwd))) return rc;
    if ((rc = upload_layer(h, op.bwd))) return rc;
    if ((rc = upload(h, op.h_edge_w, &op.d_edge_w))) return rc;
    if ((rc = upload(h, op.h_b1_fwd, &op.d_b1_fwd))) return rc;
    if ((rc = upload(h, op.h_b1_bwd, &op.d_b1_bwd))) return rc;
    std::vector<float>().swap(op.h_b1_fwd);
    std::vector<float>().swap(op.h_b1_bwd);
    if ((rc = upload(h, op.h_scale, &op.d_scale))) return rc;
    if ((rc = upload(h, op.h_shift, &op.d_shift))) return rc;
    std::vector<float>().swap(op.h_edge_w);
  }
  h->params.clear();
  h->finalized = true;
  return find_head_plan(h);
}

int ian_encode_pre_iaf(ian_handle* h, const float* x, int32_t n, float* z, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  TotalTimer tt(h, st);
  if ((rc = set_image_input(h, x, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_ENC, n, st))) return rc;
  return get_latent_output(h, h->desc.zpre_slot, z, n, st);
}

int ian_encode(ian_handle* h, const float* x, int32_t n, float* z, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  TotalTimer tt(h, st);
  h->dec_cache_valid = false;
  if ((rc = set_image_input(h, x, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_ENC, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_IAF, n, st))) return rc;
  return get_latent_output(h, h->desc.z_slot, z, n, st);
}

int ian_iaf(ian_handle* h, const float* zpre, int32_t n, float* z, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  h->dec_cache_valid = false;
  if ((rc = set_latent_input(h, h->desc.zpre_slot, zpre, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_IAF, n, st))) return rc;
  return get_latent_output(h, h->desc.z_slot, z, n, st);
}

int ian_decode(ian_handle* h, const float* z, int32_t n, float* x, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  if (!z || !x) return fail(h, -1, "null pointer passed to ian_decode");
  if (n == 1 && edit_graph_eligible(h, stream, {z, x})) {   // NPE.py:110,218,261: one latent, host buffers
    if ((rc = edit_ctx(h))) return rc;
    hipStream_t st = h->edit_stream;
    enter_stream(h, st);
    if ((rc = decode_one_graph(h, z))) return rc;
    Slot& os = h->slots[h->desc.out_slot];
    if (!h->pin_img_valid) {   // the image kernel did not write the pinned image itself (no zero-copy / another kernel path)
      HIPCHK(h, hipMemcpyAsync(h->pin + PIN_IMG, os.d, os.per_image() * sizeof(float), hipMemcpyDeviceToHost, st));
      h->pin_img_valid = true;
    }
    HIPCHK(h, wait_edit_stream(h, st));
    h->last_pending = false;
    memcpy(x, h->pin + PIN_IMG, os.per_image() * sizeof(float));
    return 0;
  }
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  TotalTimer tt(h, st);
  h->dec_cache_valid = false;
  if ((rc = set_latent_input(h, h->desc.z_slot, z, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;
  if ((rc = get_image_output(h, x, n, st))) return rc;
  if (n == 1 && !is_device_ptr(z)) {  // remember which latent the resident batch-1 activations belong to
    h->dec_cache_z.assign(z, z + h->desc.num_latents);
    h->dec_cache_valid = true;
  }
  return 0;
}

int ian_reconstruct(ian_handle* h, const float* x, int32_t n, float* xhat, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  TotalTimer tt(h, st);
  h->dec_cache_valid = false;
  if (!x || !xhat) return fail(h, -1, "null pointer passed to ian_reconstruct");
  SlotAlias in_alias, out_alias;
  if (h->opt.alias_io && is_device_ptr(x) && h->slots[h->desc.x_slot].nchw) in_alias.bind(h, h->desc.x_slot, x, n);
  else if ((rc = set_image_input(h, x, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_ENC, n, st))) return rc;
  if ((rc = run_segment(h, IAN_SEG_IAF, n, st))) return rc;
  if (h->opt.alias_io && is_device_ptr(xhat) && h->slots[h->desc.out_slot].nchw && xhat != x) {
    out_alias.bind(h, h->desc.out_slot, xhat, n);
    return run_segment(h, IAN_SEG_DEC, n, st);
  }
  if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;
  return get_image_output(h, xhat, n, st);
}

int ian_decode_u8(ian_handle* h, const float* z, int32_t n, uint8_t* out, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  if (!z || !out) return fail(h, -1, "null pointer passed to ian_decode_u8");
  hipStream_t st = (hipStream_t)stream;
  const bool graph = n == 1 && edit_graph_eligible(h, stream, {z, out});
  if (graph) {
    if ((rc = edit_ctx(h))) return rc;
    st = h->edit_stream;
  }
  enter_stream(h, st);
  TotalTimer tt(h, st);
  if (graph) {
    if ((rc = decode_one_graph(h, z))) return rc;
  } else if (n == 1) {
    if ((rc = decode_one_cached(h, z, st))) return rc;
  } else {
    h->dec_cache_valid = false;
    if ((rc = set_latent_input(h, h->desc.z_slot, z, n, st))) return rc;
    if ((rc = run_segment(h, IAN_SEG_DEC, n, st))) return rc;
  }
  Slot& os = h->slots[h->desc.out_slot];
  const size_t count = os.per_image() * (size_t)n;
  if (is_device_ptr(out)) {
    HIPCHK(h, launch_to_uint8(os.d, out, (long long)count, st));
    return 0;
  }
  if (count > h->u8_cap) {
    if (h->d_u8) HIPCHK(h, hipFree(h->d_u8));
    HIPCHK(h, hipMalloc((void**)&h->d_u8, count));
    h->u8_cap = count;
  }
  HIPCHK(h, launch_to_uint8(os.d, h->d_u8, (long long)count, st));
  HIPCHK(h, hipMemcpyAsync(out, h->d_u8, count, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->last_pending = false;
  return 0;
}

int ian_photo_blend(ian_handle* h, const float* z, const uint8_t* recon, const float* error, const double* gauss_half,
                    int32_t radius, uint8_t* im, double* mask, void* stream) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if (!z || !recon || !error || !gauss_half || !im) return fail(h, -1, "null pointer passed to ian_photo_blend");
  if (radius < 0 || radius > 7) return fail(h, -7, "ian_photo_blend: radius %d outside 0..7", radius);
  Slot& os = h->slots[h->desc.out_slot];
  if (os.h != 64 || os.w != 64 || os.c != 3) return fail(h, -7, "ian_photo_blend needs a 3x64x64 image");
  hipStream_t st = (hipStream_t)stream;
  const bool graph = edit_graph_eligible(h, stream, {z, recon, error, im, mask});
  if (graph) {
    if ((rc = edit_ctx(h))) return rc;
    st = h->edit_stream;
  }
  enter_stream(h, st);
  TotalTimer tt(h, st);
  if (graph) {
    if ((rc = decode_one_graph(h, z))) return rc;
  } else if ((rc = decode_one_cached(h, z, st))) return rc;
  bool pending = false;
  if ((rc = enqueue_photo_blend(h, recon, error, gauss_half, radius, im, mask, st, &pending))) return rc;
  if (pending) {
    HIPCHK(h, hipStreamSynchronize(st));
    h->last_pending = false;
  }
  return 0;
}

int ian_brush_step(ian_handle* h, int32_t c1, int32_t r1, int32_t c2, int32_t r2, const float* rgb, const float* z, float coef,
                   float gscale, float* z_new, float* dz, float* x, const ian_photo_args* photo, void* stream) {
  int rc = check_ready(h, 1);
  if (rc) return rc;
  if (!z || !z_new) return fail(h, -1, "null pointer passed to ian_brush_step");
  for (const void* p : {(const void*)z, (const void*)z_new, (const void*)dz, (const void*)x})
    if (p && is_device_ptr(p)) return fail(h, -7, "ian_brush_step takes host buffers for z, z_new, dz, x (the Tk callback's arrays)");
  const int mode = rgb ? 1 : 0;
  const int zl = h->desc.num_latents;
  Slot& zs = h->slots[h->desc.z_slot];
  Slot& out = h->slots[h->desc.out_slot];
  if ((rc = check_rect(h, nullptr, 0, c1, r1, c2, r2, "patch"))) return rc;
  const bool photo_host = photo && !is_device_ptr(photo->recon) && !is_device_ptr(photo->error) && !is_device_ptr(photo->im) &&
                          !(photo->mask && is_device_ptr(photo->mask));
  if (!edit_graph_eligible(h, stream, {rgb}) || (photo && !photo_host)) {
    // the same step composed from the public calls (profiling on, a caller stream, graphs switched off, ...)
    std::vector<float> g((size_t)std::max(zs.c, zl)), zn((size_t)zl);
    if ((rc = grad_common(h, mode, c1, r1, c2, r2, rgb, z, g.data(), stream))) return rc;
    for (int i = 0; i < zl; ++i) {
      volatile float t = g[i] * gscale;   // volatile: one rounding per operation, as numpy does it
      volatile float u = coef * t;
      zn[i] = z[i] + u;
    }
    if (dz) memcpy(dz, g.data(), zl * sizeof(float));
    if (x) {
      if ((rc = ian_decode(h, zn.data(), 1, x, stream))) return rc;
    } else if (!photo) {
      hipStream_t st = (hipStream_t)stream;
      enter_stream(h, st);
      if ((rc = decode_one_cached(h, zn.data(), st))) return rc;
    }
    if (photo && (rc = ian_photo_blend(h, zn.data(), photo->recon, photo->error, photo->gauss_half, photo->radius, photo->im, photo->mask, stream)))
      return rc;
    memcpy(z_new, zn.data(), zl * sizeof(float));
    return 0;
  }
  if ((rc = edit_ctx(h))) return rc;
  hipStream_t st = h->edit_stream;
  enter_stream(h, st);
  if ((rc = decode_one_graph(h, z))) return rc;   // no-op when the resident activations already belong to z
  const float* d_rgb = nullptr;
  if (mode == 1 && (rc = upload_rgb_if_changed(h, rgb, st, &d_rgb))) return rc;
  if ((rc = ensure_slot(h, h->desc.z_slot, 1, true))) return rc;
  ian_brush_item* item = pin_brush_item(h);
  item->c1 = c1; item->r1 = r1; item->c2 = c2; item->r2 = r2; item->mode = mode;
  item->coef = coef; item->gscale = gscale;
  h->dec_cache_valid = false;
  const int wx = x ? 1 : 0;
  ian_handle::EditGraph& G = h->g_step[mode][wx];
  h->pin_img_valid = false;
  rc = run_or_replay(h, G, [&]() -> int {
    int r;
    BrushBackward rq;
    rq.seed.rgb = d_rgb;
    if (zero_copy(h)) {
      // zero-copy form (round 4): the kernels read the brush rectangle / (coef, gscale) from the pinned block and write the new
      // latent, the gradient and the image into it; the graph holds NO copy node (each was a 4.6 us copy kernel + a boundary)
      rq.seed.table = reinterpret_cast<const int*>(h->pin_dev + PIN_BRUSH);
      rq.update = BrushBackward::SINGLE;
      rq.cg = h->pin_dev + PIN_BRUSH + BRUSH_CG;
      rq.z_mirror = h->pin_dev + PIN_Z;
      rq.g_mirror = h->pin_dev + PIN_DZ;
      if ((r = run_decoder_backward(h, rq, st))) return r;
      if (!rq.updated)   // the latent's backward did not take the GEMV form: the update as its own launch
        HIPCHK(h, launch_latent_update(zs.d, zs.g, rq.cg, zl, rq.z_mirror, rq.g_mirror, st));
      h->out_mirror = wx ? h->pin_dev + PIN_IMG : nullptr;
      r = run_segment(h, IAN_SEG_DEC, 1, st);
      h->out_mirror = nullptr;
      if (r) return r;
      G.mirrors = h->pin_img_valid;
      if (wx && !G.mirrors) HIPCHK(h, hipMemcpyAsync(h->pin + PIN_IMG, out.d, out.per_image() * sizeof(float), hipMemcpyDeviceToHost, st));
      return 0;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_patch, item, sizeof(ian_brush_item), hipMemcpyHostToDevice, st));
    rq.seed.table = h->d_patch;
    if ((r = run_decoder_backward(h, rq, st))) return r;
    HIPCHK(h, hipMemcpyAsync(h->pin + PIN_DZ, zs.g, zs.c * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, launch_latent_update(zs.d, zs.g, reinterpret_cast<const float*>(h->d_patch + BRUSH_CG), zl, nullptr, nullptr, st));
    HIPCHK(h, hipMemcpyAsync(h->pin + PIN_Z, zs.d, zl * sizeof(float), hipMemcpyDeviceToHost, st));
    if ((r = run_segment(h, IAN_SEG_DEC, 1, st))) return r;
    if (wx) HIPCHK(h, hipMemcpyAsync(h->pin + PIN_IMG, out.d, out.per_image() * sizeof(float), hipMemcpyDeviceToHost, st));
    return 0;
  });
  if (rc) return rc;
  h->pin_img_valid = wx && (G.mirrors || !zero_copy(h));   // the pinned image is the resident one (also after a replay)
  bool pending = false;
  if (photo && (rc = enqueue_photo_blend(h, photo->recon, photo->error, photo->gauss_half, photo->radius, photo->im, photo->mask, st, &pending)))
    return rc;
  HIPCHK(h, wait_edit_stream(h, st));
  h->last_pending = false;
  memcpy(z_new, h->pin + PIN_Z, zl * sizeof(float));
  if (dz) memcpy(dz, h->pin + PIN_DZ, zl * sizeof(float));
  if (x) memcpy(x, h->pin + PIN_IMG, out.per_image() * sizeof(float));
  h->dec_cache_z.assign(z_new, z_new + zl);
  h->dec_cache_valid = true;
  if (h->opt.edit_keep_warm_us > 0 && zero_copy(h)) {   // experiment: keep the queue busy until the next call arrives (or the budget runs out)
    reinterpret_cast<volatile int*>(h->pin)[PIN_WARM_FLAG] = 0;
    HIPCHK(h, launch_keep_warm(reinterpret_cast<const int*>(h->pin_dev) + PIN_WARM_FLAG, (long long)h->opt.edit_keep_warm_us * 100, st));   // wall_clock64: 100 MHz
    h->warm_armed = true;
    h->last_pending = true;
  }
  return 0;
}

int ian_grad_batch(ian_handle* h, int32_t n, const ian_brush_item* items, const float* rgb, const float* z, float* dz, void* stream) {
  return batch_common(h, n, items, rgb, z, nullptr, dz, nullptr, nullptr, stream, false);
}

int ian_brush_step_batch(ian_handle* h, int32_t n, const ian_brush_item* items, const float* rgb, const float* z, float* z_new, float* dz,
                         float* x, const ian_photo_batch_args* photo, void* stream) {
  return batch_common(h, n, items, rgb, z, z_new, dz, x, photo, stream, true);
}

// the sessions' strokes (ian_rt_session.inc): every step of the batched brush above in one submission
int ian_session_stroke(ian_handle* h, int32_t n, const ian_session_stroke_item* strokes, int32_t nboxes, const ian_stroke_box* boxes,
                       int32_t flags, uint8_t* shown, void* stream) {
  return h ? session_stroke(h, n, strokes, nboxes, boxes, flags, shown, stream) : -1;
}
int ian_session_path_tip(ian_handle* h, int32_t n, const ian_session_stroke_item* strokes, const int32_t* tips, int32_t nboxes,
                         const ian_stroke_box* boxes, int32_t flags, uint8_t* shown, void* stream) {
  return h ? session_stroke(h, n, strokes, nboxes, boxes, flags, shown, stream, true, tips) : -1;
}

int ian_autotune(ian_handle* h, int32_t n, int32_t what, void* stream) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  h->dec_cache_valid = false;
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  ++h->alloc_epoch;   // schedules are rebuilt below
  const bool prof = h->prof;
  h->prof = false;
  const bool verbose = getenv("IAN_DEBUG") != nullptr;
  static const char* cfg_names[TG_NCONFIG] = {"128x128", "128x64", "64x64", "32x128", "256x128", "128x32", "128x128/8w", "128x64/8w"};
  TuneCache cache;
  tune_cache_load(cache);
  bool cache_dirty = false;
  // the opt-in split-bf16 mode tunes other kernels on other tiles: its choices live under their own keys (a handle with tg_bf16x3 on
  // that replayed the exact-fp32 choices of the same IAN_TUNE_CACHE ran fp32 kernels on every tile the split-bf16 kernel does not
  // exist for: 1.17 instead of 0.66 ms per batch-64 step in the bench line taken under scripts/profile_round.sh)
  const char* dir_fwd = h->opt.tg_bf16x3 ? "fwd+bf16x3" : "fwd";
  const char* dir_bwd = h->opt.tg_bf16x3 ? "bwd+bf16x3" : "bwd";
  auto have = [&](int slot, bool grad) {
    if (slot < 0) return true;
    const Slot& s = h->slots[slot];
    return (grad ? s.gcap : s.cap) >= s.per_image() * (size_t)n && (grad ? s.g : s.d) != nullptr;
  };
  if (what & 1) {
    for (auto& op : h->ops) {
      if (!op.fwd.valid) continue;
      if (op.d.kind == IAN_OP_MDC3 && (mdc_head_eligible(h, op) || mdc_thin_eligible(h, op.fwd))) continue;  // VALU kernels: nothing to tune
      if (!have(op.d.src, false) || !have(op.d.src2, false) || !have(op.d.dst, false)) {
        h->prof = prof;
        return fail(h, -6, "ian_autotune: run a forward call with batch >= %d first (op '%s' has no activations)", n, op.name.c_str());
      }
      TgChoice best;
      float ms = 0;
      OpPlan* opp = &op;
      auto hit = cache.find(tune_key(n, dir_fwd, op.name));
      if (hit != cache.end()) {
        op.fwd.choice[n] = hit->second;
        free_schedule_for(op.fwd, n);
        continue;
      }
      cache_dirty = true;
      if ((rc = tune_layer(h, op.fwd, n, st, [&]() { return run_op_fwd(h, *opp, n, st); }, &best, &ms))) break;
      cache[tune_key(n, dir_fwd, op.name)] = best;
      if (verbose)
        fprintf(stderr, "[ian_autotune] n=%d fwd %-14s -> tile %s, max K-steps/item %d, schedule %d, combine %d, position-major %d : %.1f us (%.1f TF/s)\n", n,
                op.name.c_str(), cfg_names[best.cfg], best.max_steps, best.variant, best.fused, best.pos_major, ms * 1e3,
                2.0 * op.fwd.macs_per_image() * n / (ms * 1e-3) / 1e12);
    }
  }
  if (!rc && (what & 2)) {
    if (n != 1) {
      h->prof = prof;
      return fail(h, -7, "ian_autotune: the latent-brush backward is a batch-1 path");
    }
    Slot& out = h->slots[h->desc.out_slot];
    if (!have(h->desc.out_slot, false)) rc = fail(h, -6, "ian_autotune: run ian_grad_* once first");
    for (auto& op : h->ops) {
      if (rc) break;
      if (op.d.segment != IAN_SEG_DEC || !op.bwd.valid || op.edge) continue;
      if (!have(op.d.dst, true)) {
        rc = fail(h, -6, "ian_autotune: run ian_grad_* once first");
        break;
      }
      TgChoice best;
      float ms = 0;
      auto hit = cache.find(tune_key(1, dir_bwd, op.name));
      if (hit != cache.end()) {
        op.bwd.choice[1] = hit->second;
        free_schedule_for(op.bwd, 1);
        continue;
      }
      cache_dirty = true;
      BrushBackward rq;   // a 4x4 lighten brush in the middle of the image, as the eager ian_grad sends it
      rq.seed.c1 = out.w / 2 - 2; rq.seed.r1 = out.h / 2 - 2; rq.seed.c2 = out.w / 2 + 2; rq.seed.r2 = out.h / 2 + 2;
      rc = tune_layer(h, op.bwd, 1, st, [&]() { return run_decoder_backward(h, rq, st); }, &best, &ms);
      if (!rc) cache[tune_key(1, dir_bwd, op.name)] = best;
      if (!rc && verbose)
        fprintf(stderr, "[ian_autotune] n=1 bwd %-14s -> tile %s, max K-steps/item %d, schedule %d, combine %d : chain %.1f us\n", op.name.c_str(),
                cfg_names[best.cfg], best.max_steps, best.variant, best.fused, ms * 1e3);
    }
  }
  h->prof = prof;
  if (!rc && cache_dirty) tune_cache_store(cache);
  return rc;
}

int ian_grad_rgb(ian_handle* h, int32_t c1, int32_t r1, int32_t c2, int32_t r2, const float* rgb, const float* z,
                 float* dz, void* stream) {
  if (!rgb) return fail(h, -1, "rgb is null");
  return grad_common(h, 1, c1, r1, c2, r2, rgb, z, dz, stream);
}

int ian_grad_light(ian_handle* h, int32_t c1, int32_t r1, int32_t c2, int32_t r2, const float* z, float* dz,
                   void* stream) {
  return grad_common(h, 0, c1, r1, c2, r2, nullptr, z, dz, stream);
}

static int read_slot_impl(ian_handle* h, int32_t slot, int32_t n, float* out, void* stream, bool grad) {
  int rc = check_ready(h, n);
  if (rc) return rc;
  if (slot < 0 || slot >= (int)h->slots.size()) return fail(h, -1, "bad slot %d", slot);
  hipStream_t st = (hipStream_t)stream;
  enter_stream(h, st);
  Slot s = h->slots[slot];
  if (grad) {
    s.d = s.g;
    s.cap = s.gcap;
    s.nchw = false;
  }
  if (!s.d || s.cap < s.per_image() * (size_t)n) return fail(h, -1, "slot %d holds no %s for batch %d", slot, grad ? "gradient" : "activation", n);
  if (!grad && h->slot_stale.count(slot) && h->slot_stale[slot])
    return fail(h, -1, "slot %d was bound to the caller's device buffer in the last call: the library holds no copy of it", slot);
  const size_t count = (size_t)n * s.c * s.h * s.w;
  const bool dev = is_device_ptr(out);
  float* tmp = nullptr;
  float* target = out;
  if (!dev) {
    HIPCHK(h, hipMalloc((void**)&tmp, count * sizeof(float)));
    target = tmp;
  }
  if (s.nchw) HIPCHK(h, hipMemcpyAsync(target, s.d, count * sizeof(float), hipMemcpyDeviceToDevice, st));
  else HIPCHK(h, launch_nhwc_to_nchw(s.d, s.cs, target, n, s.h * s.w, s.c, st));
  if (!dev) {
    HIPCHK(h, hipMemcpyAsync(out, tmp, count * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipFree(tmp));
  }
  return 0;
}

int ian_read_slot(ian_handle* h, int32_t slot, int32_t n, float* out, void* stream) {
  return read_slot_impl(h, slot, n, out, stream, false);
}

int ian_read_slot_grad(ian_handle* h, int32_t slot, int32_t n, float* out, void* stream) {
  return read_slot_impl(h, slot, n, out, stream, true);
}

int ian_profile_enable(ian_handle* h, int32_t on) {
  if (!h) return -1;
  h->prof = on != 0;
  h->ev_used = 0;
  h->ev_total_used = 0;
  h->prof_flops = 0;
  h->prof_launches = 0;
  return 0;
}

int ian_profile_read(ian_handle* h, double* tapgemm_ms, int64_t* tapgemm_launches, double* tapgemm_flops,
                     double* total_ms) {
  if (!h) return -1;
  HIPCHK(h, hipDeviceSynchronize());
  double ms = 0;
  for (size_t i = 0; i < h->ev_used; ++i) {
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, h->ev_pool[i].first, h->ev_pool[i].second));
    ms += t;
  }
  double tot = 0;
  for (size_t i = 0; i < h->ev_total_used; ++i) {
    float t = 0;
    HIPCHK(h, hipEventElapsedTime(&t, h->ev_total[i].first, h->ev_total[i].second));
    tot += t;
  }
  if (tapgemm_ms) *tapgemm_ms = ms;
  if (tapgemm_launches) *tapgemm_launches = h->prof_launches;
  if (tapgemm_flops) *tapgemm_flops = h->prof_flops;
  if (total_ms) *total_ms = tot;
  return 0;
}

int ian_set_option(ian_handle* h, const char* key, int32_t value) {
  if (!h || !key) return -1;
  if (!apply_option(h->opt, key, value)) return fail(h, -1, "unknown option '%s'", key);
  for (auto& op : h->ops) {  // schedules depend on the options
    free_schedules(op.fwd);
    free_schedules(op.bwd);
  }
  ++h->alloc_epoch;
  h->dec_cache_valid = false;   // the resident activations were produced under the previous options
  h->batch.cache_valid = false;
  h->sess.res_valid = false;
  return 0;
}

void ian_destroy(ian_handle* h) {
  if (!h) return;
  warm_release(h);
  if (h->edit_stream) (void)hipStreamSynchronize(h->edit_stream);
  IAN_GUARD_CHECK("ian_destroy");
  for (auto& op : h->ops) {
    free_schedules(op.fwd);
    free_schedules(op.bwd);
    for (TgLayer* L : {&op.fwd, &op.bwd}) {
      if (L->d_w) (void)hipFree(L->d_w);
      if (L->d_wsplit) (void)hipFree(L->d_wsplit);
      if (L->d_classes) (void)hipFree(L->d_classes);
      if (L->d_taps) (void)hipFree(L->d_taps);
    }
    for (float* p : {op.d_edge_w, op.d_scale, op.d_shift, op.d_made_w, op.d_made_b, op.d_b1_fwd, op.d_b1_bwd})
      if (p) (void)hipFree(p);
  }
  for (auto& s : h->slots) {
    if (s.d) (void)hipFree(s.d);
    if (s.g) (void)hipFree(s.g);
  }
  for (float* p : {h->d_slab, h->d_stage_in, h->d_stage_out, h->d_gseed, h->d_rgb, h->head.d_ftab, h->head.d_comp})
    if (p) (void)hipFree(p);
  if (h->head.d_itab) (void)hipFree(h->head.d_itab);
  for (ian_handle::EditGraph* g : {&h->g_fwd, &h->g_bwd[0], &h->g_bwd[1], &h->g_step[0][0], &h->g_step[0][1], &h->g_step[1][0], &h->g_step[1][1]})
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (h->edit_stream) (void)hipStreamDestroy(h->edit_stream);
  if (h->pin) (void)hipHostFree(h->pin);
  if (h->d_patch) (void)hipFree(h->d_patch);
  for (void* p : {(void*)h->d_recon, (void*)h->d_error, (void*)h->d_im, (void*)h->d_mask, (void*)h->d_u8})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)h->batch.d_items, (void*)h->batch.d_rgb, (void*)h->batch.d_recon, (void*)h->batch.d_error, (void*)h->batch.d_out,
                  (void*)h->batch.d_im, (void*)h->batch.d_mask})
    if (p) (void)hipFree(p);
  sessions_free(h);
  for (auto& e : h->ev_pool) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  for (auto& e : h->ev_total) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  delete h;
}

}  // extern "C"

