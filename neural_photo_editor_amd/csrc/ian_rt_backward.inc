// ian_rt_backward.inc -- latent-brush backward (API.py:59,64): reverse sweep over the decoder ops.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
namespace {

// ----- latent-brush backward (API.py:59,64): reverse sweep over the decoder ops --------------------------
// Gradient buffers (Slot::g) hold dL/d(pre-epilogue value) of the slot's producer, so each backward tapgemm's
// epilogue (TG_EPI_BWD) multiplies by act'(y)*scale of the producer of ITS output slot and no separate
// elementwise pass runs on the GEMM edges.  The decoder graph of the full IAN is a DAG (residual adds, the
// shared feature map of the RGB-Beta head, concat): the ops are visited in reverse topological order and a slot
// that has more than one consumer accumulates (the epilogue's `res` input / the accumulate flag of the
// identity-edge kernels), "touched" recording whether a contribution already arrived in this sweep.
struct ProducerEpi {
  const float* scale = nullptr;
  const float* yfwd = nullptr;
  int act = IAN_ACT_NONE;
  int scale_period = 0;
};

// One backward sweep, as its caller asks for it: fill the members by name.
struct BrushBackward {
  BrushSeedSrc seed;       // the items' rectangles, loss kinds and target colours
  int n = 1;               // items = images resident in the decoder's slots
  bool batch = false;      // the several-editors calls (ian_grad_batch / ian_brush_step_batch / ian_session_brush; n = 1 included): the
                           // latent's backward is the batched GEMV, no batch-1 kernel runs
  // the brush update Z += coef * (dZ * gscale) wanted from the latent's backward GEMV (one launch less per event):
  enum Update { NONE, SINGLE, PER_ITEM } update = NONE;   // PER_ITEM: (coef, gscale) of every row of seed.table
  const float* cg = nullptr;   // SINGLE: (coef, gscale), device-readable
  float* z_mirror = nullptr;   // SINGLE: the new latent and the gradient also go there (the pinned host block), or nullptr
  float* g_mirror = nullptr;
  bool updated = false;    // out: the GEMV applied the update; otherwise the caller launches it on its own
};

int run_decoder_backward(ian_handle* h, BrushBackward& rq, hipStream_t st) {
  const BrushSeedSrc& seed = rq.seed;
  const int n = rq.n;
  rq.updated = false;
  if (n < 1 || (!rq.batch && n != 1)) return fail(h, -7, "imgrad: %d items outside the batched calls", n);
  std::vector<OpPlan*> dec;
  for (auto& op : h->ops)
    if (op.d.segment == IAN_SEG_DEC) dec.push_back(&op);
  if (dec.empty()) return fail(h, -8, "no decoder ops");
  const int nslots = (int)h->slots.size();
  std::vector<OpPlan*> prod(nslots, nullptr);
  for (OpPlan* op : dec) prod[op->d.dst] = op;
  OpPlan& last = *dec.back();
  if (last.d.dst != h->desc.out_slot) return fail(h, -9, "imgrad: the last decoder op does not produce l_out");
  Slot& out = h->slots[last.d.dst];
  const int H = out.h, W = out.w;
  if (!seed.table)   // a table's rows were checked by the caller that filled it
    if (int rc = check_rect(h, nullptr, 0, seed.c1, seed.r1, seed.c2, seed.r2, "patch")) return rc;
  if (!h->d_gseed) {
    HIPCHK(h, hipMalloc((void**)&h->d_gseed, (size_t)3 * H * W * sizeof(float)));
    h->gseed_cap = (size_t)3 * H * W;
    ++h->alloc_epoch;
  }
  // a table + an image-producing deconv (IAN_simple): seed, tanh' and the first backward-data in one launch, inside the sweep below
  const bool fused_seed = seed.table && last.d.kind == IAN_OP_DECONV5S2 && last.edge;
  if (!fused_seed && (size_t)n * 3 * H * W > h->gseed_cap) {   // the batch-1 graphs captured the old seed buffer: the epoch moves
    HIPCHK(h, hipFree(h->d_gseed));
    h->gseed_cap = (size_t)n * 3 * H * W;
    HIPCHK(h, hipMalloc((void**)&h->d_gseed, h->gseed_cap * sizeof(float)));
    ++h->alloc_epoch;
  }
  if (!fused_seed) HIPCHK(h, launch_brush_seed(seed, n, out.d, h->d_gseed, H, W, st));  // dL/dX_hat, NCHW

  std::vector<char> touched(nslots, 0);
  auto epi_of = [&](int slot) {  // what turns a value-gradient of `slot` into its producer's pre-epilogue gradient
    ProducerEpi e;
    OpPlan* p = prod[slot];
    if (!p) return e;
    Slot& s = h->slots[slot];
    e.scale = p->d_scale;
    e.act = p->d.act;
    e.yfwd = (e.act != IAN_ACT_NONE) ? s.d : nullptr;
    // a dense producer's batch-norm is per feature = per (pixel, channel) of the map it is reshaped to
    e.scale_period = (p->d.kind == IAN_OP_DENSE && s.h * s.w > 1) ? (int)s.per_image() : 0;
    return e;
  };
  auto pass_to = [&](const float* gs, int ss, int coff, int slot, int C) -> int {
    Slot& t = h->slots[slot];
    int rc = ensure_slot(h, slot, n, true);
    if (rc) return rc;
    ProducerEpi e = epi_of(slot);
    if (e.scale_period) return fail(h, -9, "imgrad: identity edge into a per-feature batch-norm is not supported");
    HIPCHK(h, launch_grad_pass(gs, ss, coff, t.g, e.yfwd, t.cs, e.scale, (long long)n * t.h * t.w, C, e.act, touched[slot], st));
    touched[slot] = 1;
    return 0;
  };

  for (int i = (int)dec.size() - 1; i >= 0; --i) {
    OpPlan& op = *dec[i];
    const int kind = op.d.kind;
    int rc;
    if (kind == IAN_OP_BETA) {  // IAN.py:207
      const int srcs[3] = {op.d.src, op.d.src2, op.d.src3};
      BetaBwdArgs a;
      for (int c = 0; c < 3; ++c) {
        Slot& m = h->slots[srcs[c]];
        if ((rc = ensure_slot(h, srcs[c], n, true))) return rc;
        ProducerEpi e = epi_of(srcs[c]);
        a.v[c] = m.d; a.g[c] = m.g; a.scale[c] = e.scale; a.act[c] = e.act; a.accumulate[c] = touched[srcs[c]];
        touched[srcs[c]] = 1;
      }
      Slot& m0 = h->slots[srcs[0]];
      HIPCHK(h, launch_beta_bwd(h->d_gseed, a, n, m0.h * m0.w, m0.cs, st));
      continue;
    }
    if (kind == IAN_OP_DECONV5S2 && op.edge) {  // image-producing deconv (IAN_simple dec_out)
      if (op.d.dst != h->desc.out_slot) return fail(h, -9, "imgrad: edge deconv '%s' must produce l_out", op.name.c_str());
      Slot& in = h->slots[op.d.src];
      if (touched[op.d.src]) return fail(h, -9, "imgrad: '%s' input has several consumers", op.name.c_str());
      if ((rc = ensure_slot(h, op.d.src, n, true))) return rc;
      ProducerEpi e = epi_of(op.d.src);
      if (e.scale_period) return fail(h, -9, "imgrad: per-feature batch-norm directly under the image deconv");
      if (fused_seed) {
        HIPCHK(h, launch_brush_seed_dec_out(seed, n, out.d, op.d.act, op.d_scale, op.d_edge_w, in.g, e.yfwd, e.scale, op.d.in_h, op.d.in_w,
                                            in.cs, op.d.cout, e.act, st));
      } else {
        HIPCHK(h, launch_dact_nchw(h->d_gseed, out.d, op.d_scale, n, out.c, H * W, op.d.act, st));
        HIPCHK(h, launch_deconv_out_bwd(h->d_gseed, op.d_edge_w, in.g, e.yfwd, e.scale, n, op.d.in_h, op.d.in_w, in.cs,
                                        op.d.cout, e.act, st));
      }
      touched[op.d.src] = 1;
      continue;
    }
    if (!touched[op.d.dst]) return fail(h, -9, "imgrad: no gradient reached the output of '%s'", op.name.c_str());
    Slot& o = h->slots[op.d.dst];
    switch (kind) {
      case IAN_OP_DENSE:
      case IAN_OP_DECONV5S2:
      case IAN_OP_MDC3: {
        if (!op.bwd.valid) return fail(h, -9, "imgrad: op '%s' has no backward-data form", op.name.c_str());
        Slot& in = h->slots[op.d.src];
        if ((rc = ensure_slot(h, op.d.src, n, true))) return rc;
        ProducerEpi pe = epi_of(op.d.src);
        TgEpilogue e;
        e.scale = pe.scale; e.shift = nullptr; e.yfwd = pe.yfwd; e.act = pe.act; e.scale_period = pe.scale_period;
        e.res = touched[op.d.src] ? in.g : nullptr;
        e.mode = TG_EPI_BWD;
        const int ystride = (kind == IAN_OP_DENSE) ? (int)in.per_image() : in.cs;
        const bool gemv = kind == IAN_OP_DENSE && h->opt.dense_gemv && !pe.scale && !pe.yfwd && pe.act == IAN_ACT_NONE && op.d.flat_c <= 0 &&
                          (op.bwd.Cin & 3) == 0 && op.bwd.Cout <= ystride;
        const bool to_latent = op.d.src == h->desc.z_slot && !e.res;   // this launch's output is the latent's whole gradient
        if (gemv && rq.batch && (size_t)op.bwd.Cin <= o.per_image() && (o.per_image() & 3) == 0) {
          // several editors: each weight row streamed once per block of items; the brush update rides along (ian_brush_step_batch)
          const bool upd = rq.update == BrushBackward::PER_ITEM && to_latent;
          HIPCHK(h, launch_dense_bwd_gemv_batch(o.g, (int)o.per_image(), op.bwd.d_w, op.bwd.Cout, op.bwd.Cin, n, e.res, in.g, ystride,
                                                upd ? in.d : nullptr, seed.table, st));
          if (upd) rq.updated = true;
        } else if (gemv && !rq.batch) {
          // the latent's own layer: slab [in][out], row j contiguous in the (permuted) output index = o.g's order
          // ian_brush_step: the same launch applies the latent update (the latent's row = this output)
          const bool upd = rq.update == BrushBackward::SINGLE && to_latent && h->opt.fuse_latent_update;
          HIPCHK(h, launch_dense_bwd_gemv(o.g, op.bwd.d_w, op.bwd.Cout, op.bwd.Cin, e.res, in.g, upd ? in.d : nullptr, rq.cg, rq.z_mirror,
                                          rq.g_mirror, st));
          if (upd) rq.updated = true;
        } else {
          B1Params bp;
          if (!rq.batch && kind == IAN_OP_DECONV5S2 && b1_fill(h, op, 1, o, in, bp)) {
            bp.x = o.g; bp.y = in.g; bp.scale = e.scale; bp.yfwd = e.yfwd; bp.res = e.res; bp.act = e.act; bp.bwd = 1;
            bp.scale_period = e.scale_period;
#ifdef IAN_ABLATION
            HIPCHK(h, launch_b1conv(bp, 1, st));
#endif
          } else if ((rc = run_tapgemm(h, op.bwd, n, o.g, in.g, ystride, e, st))) return rc;
        }
        touched[op.d.src] = 1;
        if (kind == IAN_OP_MDC3 && op.d.src2 >= 0)  // residual operand of the fused ElemwiseSum: identity edge
          if ((rc = pass_to(o.g, o.cs, 0, op.d.src2, o.c))) return rc;
        break;
      }
      case IAN_OP_AFFINE:  // stand-alone BatchNorm(+nonlinearity): its g already is dL/d(input value)
        if ((rc = pass_to(o.g, o.cs, 0, op.d.src, o.c))) return rc;
        break;
      case IAN_OP_CONCAT: {
        const int ca = h->slots[op.d.src].c, cb = h->slots[op.d.src2].c;
        if ((rc = pass_to(o.g, o.cs, 0, op.d.src, ca))) return rc;
        if ((rc = pass_to(o.g, o.cs, ca, op.d.src2, cb))) return rc;
        break;
      }
      default:
        return fail(h, -9, "imgrad: backward of op kind %d ('%s') is not implemented", kind, op.name.c_str());
    }
  }
  if (!touched[h->desc.z_slot]) return fail(h, -9, "imgrad: no gradient reached the latent");
  return 0;
}

}  // namespace
