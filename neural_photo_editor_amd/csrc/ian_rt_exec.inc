// ian_rt_exec.inc -- slots, tapgemm launches, fused head, forward executor.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
namespace {

int ensure_slot(ian_handle* h, int slot, int n, bool grad = false) {
  Slot& s = h->slots[slot];
  const size_t need = s.per_image() * (size_t)n;
  float*& ptr = grad ? s.g : s.d;
  size_t& cap = grad ? s.gcap : s.cap;
  if (need > cap) {
    if (ptr) HIPCHK(h, hipFree(ptr));
    HIPCHK(h, hipMalloc((void**)&ptr, need * sizeof(float)));
    HIPCHK(h, hipMemset(ptr, 0, need * sizeof(float)));  // channel padding must stay zero
    cap = need;
    ++h->alloc_epoch;
  }
  return 0;
}

bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

int run_tapgemm(ian_handle* h, TgLayer& L, int nimg, const float* x, float* y, int y_stride, const TgEpilogue& epi,
                hipStream_t st) {
  Schedule* S;
  int rc = get_schedule(h, L, nimg, &S);
  if (rc) return rc;
  TgParams p;
  p.x = x; p.w = L.d_w; p.y = y; p.slab = h->d_slab;
  p.items = S->d_items; p.classes = L.d_classes; p.taps = L.d_taps; p.ttaps = S->d_ttaps;
  p.epi = epi;
  p.M = S->M; p.b_shift = S->b_shift; p.nimg = nimg;
  p.variant = h->opt.tg_variant_force >= 0 ? h->opt.tg_variant_force : (S->variant >= 0 ? S->variant : h->opt.tg_variant);
  h->stats_chunks_last = 0;
  if (h->stats_next.mode) {   // one-shot request of the training step: statistics of the stored tensor in this launch's epilogue
    const TgShape sh = tg_shape(S->cfg);
    const long long chunks = (long long)((p.M + sh.bm - 1) / sh.bm) * (long long)L.classes.size();
    if (S->ntiles == 0 && !S->pos_major && chunks * 2 * L.Cout <= h->stats_cap && chunks < (1 << 16) && tg_stats_supported(S->cfg, p.variant)) {
      p.epi.st = h->stats_next;
      p.epi.st.C = L.Cout;
      p.epi.st.ncls = (int)L.classes.size();
      h->stats_chunks_last = (int)chunks;
    }
    h->stats_next.mode = 0;
  }
  p.IH = L.IH; p.IW = L.IW; p.Cin = L.Cin;
  p.qw_shift = ilog2_exact(L.QW); p.qhw_shift = ilog2_exact(L.QH * L.QW);
  p.si = L.si; p.by = L.by; p.bx = L.bx; p.so = L.so;
  p.OH = L.OH; p.OW = L.OW; p.Cout = L.Cout; p.y_stride = y_stride; p.CoutPad = L.CoutPad;
  const size_t xb = (size_t)nimg * L.IH * L.IW * L.Cin * sizeof(float);
  if (xb > 0xFFFF0000ull) return fail(h, -7, "batch %d makes a %zu-byte activation: above the 4 GiB buffer-descriptor range, split the batch", nimg, xb);   // <= TG_OOB_TAP (kernels_tapgemm.hip)
  p.x_bytes = (unsigned)xb;
  p.w_bytes = (unsigned)(L.w_floats * sizeof(float));
  const bool bf = S->bf16x3 && (epi.mode == TG_EPI_FWD ? h->opt.tg_bf16x3_fwd : h->opt.tg_bf16x3_bwd) != 0;
  p.variant = bf ? TG_VARIANT_BF16X3 : (h->opt.tg_variant_force >= 0 ? h->opt.tg_variant_force : (S->variant >= 0 ? S->variant : h->opt.tg_variant));
  if (p.variant == TG_SCHED_AHEAD2 && L.Cin > 16384) p.variant = TG_SCHED_ROTATED;   // schedule 7 keeps the channel chunk of a K-step in a scalar offset < 64 KB on top of TG_OOB_TAP
  p.wsplit = nullptr;
  p.bf_sched = h->opt.tg_bf16x3_sched;
  p.noepi = h->opt.tg_noepi;
  {
    const size_t yb = (size_t)nimg * L.OH * L.OW * (size_t)y_stride * sizeof(float);
    p.y_bytes = (h->opt.tg_fast_epilogue && yb <= 0xFFFF0000ull) ? (unsigned)yb : 0u;   // <= TG_OOB_Y (kernels_tapgemm.hip)
  }
  if (bf && h->opt.tg_bf16x3_wsplit) {
    if (!L.d_wsplit) {
      HIPCHK(h, hipMalloc((void**)&L.d_wsplit, L.w_floats * 2 * sizeof(unsigned short)));
      L.wsplit_valid = false;
    }
    if (!L.wsplit_valid) {       // stream-ordered in front of the launch that reads it
      HIPCHK(h, launch_wsplit(L.d_w, L.d_wsplit, (long long)L.w_floats, st));
      L.wsplit_valid = true;
    }
    p.wsplit = L.d_wsplit;
  }
  const bool fused = S->ntiles > 0 && S->fused != 0;
  p.tiles = S->d_tiles;
  p.counters = S->d_counters;
  p.raw = S->d_raw;
  p.fused = fused ? S->fused : 0;
  std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
  if (h->prof) {
    if (h->ev_used == h->ev_pool.size()) {
      hipEvent_t a, b;
      HIPCHK(h, hipEventCreate(&a));
      HIPCHK(h, hipEventCreate(&b));
      h->ev_pool.push_back({a, b});
    }
    ev = &h->ev_pool[h->ev_used++];
    HIPCHK(h, hipEventRecord(ev->first, st));
  }
  HIPCHK(h, launch_tapgemm(S->cfg, p, S->nitems, st));
  if (S->ntiles > 0 && !fused) {
    TgReduceParams r;
    r.slab = h->d_slab; r.y = y; r.tiles = S->d_tiles; r.classes = L.d_classes; r.epi = epi;
    r.M = p.M; r.qw_shift = p.qw_shift; r.qhw_shift = p.qhw_shift; r.so = L.so; r.OH = L.OH; r.OW = L.OW;
    r.Cout = L.Cout; r.y_stride = y_stride; r.b_shift = p.b_shift; r.nimg = nimg;
    HIPCHK(h, launch_tapgemm_reduce(S->cfg, r, S->ntiles, (S->max_nsplit >= 8 && h->opt.tg_reduce_kp > 1) ? 4 : 1, st));
  }
  if (ev) {
    HIPCHK(h, hipEventRecord(ev->second, st));
    h->prof_flops += 2.0 * L.macs_per_image() * nimg;
    h->prof_launches += 1;
  }
  return 0;
}

// thin MDCL: <= 4 real input channels (forward of G_b/B_b; backward-data form of every 2-filter head layer)
bool mdc_thin_eligible(const ian_handle* h, const TgLayer& L) {
  if (!h->opt.mdc_head || !L.valid || L.cin_real > 4 || L.classes.size() != 1 || L.taps.size() > 36) return false;
  if (L.si != 1 || L.so != 1 || L.by != 0 || L.bx != 0 || L.QH != L.IH || L.QW != L.IW) return false;
  if (L.Cout > 4) return false;  // wide outputs (backward-data of the 2-filter heads) measured 10x slower here than on tapgemm
  for (auto& t : L.taps)
    if (t.dy < -64 || t.dy > 64 || t.dx < -64 || t.dx > 64) return false;
  return true;
}

void mdc_thin_fill(MdcThinArgs& a, const TgLayer& L, const float* x, int xs, float* y, int ys, int n, const ian_handle* h) {
  memset(&a, 0, sizeof a);
  a.no_tile = h->opt.mdc_thin_tile ? 0 : 1;
  a.x = x; a.w = L.d_w; a.y = y; a.n = n; a.H = L.IH; a.W = L.IW; a.xs = xs; a.ys = ys; a.Cout = L.Cout;
  a.CoutPad = L.CoutPad; a.CinPad = L.Cin; a.ntaps = (int)L.taps.size();
  for (int t = 0; t < a.ntaps; ++t) { a.dy[t] = (signed char)L.taps[t].dy; a.dx[t] = (signed char)L.taps[t].dx; }
}

bool mdc_head_eligible(const ian_handle* h, const OpPlan& op) {
  const TgLayer& L = op.fwd;
  if (!h->opt.mdc_head || L.Cout > 4 || (L.Cin != 128 && L.Cin != 64) || L.cin_real != L.Cin) return false;
  if ((L.IH % 4) || (L.IW % 16) || L.taps.size() > 48 || L.classes.size() != 1) return false;
  for (auto& t : L.taps)
    if (t.dy < -4 || t.dy > 4 || t.dx < -4 || t.dx > 4) return false;
  return true;
}

// Fill the per-filter slots of MdcHeadArgs for one layer; weights/scale/shift are read back from the host copies.
int mdc_head_add(ian_handle* h, MdcHeadArgs& a, int& nco, const OpPlan& op, float* y, int ys, const float* res) {
  const TgLayer& L = op.fwd;
  for (int co = 0; co < L.Cout; ++co) {
    if (nco >= MH_MAXCO) return fail(h, -4, "mdc head: too many filters");
    a.w[nco] = L.d_w + (size_t)co * L.Cin;
    a.res[nco] = res;
    a.y[nco] = y;
    a.ys[nco] = ys;
    a.yc[nco] = co;
    a.act[nco] = op.d.act;
    a.scale[nco] = op.h_scale.empty() ? 1.f : op.h_scale[co];
    a.shift[nco] = op.h_shift.empty() ? 0.f : op.h_shift[co];
    ++nco;
  }
  return 0;
}

// Inference: few-filter MDCL layers on the VALU kernel.  Sibling layers that read the same map with the same taps and
// have no residual input are computed by ONE launch when the first of them is reached (their inputs are ready: same
// source); the others are skipped when their turn comes (OpPlan::head_done_for marks the batch they were computed for).
int run_mdc_head_group(ian_handle* h, OpPlan& op, int n, hipStream_t st) {
  if (op.head_done_serial == h->run_serial) return 0;  // already produced by its group leader in this call
  const TgLayer& L = op.fwd;
  MdcHeadArgs a;
  memset(&a, 0, sizeof a);
  Slot& src = h->slots[op.d.src];
  a.x = src.d; a.H = L.IH; a.W = L.IW; a.xs = src.cs; a.ntaps = (int)L.taps.size();
  a.w_tap_stride = (long long)L.CoutPad * L.Cin;
  for (int t = 0; t < a.ntaps; ++t) { a.dy[t] = (signed char)L.taps[t].dy; a.dx[t] = (signed char)L.taps[t].dx; }
  int nco = 0, rc;
  Slot& dst = h->slots[op.d.dst];
  const float* res = op.d.src2 >= 0 ? h->slots[op.d.src2].d : nullptr;
  if ((rc = mdc_head_add(h, a, nco, op, dst.d, dst.cs, res))) return rc;
  if (h->opt.mdc_head >= 2 && op.d.src2 < 0) {
    for (auto& o : h->ops) {
      if (&o == &op || o.d.kind != IAN_OP_MDC3 || o.d.segment != op.d.segment || o.d.src != op.d.src || o.d.src2 >= 0) continue;
      if (o.head_done_serial == h->run_serial || !mdc_head_eligible(h, o)) continue;
      const TgLayer& M = o.fwd;
      if (M.taps.size() != L.taps.size() || M.Cin != L.Cin || M.CoutPad != L.CoutPad || nco + M.Cout > MH_MAXCO) continue;
      bool same = true;
      for (size_t t = 0; t < L.taps.size(); ++t) same = same && M.taps[t].dy == L.taps[t].dy && M.taps[t].dx == L.taps[t].dx;
      if (!same) continue;
      if ((rc = ensure_slot(h, o.d.dst, n))) return rc;
      Slot& od = h->slots[o.d.dst];
      if ((rc = mdc_head_add(h, a, nco, o, od.d, od.cs, nullptr))) return rc;
      o.head_done_serial = h->run_serial;
    }
  }
  HIPCHK(h, launch_mdc_head(a, n, L.Cin, nco, st));
  return 0;
}

// ----- fused RGB-Beta head (kernels_head.hip) --------------------------------------------------------------------
bool same_taps(const TgLayer& A, const TgLayer& B) {
  if (A.taps.size() != B.taps.size() || A.classes.size() != 1 || B.classes.size() != 1) return false;
  for (size_t t = 0; t < A.taps.size(); ++t)
    if (A.taps[t].dy != B.taps[t].dy || A.taps[t].dx != B.taps[t].dx) return false;
  return true;
}

int find_head_plan(ian_handle* h) {
  HeadPlan& P = h->head;
  P.searched = true;
  const int nops = (int)h->ops.size();
  std::vector<int> prod(h->slots.size(), -1);
  for (int i = 0; i < nops; ++i) prod[h->ops[i].d.dst] = i;
  auto mdc2 = [&](int i) { return i >= 0 && h->ops[i].d.kind == IAN_OP_MDC3 && h->ops[i].d.cout == 2 && h->ops[i].d.segment == IAN_SEG_DEC; };
  for (int ib = 0; ib < nops; ++ib) {
    const ian_op_desc& b = h->ops[ib].d;
    if (b.kind != IAN_OP_BETA || b.dst != h->desc.out_slot || b.src < 0 || b.src2 < 0 || b.src3 < 0) continue;
    const int iR = prod[b.src], iGb = prod[b.src2], iBb = prod[b.src3];
    if (!mdc2(iR) || !mdc2(iGb) || !mdc2(iBb)) continue;
    const ian_op_desc &R = h->ops[iR].d, &Gb = h->ops[iGb].d, &Bb = h->ops[iBb].d;
    if (R.src2 >= 0 || Gb.src != R.dst || Gb.src2 < 0 || Bb.src2 < 0 || Gb.cin != 2 || Bb.cin != 4) continue;
    const int iGa = prod[Gb.src2], iBa = prod[Bb.src2], iCat = prod[Bb.src];
    if (!mdc2(iGa) || !mdc2(iBa) || iCat < 0) continue;
    const ian_op_desc &Ga = h->ops[iGa].d, &Ba = h->ops[iBa].d, &Cat = h->ops[iCat].d;
    if (Cat.kind != IAN_OP_CONCAT || Cat.src != R.dst || Cat.src2 != Gb.dst) continue;
    if (Ga.src != R.src || Ba.src != R.src || Ga.src2 >= 0 || Ba.src2 >= 0) continue;
    if (R.cin != 128 || R.in_w != 64 || h->slots[R.src].cs != 128) continue;
    const TgLayer& LR = h->ops[iR].fwd;
    bool ok = same_taps(LR, h->ops[iGa].fwd) && same_taps(LR, h->ops[iBa].fwd) && same_taps(LR, h->ops[iGb].fwd) &&
              same_taps(LR, h->ops[iBb].fwd) && LR.taps.size() <= 37;
    int halo = 0;
    std::vector<int> per_dy(9, 0);
    for (auto& t : LR.taps) {
      if (t.dy < -4 || t.dy > 4 || t.dx < -64 || t.dx > 64) ok = false;
      else if (++per_dy[t.dy + 4] > 12) ok = false;
      halo = std::max(halo, std::abs(t.dy));
    }
    // each of the three slots must feed nothing but the head (they are never materialised by the fused launch)
    for (int i = 0; i < nops && ok; ++i) {
      const ian_op_desc& d = h->ops[i].d;
      for (int sl : {Ga.dst, Ba.dst, Cat.dst})
        if ((d.src == sl || d.src2 == sl || d.src3 == sl) && i != iGb && i != iBb) ok = false;
    }
    if (!ok) continue;
    P.opR = iR; P.opGa = iGa; P.opGb = iGb; P.opBa = iBa; P.opBb = iBb; P.opCat = iCat; P.opBeta = ib; P.halo = halo;
    P.first = std::min({iR, iGa, iBa});
    // tables: taps grouped by dy (the shift-add of head6_kernel) and the six filters' epilogues
    std::vector<int> itab(44, -1);   // head6_kernel's static slot layout
    std::vector<int> used(9, 0);
    for (size_t t = 0; t < LR.taps.size() && ok; ++t) {
      const int dy = LR.taps[t].dy, g = dy == 0 ? 0 : (dy < 0 ? dy + 5 : dy + 4);
      const int cap = g == 0 ? 12 : 4, s0 = g == 0 ? 0 : 12 + (g - 1) * 4;
      if (used[g] >= cap || LR.taps[t].dx < -63 || LR.taps[t].dx > 63) { ok = false; break; }
      itab[s0 + used[g]++] = (int)t | ((LR.taps[t].dx + 64) << 8);
    }
    if (!ok) continue;
    std::vector<float> ftab(32, 0.f);
    const int six[3] = {iR, iGa, iBa};
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 2; ++c) {
        const OpPlan& o = h->ops[six[k]];
        ftab[2 * k + c] = o.h_scale.empty() ? 1.f : o.h_scale[c];
        ftab[8 + 2 * k + c] = o.h_shift.empty() ? 0.f : o.h_shift[c];
        ftab[16 + 2 * k + c] = (float)o.d.act;
      }
    int rc;
    if ((rc = upload(h, itab, &P.d_itab))) return rc;
    if ((rc = upload(h, ftab, &P.d_ftab))) return rc;
    P.valid = true;
    return 0;
  }
  return 0;
}

bool head_fused_active(const ian_handle* h, int n) {
  // keep_layer_acts: the batched latent brush runs a backward sweep after this forward and needs every layer's activation
  return h->head.valid && h->opt.head_fused && h->opt.mdc_head && n >= h->opt.head_fused_min_n && !h->keep_layer_acts;
}

int run_head_fused(ian_handle* h, int n, hipStream_t st) {
  HeadPlan& P = h->head;
  const OpPlan &R = h->ops[P.opR], &Ga = h->ops[P.opGa], &Gb = h->ops[P.opGb], &Ba = h->ops[P.opBa], &Bb = h->ops[P.opBb];
  const Slot& src = h->slots[R.d.src];
  const int H = R.d.in_h, W = R.d.in_w;
  const size_t need = (size_t)n * H * W * 8;
  if (need > P.comp_cap) {
    if (P.d_comp) HIPCHK(h, hipFree(P.d_comp));
    HIPCHK(h, hipMalloc((void**)&P.d_comp, need * sizeof(float)));
    P.comp_cap = need;
  }
  int rc;
  if ((rc = ensure_slot(h, h->desc.out_slot, n))) return rc;
  HeadFusedArgs a;
  memset(&a, 0, sizeof a);
  a.x = src.d; a.w0 = R.fwd.d_w; a.w1 = Ga.fwd.d_w; a.w2 = Ba.fwd.d_w; a.out = P.d_comp; a.itab = P.d_itab; a.ftab = P.d_ftab;
  a.H = H; a.W = W; a.xs = src.cs; a.ntaps = (int)R.fwd.taps.size(); a.halo = P.halo;
  a.w_tap_stride = (long long)R.fwd.CoutPad * R.fwd.Cin;
  // bands: whole images per workgroup when the batch alone fills the chip (no halo rows recomputed); smaller batches
  // are cut into row bands so that at least head_wgs (256) workgroups exist (each band re-reads 2*halo rows)
  a.bands = row_bands(n, h->opt.head_wgs, H, 1, 2 * P.halo);
  HIPCHK(h, launch_head6(a, n, st));
  HeadTailArgs t;
  memset(&t, 0, sizeof t);
  t.comp = P.d_comp; t.w_gb = Gb.fwd.d_w; t.w_bb = Bb.fwd.d_w; t.out = h->slots[h->desc.out_slot].d;
  t.gb_tap_stride = (long long)Gb.fwd.CoutPad * Gb.fwd.Cin; t.bb_tap_stride = (long long)Bb.fwd.CoutPad * Bb.fwd.Cin;
  t.gb_cin = Gb.fwd.Cin; t.bb_cin = Bb.fwd.Cin;
  for (int c = 0; c < 2; ++c) {
    t.scale_g[c] = Gb.h_scale.empty() ? 1.f : Gb.h_scale[c]; t.shift_g[c] = Gb.h_shift.empty() ? 0.f : Gb.h_shift[c];
    t.scale_b[c] = Bb.h_scale.empty() ? 1.f : Bb.h_scale[c]; t.shift_b[c] = Bb.h_shift.empty() ? 0.f : Bb.h_shift[c];
  }
  t.act_g = Gb.d.act; t.act_b = Bb.d.act; t.H = H; t.W = W; t.ntaps = a.ntaps;
  for (int k = 0; k < a.ntaps; ++k) { t.dy[k] = (signed char)R.fwd.taps[k].dy; t.dx[k] = (signed char)R.fwd.taps[k].dx; }
  HIPCHK(h, launch_head_tail(t, n, st));
  return 0;
}

TgEpilogue fwd_epi(const OpPlan& op, const float* res) {
  TgEpilogue e;
  e.scale = op.d_scale; e.shift = op.d_shift; e.res = res; e.yfwd = nullptr; e.act = op.d.act; e.mode = TG_EPI_FWD;
  e.scale_period = 0;
  return e;
}

// batch-1 transposed conv / its backward-data as one whole-contraction streaming launch (kernels_b1.hip).
// mode 0: x = the layer input (H x W x cin), y = its output;  mode 1: x = dL/d(pre-epilogue output) (2H x 2W x cout), y = dL/d(input)
bool b1_fill(const ian_handle* h, const OpPlan& op, int mode, const Slot& xin, const Slot& yout, B1Params& p) {
#ifndef IAN_ABLATION
  (void)h; (void)op; (void)mode; (void)xin; (void)yout; (void)p;
  return false;   // kernels_b1.hip (batch-1 streaming deconv, measured slower) is compiled into libian_ablation.so only
#else
  if (!h->opt.b1_conv || op.d.kind != IAN_OP_DECONV5S2 || op.edge) return false;
  const float* w = mode == 0 ? op.d_b1_fwd : op.d_b1_bwd;
  if (!w) return false;
  const int H = op.d.in_h, W = op.d.in_w, cin = op.d.cin, cout = op.d.cout;
  p = B1Params();
  p.w = w;
  if (mode == 0) {
    p.IH = H; p.IW = W; p.Cr = cin; p.OH = 2 * H; p.OW = 2 * W;
    p.nslices = cout / 16;
    for (int c = 0; c < 4; ++c) p.cls_off[c] = op.b1_cls_off[c];
  } else {
    p.IH = 2 * H; p.IW = 2 * W; p.Cr = cout; p.OH = H; p.OW = W;
    p.nslices = cin / 16;
  }
  p.xs = xin.cs; p.ys = yout.cs;
  if (p.xs < p.Cr || (p.xs & 3)) return false;
  p.tiles_x = W / 4;
  p.ntiles = (H / 4) * (W / 4);
  const size_t xb = (size_t)p.IH * p.IW * p.xs * sizeof(float);
  if (xb > 0xFFFFFFC0ull) return false;
  p.x_bytes = (unsigned)xb;
  p.kshift = ilog2_exact(p.Cr / 32);
  return p.kshift >= 0;
#endif
}

// ----- forward executor ---------------------------------------------------------------------------------
int run_op_fwd(ian_handle* h, OpPlan& op, int n, hipStream_t st) {
  Slot& src = h->slots[op.d.src];
  Slot& dst = h->slots[op.d.dst];
  int rc;
  if ((rc = ensure_slot(h, op.d.dst, n))) return rc;
  const float* res = nullptr;
  switch (op.d.kind) {
    case IAN_OP_CONV5S2:
      if (op.edge) {
        HIPCHK(h, launch_conv1_nchw(src.d, op.d_edge_w, op.d_scale, op.d_shift, dst.d, n, op.d.in_h, op.d.in_w,
                                    op.d.cout, op.d.act, st));
        return 0;
      }
      return run_tapgemm(h, op.fwd, n, src.d, dst.d, dst.cs, fwd_epi(op, nullptr), st);
    case IAN_OP_DECONV5S2:
      if (op.edge && h->opt.dec_out_mfma && n >= 4 && op.d.cin == 128 && src.cs == 128 && op.d.in_w == 32 && (op.d.in_h % 2) == 0 &&
          (op.d.cout == 3 || op.d.cout == 4)) {
        // image-producing deconv on the matrix cores (kernels_head.hip: contract first, scatter the 25 taps later)
        DeconvSmallArgs a;
        a.x = src.d; a.w = op.d_edge_w; a.scale = op.d_scale; a.shift = op.d_shift; a.y = dst.d;
        a.H = op.d.in_h; a.W = op.d.in_w; a.xs = src.cs; a.act = op.d.act;
        a.bands = row_bands(n, h->opt.dec_out_wgs, op.d.in_h, 2, 0);   // whole row pairs; one halo row per side of a band
        a.balanced = h->opt.dec_out_bal;
        HIPCHK(h, launch_deconv_small(a, n, op.d.cout, st));
        h->pin_img_valid = false;
        return 0;
      }
      if (op.edge && h->opt.dec_out_px && n < 4 && (src.cs == 64 || src.cs == 128 || src.cs == 256)) {
        float* mirror = (n == 1 && op.d.dst == h->desc.out_slot) ? h->out_mirror : nullptr;
        HIPCHK(h, launch_deconv_out_px(src.d, op.d_edge_w, op.d_scale, op.d_shift, dst.d, mirror, n, op.d.in_h, op.d.in_w, src.cs,
                                       op.d.cout, op.d.act, st));
        h->pin_img_valid = mirror != nullptr;
        return 0;
      }
      if (op.edge) {
        h->pin_img_valid = false;
        HIPCHK(h, launch_deconv_out_nchw(src.d, op.d_edge_w, op.d_scale, op.d_shift, dst.d, n, op.d.in_h, op.d.in_w,
                                         src.cs, op.d.cout, op.d.act, st));
        return 0;
      }
      if (n == 1) {
        B1Params bp;
        if (b1_fill(h, op, 0, src, dst, bp)) {
          bp.x = src.d; bp.y = dst.d; bp.scale = op.d_scale; bp.shift = op.d_shift; bp.act = op.d.act; bp.bwd = 0;
#ifdef IAN_ABLATION
          HIPCHK(h, launch_b1conv(bp, 0, st));
#endif
          return 0;
        }
      }
      return run_tapgemm(h, op.fwd, n, src.d, dst.d, dst.cs, fwd_epi(op, nullptr), st);
    case IAN_OP_MDC3:
      if (op.d.src2 >= 0) res = h->slots[op.d.src2].d;
      if (mdc_head_eligible(h, op)) return run_mdc_head_group(h, op, n, st);
      if (mdc_thin_eligible(h, op.fwd)) {
        MdcThinArgs a;
        mdc_thin_fill(a, op.fwd, src.d, src.cs, dst.d, dst.cs, n, h);
        a.res = res; a.scale = op.d_scale; a.shift = op.d_shift; a.act = op.d.act;
        HIPCHK(h, launch_mdc_thin(a, st));
        return 0;
      }
      return run_tapgemm(h, op.fwd, n, src.d, dst.d, dst.cs, fwd_epi(op, res), st);
    case IAN_OP_DENSE:
      if (n == 1 && h->opt.dense_gemv && op.d.flat_c <= 0 && op.fwd.Cin <= 256 && (op.fwd.Cin & 31) == 0 && op.fwd.Cout >= 1024) {
        // the latent's own layer at batch 1 (interactive decoder): one short-vector GEMV launch, no split-K pass
        HIPCHK(h, launch_dense_fwd_gemv(src.d, op.fwd.d_w, op.fwd.Cin, op.fwd.Cout, op.d_scale, op.d_shift, op.d.act, dst.d, st));
        return 0;
      }
      return run_tapgemm(h, op.fwd, n, src.d, dst.d, (int)dst.per_image(), fwd_epi(op, nullptr), st);
    case IAN_OP_AFFINE:
      HIPCHK(h, launch_affine(src.d, dst.d, op.d_scale, op.d_shift, (long long)n * src.h * src.w, src.c, src.cs,
                              op.d.act, st));
      return 0;
    case IAN_OP_MADE_IAF:
      HIPCHK(h, launch_made_iaf(src.d, dst.d, op.d_made_w, op.d_made_b, n, op.d.cin, src.cs, st));
      return 0;
    case IAN_OP_BETA:
      HIPCHK(h, launch_beta(src.d, h->slots[op.d.src2].d, h->slots[op.d.src3].d, dst.d, n, src.h * src.w, src.cs, st));
      return 0;
    case IAN_OP_CONCAT: {
      Slot& b = h->slots[op.d.src2];
      HIPCHK(h, launch_concat2(src.d, src.c, src.cs, b.d, b.c, b.cs, dst.d, dst.cs, (long long)n * src.h * src.w, st));
      return 0;
    }
  }
  return fail(h, -5, "unknown op kind %d", op.d.kind);
}

int run_segment(ian_handle* h, int seg, int n, hipStream_t st) {
  ++h->run_serial;
  if (seg == IAN_SEG_DEC) {
    h->pin_img_valid = false;   // the output slot is about to change; only the mirrored image kernel re-validates
    // the decoder refills the output slot: its OWN buffer is fresh again unless a caller's device buffer stands in for it
    // (ADVICE r3: ian_decode_u8, the decoder cache, the graph and brush paths used to leave it marked stale forever)
    if (!h->slot_aliased.count(h->desc.out_slot) || !h->slot_aliased[h->desc.out_slot]) h->slot_stale[h->desc.out_slot] = 0;
  }
  const bool fused = seg == IAN_SEG_DEC && head_fused_active(h, n);
  const HeadPlan& P = h->head;
  for (int i = 0; i < (int)h->ops.size(); ++i) {
    OpPlan& op = h->ops[i];
    if (op.d.segment != seg) continue;
    if (fused && (i == P.opR || i == P.opGa || i == P.opGb || i == P.opBa || i == P.opBb || i == P.opCat || i == P.opBeta)) {
      if (i == P.first) {   // the 128-channel map all of them hang off is ready: the whole head in two launches
        int rc = run_head_fused(h, n, st);
        if (rc) return rc;
      }
      continue;
    }
    int rc = run_op_fwd(h, op, n, st);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace
