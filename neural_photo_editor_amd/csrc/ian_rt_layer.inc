// ian_rt_layer.inc -- layer objects of include/ian_train.h (ian_layer_*).
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
// ====================================== layer objects (include/ian_train.h) ==============================
// One object per linear Lasagne layer of the training graph (train_IAN.py:116-149).  It reuses the inference
// packers to learn WHERE every reference-layout weight lands in the forward / backward slabs (the packers are run
// once on an index tensor), so that the per-step repacking after each optimiser update is a device-side gather.
struct WgSchedule {
  int cfg = 0, nitems = 0, nsplit = 1;
  WgItem* d_items = nullptr;
};

struct ian_layer {
  ian_handle ctx;  // options, split-K workspace, error text
  OpPlan op;
  bool is_mdc = false;
  std::vector<int64_t> pnumel;
  int* d_fwd_map = nullptr;
  int* d_bwd_map = nullptr;
  int* d_inv_map = nullptr;  // reference index -> forward slab index
  WgReduceTiledDesc rtd;     // ... and the same map in closed form, when it is affine (the tiled split reduce, the tiled repack)
  WgReduceTiledDesc rtd_b;   // the backward slab's map in closed form (rows = input channels, columns = filters)
  int* d_rt_tab[4] = {nullptr, nullptr, nullptr, nullptr};   // offset tables of the two maps (dense layers with a flatten / unflatten permutation)
  size_t fwd_count = 0, bwd_count = 0;
  MdcPackArgs mdc;
  int mdc_param_branch[1 + IAN_MAX_SCALES];  // parameter i (>=1) -> branch id, or -1 for the 1x1 coefficient
  float* d_partial = nullptr;
  size_t partial_cap = 0;
  float* d_dS = nullptr;  // MDC: reduced slab gradient
  // contract-first backward-weight of three sibling head layers (ian_layer_head6_backward_weight): owned by the first one
  ian_layer* h6_helper = nullptr;   // dense 128 -> 6*taps layer whose backward-weight is the one GEMM
  float* h6_Z = nullptr;
  size_t h6_Z_cap = 0;
  float* h6_dW = nullptr;
  int* h6_taps = nullptr;
  std::map<int, WgSchedule> wsched;
};

namespace {

int lfail(ian_layer* l, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (l) l->ctx.err = buf;
  return code;
}

#define LHIP(l, expr)                                                                                          \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess) return lfail(l, -2, "HIP error %s at %s:%d (%s)", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
  } while (0)

// index tensor: value = reference index + 1 (exact in float32 below 2^24), 0 marks padding
void add_index_param(ian_handle* h, const std::string& name, std::vector<int64_t> shape) {
  HostTensor t;
  t.shape = shape;
  const int64_t n = t.numel();
  t.data.resize(n);
  for (int64_t i = 0; i < n; ++i) t.data[i] = (float)(i + 1);
  h->params[name] = std::move(t);
}

std::vector<int> slab_to_map(const std::vector<float>& hw) {
  std::vector<int> m(hw.size());
  for (size_t i = 0; i < hw.size(); ++i) m[i] = (int)hw[i] - 1;
  return m;
}


// Is the forward slab -> reference map affine,  ref(t, co, ci) = co * s_co + ci * s_ci + tap_off[t]  with the taps of one (filter,
// channel) pair contiguous in the reference (tap_off a permutation of 0..ntaps-1) and everything else padding?  True for the 5x5
// conv (Cout, Cin, 5, 5) and the transposed conv (Cin, Cout, 5, 5) with either flip convention, and for dense layers without a
// flatten permutation.  Checked entry by entry: a layer that fails keeps the gathering reduce.
WgReduceTiledDesc affine_slab_map(const TgLayer& L, const std::vector<int>& fm, int64_t pnumel, std::vector<int>& co_tab, std::vector<int>& ci_tab, int reduce_tci = 16) {
  WgReduceTiledDesc d;
  co_tab.clear();
  ci_tab.clear();
  const int nt = (int)L.taps.size(), CoP = L.CoutPad, CiP = L.Cin, Co = L.Cout;
  if (nt < 1 || nt > 48 || (size_t)nt * CoP * CiP != fm.size() || (CiP & 3)) return d;
  auto at = [&](int t, int co, int ci) { return fm[((size_t)t * CoP + co) * CiP + ci]; };
  int Ci = 0;                                       // real input channels: the non-padding prefix of row 0
  while (Ci < CiP && at(0, 0, Ci) >= 0) ++Ci;
  if (Ci < 2 || Co < 2 || (int64_t)Co * Ci * nt != pnumel) return d;
  // separable form: ref(t, co, ci) = co_off[co] + ci_off[ci] + tap_off[t]; the offsets are linear (co * s_co, ci * s_ci) for the conv
  // layouts and a table along the one axis a dense layer's flatten / unflatten permutation (DenseLayer after (C,H,W)) reorders
  std::vector<int> co_off(Co), ci_off(Ci);
  int base = INT_MAX;
  for (int t = 0; t < nt; ++t) base = std::min(base, at(t, 0, 0));
  for (int co = 0; co < Co; ++co) co_off[co] = at(0, co, 0) - at(0, 0, 0);
  for (int ci = 0; ci < Ci; ++ci) ci_off[ci] = at(0, 0, ci) - at(0, 0, 0);
  std::vector<int> seen(nt, 0);
  for (int t = 0; t < nt; ++t) {
    const int off = at(t, 0, 0) - base;
    if (off < 0 || off >= nt || seen[off]) return d;
    seen[off] = 1;
    d.tap_off[t] = (unsigned char)off;
    d.tap_inv[off] = (unsigned char)t;
  }
  if (base != 0) {   // the (0, 0) pair need not be reference element 0 under a permutation: fold its offset into the filter offsets
    for (int co = 0; co < Co; ++co) co_off[co] += base;
  }
  for (int t = 0; t < nt; ++t)
    for (int co = 0; co < CoP; ++co)
      for (int ci = 0; ci < CiP; ++ci) {
        const int want = (co < Co && ci < Ci) ? co_off[co] + ci_off[ci] + d.tap_off[t] : -1;
        if (at(t, co, ci) != want) return d;
      }
  const int s_co = co_off[1] - co_off[0], s_ci = ci_off[1] - ci_off[0];
  bool co_lin = co_off[0] == 0, ci_lin = true;
  for (int co = 0; co < Co && co_lin; ++co) co_lin = co_off[co] == co * s_co;
  for (int ci = 0; ci < Ci && ci_lin; ++ci) ci_lin = ci_off[ci] == ci * s_ci;
  // one of the two axes must walk the reference contiguously (stride = the tap count) for the write-out / read-in runs
  const bool ci_inner = ci_lin && s_ci == nt, co_inner = co_lin && s_co == nt;
  if (!ci_inner && !co_inner) return d;
  d.ntaps = nt; d.CoutPad = CoP; d.CinPad = CiP; d.Cout = Co; d.Cin = Ci;
  d.s_co = co_lin ? s_co : 0; d.s_ci = ci_lin ? s_ci : 0;
  d.ci_inner = ci_inner;
  if (!co_lin) co_tab = co_off;
  if (!ci_lin) ci_tab = ci_off;
  // 16 x 16 pairs x 25 taps = 26 KB of LDS and runs of 400 floats; one-tap (dense) layers take 64 x 64
  // ... halved along the filters until the launch has 512 workgroups (a 128 x 256 layer is only 128 blocks of 16 x 16, half the chip)
  d.tco = nt == 1 ? 64 : 16;
  d.tci = nt == 1 ? 64 : 16;
  if (nt > 1 && reduce_tci == 32 && CiP % 32 == 0) { d.tci = 32; d.tco = 8; }   // 128-byte runs out of the slabs (wg_reduce_tci)
  while (d.tco > 4 && (long long)((Co + d.tco - 1) / d.tco) * ((Ci + d.tci - 1) / d.tci) < 512) d.tco >>= 1;
  d.valid = true;
  return d;
}

int build_wg_schedule(ian_layer* l, int nimg, WgSchedule** out) {
  auto it = l->wsched.find(nimg);
  if (it != l->wsched.end()) {
    *out = &it->second;
    return 0;
  }
  const TgLayer& L = l->op.fwd;
  WgSchedule S;
  const int M = nimg * L.QH * L.QW;
  int bm, bn;
  if (L.Cout <= 32) { S.cfg = WG_32x128; bm = 32; bn = 128; }
  else if (L.Cin <= 32) { S.cfg = WG_128x32; bm = 128; bn = 32; }
  else { S.cfg = l->ctx.opt.wg_w8 ? (l->ctx.opt.wg_pipe == 3 ? WG_128x128P3 : l->ctx.opt.wg_pipe == 2 ? WG_128x128P2 : l->ctx.opt.wg_pipe ? WG_128x128P : WG_128x128W8) : WG_128x128; bm = 128; bn = 128; }
  const int tiles_co = (std::min(L.CoutPad, round_up(L.Cout, bm)) + bm - 1) / bm;
  const int tiles_ci = (L.Cin + bn - 1) / bn;
  const int ntaps = (int)L.taps.size();
  const long long base = (long long)ntaps * tiles_co * tiles_ci;
  const int steps = (M + 31) / 32;
  const int target = std::max(1, l->ctx.opt.wg_target_items);
  int nsplit = (int)std::max<long long>(1, (target + base - 1) / base);
  nsplit = std::min(nsplit, std::max(1, steps / 4));  // at least 4 K-steps (128 pixels) per item
  // partial-slab workspace cap (ADVICE r5): d_partial holds nsplit copies of the layer's whole slab set; like the tap-GEMM tuner's
  // 512 MB slab limit, never let the split count push one layer's partials past that (a 26 MB slab set x 64 splits would be 1.7 GB)
  const size_t slab_floats = (size_t)ntaps * L.CoutPad * L.Cin;
  const int cap_split = (int)std::max<size_t>(1, ((size_t)512 << 20) / (slab_floats * sizeof(float)));
  nsplit = std::min(nsplit, cap_split);
  // XCD-aware dealing (round 5).  Every item of one pixel range (split) reads the SAME rows of x and dy -- the taps of a layer
  // differ by a shift of at most a few pixels, the channel tiles by the slice of the row they take -- but block b runs on XCD
  // b % 8 and each XCD has its own L2: dealt in (split, tap) order every XCD saw a few taps of EVERY split, i.e. streamed the
  // whole of x and dy through its L2 (8x the unique bytes; profiles/r05_layer_rates.json: backward-weight 0.51-0.65 of the fp32
  // peak in isolation where forward / backward-data of the same layers run at 0.81-0.88).  Now a split's items all go to ONE
  // XCD (split s -> XCD s % 8) and start together, so its rows are fetched into that L2 once and the other taps hit; the split
  // count is rounded to a multiple of 8 so that the XCDs carry equal loads.  Same partial slabs, same fixed-order reduce:
  // bitwise reproducible as before (the sums differ from round 4's only where the split count changed).
  const bool by_xcd = l->ctx.opt.wg_xcd_split && nsplit >= 8;
  if (by_xcd) {
    // which multiple of 8: the one whose item count fills whole rounds of the chip best (the 8-wave tile runs two workgroups
    // per CU = 512 at a time; 800 or 1200 items leave the last round 44 % empty -- measured on dec_conv3a, 1046 -> 1160 us with
    // 8 splits), with a small charge per 8 splits for the partial-slab traffic they add, at least 4 K-steps per item
    int best = 0;
    double best_score = -1.0;
    for (int ns = 8; ns <= 64; ns += 8) {
      if ((steps + ns - 1) / ns < 4 || ns > cap_split) break;
      const long long items = base * ns;
      if (items * 4 < (long long)target * 3 && ns < 64 && (steps + ns + 8 - 1) / (ns + 8) >= 4) continue;   // too few: keep growing
      const long long rounds = (items + 511) / 512;
      const double score = (double)items / (double)(rounds * 512) - 0.02 * (ns / 8);
      if (score > best_score) { best_score = score; best = ns; }
    }
    if (best) nsplit = best;
    else nsplit = std::max(8, std::min(((nsplit + 4) / 8) * 8, cap_split / 8 * 8));
  }
  int per = ((steps + nsplit - 1) / nsplit) * 32;
  nsplit = (M + per - 1) / per;
  if (by_xcd && nsplit % 8) {                            // the ceil above may drop a split: shorten the ranges until the count is a multiple of 8 again
    const int want = ((nsplit + 7) / 8) * 8;
    while (per > 32 && (M + (per - 32) - 1) / (per - 32) <= want) per -= 32;
    nsplit = (M + per - 1) / per;
  }
  S.nsplit = nsplit;
  std::vector<WgItem> items;
  auto emit = [&](std::vector<WgItem>& dst, int s) {
    for (int c = 0; c < (int)L.classes.size(); ++c)
      for (int t = 0; t < L.classes[c].ntaps; ++t)
        for (int a = 0; a < tiles_co; ++a)
          for (int b = 0; b < tiles_ci; ++b) {
            WgItem wi{c, L.classes[c].tap0 + t, a * bm, b * bn, s * per, std::min(M, (s + 1) * per), s, 0};
            dst.push_back(wi);
          }
  };
  if (by_xcd && nsplit % 8 == 0) {
    std::vector<WgItem> lists[8];
    for (int s = 0; s < nsplit; ++s) emit(lists[s % 8], s);
    const size_t longest = lists[0].size();            // equal by construction
    for (size_t k = 0; k < longest; ++k)
      for (int x = 0; x < 8; ++x) items.push_back(lists[x][k]);
  } else {
    for (int s = 0; s < nsplit; ++s) emit(items, s);
  }
  S.nitems = (int)items.size();
  int rc = upload(&l->ctx, items, &S.d_items);
  if (rc) return rc;
  const size_t slab_total = (size_t)ntaps * L.CoutPad * L.Cin;
  const size_t need = slab_total * nsplit;
  if (need > l->partial_cap) {
    if (l->d_partial) LHIP(l, hipFree(l->d_partial));
    LHIP(l, hipMalloc((void**)&l->d_partial, need * sizeof(float)));
    LHIP(l, hipMemset(l->d_partial, 0, need * sizeof(float)));
    // the memset is ordered on the NULL stream only: a caller that launches this layer's backward-weight on a non-blocking
    // stream (ian_train_step's weight-gradient stream) must not start before the zeros have landed
    LHIP(l, hipDeviceSynchronize());
    l->partial_cap = need;
  }
  it = l->wsched.emplace(nimg, S).first;
  *out = &it->second;
  return 0;
}

}  // namespace

extern "C" {

const char* ian_layer_last_error(ian_layer* l) { return l ? l->ctx.err.c_str() : "null layer"; }

int ian_layer_create(const ian_op_desc* desc, int32_t deconv_flip, ian_layer** out) {
  if (!desc || !out) return -1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return -10;  // no HIP device: libian has no CPU fallback
  }
  std::unique_ptr<ian_layer> l(new ian_layer());
  ian_handle* h = &l->ctx;
  h->opt.tg_pos_major = 0;   // the training step keeps image-major rows (its statistics epilogues are defined in that order); IAN_OPTS may say otherwise
  apply_env_options(h->opt);
  h->desc.deconv_flip = deconv_flip;
  h->finalized = true;
  OpPlan& op = l->op;
  op.d = *desc;
  op.name = "L";
  op.d.name = nullptr;
  op.d.bn_name = nullptr;
  op.d.has_bias = 0;
  const int cin = op.d.cin, cout = op.d.cout;
  int rc = 0;
  switch (op.d.kind) {
    case IAN_OP_CONV5S2:
      add_index_param(h, "L.W", {cout, cin, 5, 5});
      if ((rc = pack_conv_fwd(h, op, false)) || (rc = pack_conv_bwd(h, op))) return rc;
      l->pnumel = {(int64_t)cout * cin * 25};
      break;
    case IAN_OP_DECONV5S2:
      if (cout <= 4) return -4;  // image-producing deconvs are not part of the trainable graph (IAN.py:139-181)
      add_index_param(h, "L.W", {cin, cout, 5, 5});
      if ((rc = pack_deconv(h, op))) return rc;
      l->pnumel = {(int64_t)cout * cin * 25};
      break;
    case IAN_OP_DENSE: {
      add_index_param(h, "L.W", {cin, cout});
      std::vector<int> perm;
      bool has = false;
      if ((rc = pack_dense(h, op, perm, has))) return rc;
      l->pnumel = {(int64_t)cout * cin};
      break;
    }
    case IAN_OP_MDC3: {
      if (op.d.n_scales < 0 || op.d.n_scales > IAN_MAX_SCALES) return -1;
      // geometry / buffer sizes from the inference packer (values are overwritten by ian_layer_set_params)
      HostTensor w; w.shape = {cout, cin, 3, 3}; w.data.assign((size_t)cout * cin * 9, 0.f);
      h->params["LW"] = w;
      HostTensor c; c.shape = {cout}; c.data.assign(cout, 0.f);
      h->params["L_coeff_base"] = c;
      for (int i = 0; i < op.d.n_scales; ++i)
        h->params[op.d.scales[i] == 0 ? std::string("L_coeff_1x1") : "L_coeff_" + std::to_string(op.d.scales[i])] = c;
      if ((rc = pack_mdc(h, op))) return rc;
      l->is_mdc = true;
      const MdcTable T = mdc_table(op.d);
      if (T.taps.size() != op.fwd.taps.size() || T.taps.size() > 47) return -4;
      MdcPackArgs& a = l->mdc;
      memset(&a, 0, sizeof a);
      a.ntaps = (int)T.taps.size(); a.cout = cout; a.cin = cin; a.nbranch = (int)T.dil.size();
      a.f_rows = op.fwd.CoutPad; a.f_cols = op.fwd.Cin; a.b_rows = op.bwd.CoutPad; a.b_cols = op.bwd.Cin;
      int e = 0;
      for (int t = 0; t < a.ntaps; ++t) {
        a.tap_start[t] = e;
        for (int b = 0; b < a.nbranch; ++b)
          for (int pq = 0; pq < 9; ++pq)
            if (T.tapof[b][pq] == t) {
              if (e >= 48) return -4;
              a.ent_branch[e] = (unsigned char)b;
              a.ent_pq[e] = (unsigned char)pq;
              ++e;
            }
      }
      a.tap_start[a.ntaps] = e;
      l->pnumel = {(int64_t)cout * cin * 9, cout};
      l->mdc_param_branch[0] = 0;
      int nb = 1;
      for (int i = 0; i < op.d.n_scales; ++i) {
        l->pnumel.push_back(cout);
        l->mdc_param_branch[1 + i] = (op.d.scales[i] == 0) ? -1 : nb++;
      }
      break;
    }
    default:
      return -5;
  }
  if (!l->is_mdc) {
    std::vector<int> fm = slab_to_map(op.fwd.h_w), bm;
    if (op.bwd.valid) bm = slab_to_map(op.bwd.h_w);
    std::vector<int> inv((size_t)l->pnumel[0], -1);
    for (size_t i = 0; i < fm.size(); ++i)
      if (fm[i] >= 0) inv[fm[i]] = (int)i;
    l->fwd_count = fm.size();
    l->bwd_count = bm.size();
    std::vector<int> cot, cit;
    l->rtd = affine_slab_map(op.fwd, fm, l->pnumel[0], cot, cit, l->ctx.opt.wg_reduce_tci);
    if ((!cot.empty() && (rc = upload(h, cot, &l->d_rt_tab[0]))) || (!cit.empty() && (rc = upload(h, cit, &l->d_rt_tab[1])))) return rc;
    l->rtd.co_off = l->d_rt_tab[0]; l->rtd.ci_off = l->d_rt_tab[1];
    if (op.bwd.valid) {
      l->rtd_b = affine_slab_map(op.bwd, bm, l->pnumel[0], cot, cit, l->ctx.opt.wg_reduce_tci);
      if ((!cot.empty() && (rc = upload(h, cot, &l->d_rt_tab[2]))) || (!cit.empty() && (rc = upload(h, cit, &l->d_rt_tab[3])))) return rc;
      l->rtd_b.co_off = l->d_rt_tab[2]; l->rtd_b.ci_off = l->d_rt_tab[3];
    }
    if ((rc = upload(h, fm, &l->d_fwd_map)) || (rc = upload(h, bm, &l->d_bwd_map)) || (rc = upload(h, inv, &l->d_inv_map))) return rc;
  }
  if ((rc = upload_layer(h, op.fwd)) || (rc = upload_layer(h, op.bwd))) return rc;
  if (l->is_mdc) {
    l->mdc.slab_f = op.fwd.d_w;
    l->mdc.slab_b = op.bwd.d_w;
    if (hipMalloc((void**)&l->d_dS, op.fwd.w_floats * sizeof(float)) != hipSuccess) return -2;
  }
  h->params.clear();
  *out = l.release();
  return 0;
}

int32_t ian_layer_num_params(ian_layer* l) { return l ? (int32_t)l->pnumel.size() : -1; }
int64_t ian_layer_param_numel(ian_layer* l, int32_t which) {
  return (l && which >= 0 && which < (int)l->pnumel.size()) ? l->pnumel[which] : -1;
}

int ian_layer_set_params(ian_layer* l, const float* const* params, int32_t nparams, void* stream) {
  if (!l || !params || nparams != (int)l->pnumel.size()) return lfail(l, -1, "ian_layer_set_params: expected %d parameter tensors", l ? (int)l->pnumel.size() : 0);
  hipStream_t st = (hipStream_t)stream;
  if (!l->is_mdc) {
    l->op.fwd.wsplit_valid = l->op.bwd.wsplit_valid = false;   // the slabs change: a split-bf16 copy (tg_bf16x3) is re-made at its next use
    const bool tiled = l->ctx.opt.pack_tiled != 0;
    if (tiled && l->rtd.valid) LHIP(l, launch_pack_tiled(l->rtd, params[0], l->op.fwd.d_w, st));
    else LHIP(l, launch_gather_pack(params[0], l->d_fwd_map, l->op.fwd.d_w, (long long)l->fwd_count, st));
    if (l->op.bwd.valid) {
      if (tiled && l->rtd_b.valid) LHIP(l, launch_pack_tiled(l->rtd_b, params[0], l->op.bwd.d_w, st));
      else LHIP(l, launch_gather_pack(params[0], l->d_bwd_map, l->op.bwd.d_w, (long long)l->bwd_count, st));
    }
    return 0;
  }
  l->op.fwd.wsplit_valid = l->op.bwd.wsplit_valid = false;
  MdcPackArgs& a = l->mdc;
  a.W = params[0];
  a.coeff_1x1 = nullptr;
  for (int i = 1; i < nparams; ++i) {
    const int b = (i == 1) ? 0 : l->mdc_param_branch[i - 1];
    if (i == 1) a.coeff[0] = params[1];
    else if (b < 0) a.coeff_1x1 = params[i];
    else a.coeff[b] = params[i];
  }
  LHIP(l, launch_mdc_pack(a, st));
  return 0;
}

int ian_layer_stats_next(ian_layer* l, int32_t mode, const float* a, const float* yraw, const float* mean, const float* inv_std,
                         int32_t act, double* partial, int64_t cap_doubles) {
  if (!l || mode < 0 || mode > 2 || (mode && (!partial || cap_doubles <= 0)) || (mode == 2 && act && !a) ||
      (mode == 2 && yraw && (!mean || !inv_std)))
    return lfail(l, -1, "bad argument to ian_layer_stats_next");
  TgStats& s = l->ctx.stats_next;
  s = TgStats();
  s.mode = mode; s.a = a; s.yraw = yraw; s.mean = mean; s.inv_std = inv_std; s.act = act; s.partial = partial;
  l->ctx.stats_cap = cap_doubles;
  return 0;
}
int32_t ian_layer_stats_chunks(ian_layer* l) { return l ? l->ctx.stats_chunks_last : 0; }

int ian_layer_forward(ian_layer* l, const float* x, int32_t n, float* y, int32_t y_stride, const float* bias,
                      const float* res, int32_t act, void* stream) {
  if (!l || !x || !y || n <= 0) return lfail(l, -1, "bad argument to ian_layer_forward");
  struct OneShot { ian_handle* h; ~OneShot() { h->stats_next.mode = 0; } } one_shot{&l->ctx};   // a VALU path below leaves no request behind
  l->ctx.stats_chunks_last = 0;
  TgEpilogue e;
  e.scale = nullptr; e.shift = bias; e.res = res; e.yfwd = nullptr; e.act = act; e.scale_period = 0; e.mode = TG_EPI_FWD;
  if (y_stride <= 0) y_stride = round_up(l->op.fwd.Cout, 32);
  if (l->op.d.kind == IAN_OP_MDC3 && mdc_head_eligible(&l->ctx, l->op)) {  // RGB-Beta head: VALU kernel
    const TgLayer& L = l->op.fwd;
    MdcHeadArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.H = L.IH; a.W = L.IW; a.xs = L.Cin; a.ntaps = (int)L.taps.size();
    a.w_tap_stride = (long long)L.CoutPad * L.Cin;
    for (int t = 0; t < a.ntaps; ++t) { a.dy[t] = (signed char)L.taps[t].dy; a.dx[t] = (signed char)L.taps[t].dx; }
    if (bias) return lfail(l, -1, "head layers take no bias");
    for (int co = 0; co < L.Cout; ++co) {
      a.w[co] = L.d_w + (size_t)co * L.Cin; a.res[co] = res; a.y[co] = y; a.ys[co] = y_stride; a.yc[co] = co; a.act[co] = act;
      a.scale[co] = 1.f; a.shift[co] = 0.f;
    }
    LHIP(l, launch_mdc_head(a, n, L.Cin, L.Cout, (hipStream_t)stream));
    return 0;
  }
  if (l->op.d.kind == IAN_OP_MDC3 && mdc_thin_eligible(&l->ctx, l->op.fwd)) {
    MdcThinArgs a;
    mdc_thin_fill(a, l->op.fwd, x, l->op.fwd.Cin, y, y_stride, n, &l->ctx);
    a.res = res; a.shift = bias; a.act = act;
    LHIP(l, launch_mdc_thin(a, (hipStream_t)stream));
    return 0;
  }
  return run_tapgemm(&l->ctx, l->op.fwd, n, x, y, y_stride, e, (hipStream_t)stream);
}

int ian_layer_backward_data(ian_layer* l, const float* dy, int32_t n, float* dx, int32_t dx_stride, int32_t accumulate,
                            void* stream) {
  if (!l || !dy || !dx || n <= 0) return lfail(l, -1, "bad argument to ian_layer_backward_data");
  struct OneShot { ian_handle* h; ~OneShot() { h->stats_next.mode = 0; } } one_shot{&l->ctx};
  l->ctx.stats_chunks_last = 0;
  if (!l->op.bwd.valid) return lfail(l, -9, "layer has no backward-data form");
  TgEpilogue e;
  e.scale = nullptr; e.shift = nullptr; e.res = accumulate ? dx : nullptr; e.yfwd = nullptr; e.act = IAN_ACT_NONE;
  e.scale_period = 0; e.mode = TG_EPI_BWD;
  if (dx_stride <= 0) dx_stride = round_up(l->op.bwd.Cout, 32);
  if (l->op.d.kind == IAN_OP_MDC3 && mdc_thin_eligible(&l->ctx, l->op.bwd)) {
    MdcThinArgs a;
    mdc_thin_fill(a, l->op.bwd, dy, l->op.bwd.Cin, dx, dx_stride, n, &l->ctx);
    a.res = accumulate ? dx : nullptr;
    LHIP(l, launch_mdc_thin(a, (hipStream_t)stream));
    return 0;
  }
  return run_tapgemm(&l->ctx, l->op.bwd, n, dy, dx, dx_stride, e, (hipStream_t)stream);
}

int ian_layer_backward_weight(ian_layer* l, const float* x, const float* dy, int32_t n, float* const* dparams,
                              int32_t nparams, int32_t accumulate, void* stream) {
  if (!l || !x || !dy || !dparams || n <= 0 || nparams != (int)l->pnumel.size()) return lfail(l, -1, "bad argument to ian_layer_backward_weight");
  hipStream_t st = (hipStream_t)stream;
  const TgLayer& L = l->op.fwd;
  const bool thin_in = l->is_mdc && l->ctx.opt.mdc_head && L.cin_real <= 4 && L.Cout <= 4 && (L.IH % 4) == 0 && (L.IW % 16) == 0 &&
                       L.taps.size() <= 48 && mdc_thin_eligible(&l->ctx, L);
  if (l->is_mdc && (mdc_head_eligible(&l->ctx, l->op) || thin_in)) {  // RGB-Beta head: VALU backward-weight, no padded MFMA tile
    const int kcin = thin_in ? 4 : L.Cin;  // thin layers: the 2-4 real channels (+ zero padding) of the 32-float pixel row
    MdcHeadWgradArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.dy = dy; a.H = L.IH; a.W = L.IW; a.xs = L.Cin; a.dys = round_up(L.Cout, 32); a.ntaps = (int)L.taps.size();
    a.total_tiles = n * (L.IH / 4) * (L.IW / 16);
    for (int t = 0; t < a.ntaps; ++t) { a.dy_[t] = (signed char)L.taps[t].dy; a.dx_[t] = (signed char)L.taps[t].dx; }
    const int nblocks = std::min(a.total_tiles, 512);
    const int cpad = L.Cout <= 2 ? 2 : 4;
    const size_t need = (size_t)nblocks * a.ntaps * cpad * kcin;
    if (need > l->partial_cap) {
      if (l->d_partial) LHIP(l, hipFree(l->d_partial));
      LHIP(l, hipMalloc((void**)&l->d_partial, need * sizeof(float)));
      l->partial_cap = need;
    }
    a.partial = l->d_partial;
    LHIP(l, hipMemsetAsync(l->d_dS, 0, l->op.fwd.w_floats * sizeof(float), st));
    LHIP(l, launch_mdc_head_wgrad(a, nblocks, kcin, L.Cout, l->d_dS, L.CoutPad, L.Cin, st));
    MdcCoeffGrads g;
    memset(&g, 0, sizeof g);
    g.d[0] = dparams[1];
    for (int i = 2; i < nparams; ++i) {
      const int b = l->mdc_param_branch[i - 1];
      if (b < 0) g.d1x1 = dparams[i];
      else g.d[b] = dparams[i];
    }
    LHIP(l, launch_mdc_unpack_grad(l->mdc, l->d_dS, dparams[0], g, accumulate, st));
    return 0;
  }
  WgSchedule* S;
  int rc = build_wg_schedule(l, n, &S);
  if (rc) return rc;
  WgParams p;
  p.x = x; p.dy = dy; p.partial = l->d_partial; p.items = S->d_items; p.classes = L.d_classes; p.taps = L.d_taps;
  p.M = n * L.QH * L.QW; p.IH = L.IH; p.IW = L.IW; p.Cin = L.Cin;
  p.qw_shift = ilog2_exact(L.QW); p.qhw_shift = ilog2_exact(L.QH * L.QW);
  p.si = L.si; p.by = L.by; p.bx = L.bx; p.so = L.so; p.OH = L.OH; p.OW = L.OW;
  p.dy_stride = (l->op.d.kind == IAN_OP_DENSE && l->op.d.unflat_c > 0) ? L.Cout : round_up(L.Cout, 32);
  p.CoutPad = L.CoutPad; p.CinPad = L.Cin;
  p.slab_total = (long long)L.taps.size() * L.CoutPad * L.Cin;
  const size_t xb = (size_t)n * L.IH * L.IW * L.Cin * 4, yb = (size_t)n * L.OH * L.OW * p.dy_stride * 4;
  if (xb > 0xFFFFFFF0ull || yb > 0xFFFFFFF0ull) return lfail(l, -7, "batch %d exceeds the 4 GiB buffer-descriptor range", n);
  p.x_bytes = (unsigned)xb; p.dy_bytes = (unsigned)yb;
  LHIP(l, launch_tapwgrad(S->cfg, p, S->nitems, st));
  if (!l->is_mdc) {
    if (l->rtd.valid && l->ctx.opt.wg_reduce_tiled)
      LHIP(l, launch_wgrad_reduce_tiled(l->rtd, l->d_partial, p.slab_total, S->nsplit, dparams[0], accumulate, st));
    else
      LHIP(l, launch_wgrad_reduce(l->d_partial, p.slab_total, S->nsplit, l->d_inv_map, dparams[0], l->pnumel[0], accumulate, st));
    return 0;
  }
  LHIP(l, launch_wgrad_reduce(l->d_partial, p.slab_total, S->nsplit, nullptr, l->d_dS, p.slab_total, 0, st));
  MdcCoeffGrads g;
  memset(&g, 0, sizeof g);
  g.d[0] = dparams[1];
  for (int i = 2; i < nparams; ++i) {
    const int b = l->mdc_param_branch[i - 1];
    if (b < 0) g.d1x1 = dparams[i];
    else g.d[b] = dparams[i];
  }
  LHIP(l, launch_mdc_unpack_grad(l->mdc, l->d_dS, dparams[0], g, accumulate, st));
  return 0;
}

int ian_layer_head6_forward(ian_layer* l0, ian_layer* l1, ian_layer* l2, const float* x, int32_t n, float* y0, float* y1,
                            float* y2, int32_t y_stride, int32_t act0, int32_t act1, int32_t act2, void* stream) {
  if (!l0 || !l1 || !l2 || !x || !y0 || !y1 || !y2 || n <= 0) return lfail(l0, -1, "bad argument to ian_layer_head6_forward");
  hipStream_t st = (hipStream_t)stream;
  ian_layer* ls[3] = {l0, l1, l2};
  const TgLayer& L = l0->op.fwd;
  for (ian_layer* l : ls) {
    const TgLayer& M = l->op.fwd;
    if (!l->is_mdc || l->op.d.cin != 128 || l->op.d.cout != 2 || l->op.d.in_w != 64 || M.Cin != 128 || !same_taps(L, M)) return -4;
  }
  if (L.taps.size() > 37) return -4;
  ian_handle* h = &l0->ctx;
  HeadPlan& P = h->head;   // tables + compact workspace live in the first layer's context
  if (!P.d_itab) {
    std::vector<int> itab(44, -1), used(9, 0);
    int halo = 0;
    for (size_t t = 0; t < L.taps.size(); ++t) {
      const int dy = L.taps[t].dy, dx = L.taps[t].dx;
      if (dy < -4 || dy > 4 || dx < -63 || dx > 63) return -4;
      const int g = dy == 0 ? 0 : (dy < 0 ? dy + 5 : dy + 4), cap = g == 0 ? 12 : 4, s0 = g == 0 ? 0 : 12 + (g - 1) * 4;
      if (used[g] >= cap) return -4;
      itab[s0 + used[g]++] = (int)t | ((dx + 64) << 8);
      halo = std::max(halo, std::abs(dy));
    }
    P.halo = halo;
    int rc = upload(h, itab, &P.d_itab);
    if (rc) return rc;
    LHIP(l0, hipMalloc((void**)&P.d_ftab, 32 * sizeof(float)));
  }
  const int acts[3] = {act0, act1, act2};
  const int act_key = 1 + act0 + 16 * act1 + 256 * act2;
  if (P.opBeta != act_key) {   // (field reused as "epilogue table uploaded for these activations"): synchronous, first call only
    float ftab[32] = {0};
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 2; ++c) { ftab[2 * k + c] = 1.f; ftab[16 + 2 * k + c] = (float)acts[k]; }
    LHIP(l0, hipStreamSynchronize(st));
    LHIP(l0, hipMemcpy(P.d_ftab, ftab, sizeof ftab, hipMemcpyHostToDevice));
    P.opBeta = act_key;
  }
  const int H = l0->op.d.in_h, W = l0->op.d.in_w;
  const size_t need = (size_t)n * H * W * 8;
  if (need > P.comp_cap) {
    if (P.d_comp) LHIP(l0, hipFree(P.d_comp));
    LHIP(l0, hipMalloc((void**)&P.d_comp, need * sizeof(float)));
    P.comp_cap = need;
  }
  HeadFusedArgs a;
  memset(&a, 0, sizeof a);
  a.x = x; a.w0 = l0->op.fwd.d_w; a.w1 = l1->op.fwd.d_w; a.w2 = l2->op.fwd.d_w; a.out = P.d_comp; a.itab = P.d_itab; a.ftab = P.d_ftab;
  a.H = H; a.W = W; a.xs = L.Cin; a.ntaps = (int)L.taps.size(); a.halo = P.halo;
  a.w_tap_stride = (long long)L.CoutPad * L.Cin;
  a.bands = row_bands(n, h->opt.head_wgs, H, 1, 2 * P.halo);   // as run_head_fused (ian_rt_exec.inc)
  LHIP(l0, launch_head6(a, n, st));
  LHIP(l0, launch_head6_scatter(P.d_comp, y0, y1, y2, y_stride, (long long)n * H * W, st));
  return 0;
}

int ian_layer_head6_backward(ian_layer* l0, ian_layer* l1, ian_layer* l2, const float* x, const float* dy0, const float* dy1,
                             const float* dy2, int32_t n, int32_t dy_stride, float* dx, int32_t dx_stride, int32_t dx_accumulate,
                             float* const* dparams0, float* const* dparams1, float* const* dparams2, int32_t nparams,
                             int32_t accumulate, void* stream) {
  const bool want_w = dparams0 || dparams1 || dparams2;
  if (l0) l0->ctx.stats_chunks_last = 0;
  if (!l0 || !l1 || !l2 || !dy0 || !dy1 || !dy2 || n <= 0 || (!dx && !want_w) || (want_w && (!x || !dparams0 || !dparams1 || !dparams2)))
    return lfail(l0, -1, "bad argument to ian_layer_head6_backward");
  hipStream_t st = (hipStream_t)stream;
  ian_layer* ls[3] = {l0, l1, l2};
  float* const* dps[3] = {dparams0, dparams1, dparams2};
  const TgLayer& L = l0->op.fwd;
  for (ian_layer* l : ls) {
    const TgLayer& M = l->op.fwd;
    if (!l->is_mdc || l->op.d.cin != 128 || l->op.d.cout != 2 || M.Cin != 128 || !same_taps(L, M) ||
        (want_w && nparams != (int)l->pnumel.size()))
      return -4;
  }
  const int ntaps = (int)L.taps.size(), nout = 6 * ntaps, zs = round_up(nout, 32);
  const int H = l0->op.d.in_h, W = l0->op.d.in_w;
  const long long npix = (long long)n * H * W;
  if (npix * zs * 4 > 0xFFFFFFF0ll || npix > 0x7FFFFFFFll) return -4;   // buffer-descriptor range of the helper GEMMs
  if (!l0->h6_helper) {
    ian_op_desc d;
    memset(&d, 0, sizeof d);
    d.kind = IAN_OP_DENSE; d.cin = 128; d.cout = nout; d.in_h = d.in_w = 1; d.src2 = d.src3 = -1;
    int rc = ian_layer_create(&d, 1, &l0->h6_helper);
    if (rc) return lfail(l0, rc, "head6 backward: helper layer creation failed (%d)", rc);
    // the helper is created here, after ian_trainer_autotune has walked the layers: give its backward-data GEMM (npix x 6*taps -> 128,
    // 7 K-steps per item) the schedule the tuner picks for every other large-M launch instead of the untuned 4-wave default
    // (round 6: 480 -> 330 us per call at 128 images)
    {
      TgChoice c;
      c.cfg = TG_128x128W8; c.max_steps = 0; c.variant = TG_SCHED_AHEAD2; c.fused = 0;
      l0->h6_helper->op.bwd.choice[(int)npix] = c;
    }
    std::vector<int> tp(ntaps);
    for (int t = 0; t < ntaps; ++t) tp[t] = (L.taps[t].dy + 64) | ((L.taps[t].dx + 64) << 8);
    if ((rc = upload(&l0->ctx, tp, &l0->h6_taps))) return rc;
    LHIP(l0, hipMalloc((void**)&l0->h6_dW, (size_t)2 * 128 * nout * sizeof(float)));   // [0]: dW of the helper, [1]: its W
  }
  const size_t need = (size_t)npix * zs;
  if (need > l0->h6_Z_cap) {
    if (l0->h6_Z) LHIP(l0, hipFree(l0->h6_Z));
    LHIP(l0, hipMalloc((void**)&l0->h6_Z, need * sizeof(float)));
    l0->h6_Z_cap = need;
  }
  int max_shift = 0;
  for (auto& tp : L.taps) max_shift = std::max(max_shift, std::max(std::abs((int)tp.dy), std::abs((int)tp.dx)));
  LHIP(l0, launch_head6_zbuild(dy0, dy1, dy2, dy_stride, l0->h6_Z, zs, H, W, ntaps, l0->h6_taps, npix, st, l0->ctx.opt.zbuild_rows ? max_shift : -1));
  int rc;
  if (dx) {  // dx[q][c] = sum_j Z[q][j] * Wcat[c][j], Wcat[c][(t,k,f)] = slab_k[t][f][c]: the helper's backward-data GEMM
    float* wcat = l0->h6_dW + (size_t)128 * nout;
    for (int k = 0; k < 3; ++k)
      LHIP(l0, launch_head6_wcat(ls[k]->op.fwd.d_w, ls[k]->op.fwd.CoutPad, ls[k]->op.fwd.Cin, k, ntaps, wcat, nout, st));
    float* wp[1] = {wcat};
    if ((rc = ian_layer_set_params(l0->h6_helper, wp, 1, stream))) return lfail(l0, rc, "head6 backward-data GEMM: %s", ian_layer_last_error(l0->h6_helper));
    // a statistics request on the first layer (ian_layer_stats_next) rides on the helper's GEMM, which is what stores dx
    l0->h6_helper->ctx.stats_next = l0->ctx.stats_next;
    l0->h6_helper->ctx.stats_cap = l0->ctx.stats_cap;
    l0->ctx.stats_next.mode = 0;
    if ((rc = ian_layer_backward_data(l0->h6_helper, l0->h6_Z, (int32_t)npix, dx, dx_stride, dx_accumulate, stream)))
      return lfail(l0, rc, "head6 backward-data GEMM: %s", ian_layer_last_error(l0->h6_helper));
    l0->ctx.stats_chunks_last = l0->h6_helper->ctx.stats_chunks_last;
  }
  if (!want_w) return 0;
  float* dw_ptr[1] = {l0->h6_dW};
  rc = ian_layer_backward_weight(l0->h6_helper, x, l0->h6_Z, (int32_t)npix, dw_ptr, 1, 0, stream);
  if (rc) return lfail(l0, rc, "head6 backward-weight GEMM: %s", ian_layer_last_error(l0->h6_helper));
  for (int k = 0; k < 3; ++k) {
    ian_layer* l = ls[k];
    LHIP(l, hipMemsetAsync(l->d_dS, 0, l->op.fwd.w_floats * sizeof(float), st));
    LHIP(l, launch_head6_dS_scatter(l0->h6_dW, nout, k, ntaps, l->d_dS, l->op.fwd.CoutPad, l->op.fwd.Cin, st));
    MdcCoeffGrads g;
    memset(&g, 0, sizeof g);
    g.d[0] = dps[k][1];
    for (int i = 2; i < nparams; ++i) {
      const int b = l->mdc_param_branch[i - 1];
      if (b < 0) g.d1x1 = dps[k][i];
      else g.d[b] = dps[k][i];
    }
    LHIP(l, launch_mdc_unpack_grad(l->mdc, l->d_dS, dps[k][0], g, accumulate, st));
  }
  return 0;
}

int ian_layer_autotune(ian_layer* l, int32_t n, float* scratch_a, float* scratch_b, int64_t cap_floats, void* stream) {
  if (!l || !scratch_a || !scratch_b || n <= 0) return lfail(l, -1, "bad argument to ian_layer_autotune");
  hipStream_t st = (hipStream_t)stream;
  ian_handle* h = &l->ctx;
  TgEpilogue e;
  e.scale = nullptr; e.shift = nullptr; e.res = nullptr; e.yfwd = nullptr; e.act = IAN_ACT_NONE; e.scale_period = 0; e.mode = TG_EPI_FWD;
  struct Dir { TgLayer* L; float* in; float* out; };
  Dir dirs[2] = {{&l->op.fwd, scratch_a, scratch_b}, {&l->op.bwd, scratch_b, scratch_a}};
  for (int d = 0; d < 2; ++d) {
    TgLayer& L = *dirs[d].L;
    if (!L.valid) continue;
    if (d == 0 && l->op.d.kind == IAN_OP_MDC3 && (mdc_head_eligible(h, l->op) || mdc_thin_eligible(h, L))) continue;  // VALU kernels
    if (d == 1 && l->op.d.kind == IAN_OP_MDC3 && mdc_thin_eligible(h, L)) continue;
    const int ystride = round_up(L.Cout, 32);
    const int64_t need_in = (int64_t)n * L.IH * L.IW * L.Cin, need_out = (int64_t)n * L.OH * L.OW * ystride;
    if (need_in > cap_floats || need_out > cap_floats) return lfail(l, -7, "ian_layer_autotune: scratch buffers too small (%lld floats needed)", (long long)std::max(need_in, need_out));
    float* in = dirs[d].in;
    float* out = dirs[d].out;
    int rc = tune_layer(h, L, n, st, [&]() { return run_tapgemm(h, L, n, in, out, ystride, e, st); }, nullptr, nullptr);
    if (rc) return rc;
  }
  return 0;
}

void ian_layer_destroy(ian_layer* l) {
  IAN_GUARD_CHECK("ian_layer_destroy");
  if (!l) return;
  if (l->h6_helper) ian_layer_destroy(l->h6_helper);
  for (void* p : {(void*)l->h6_Z, (void*)l->h6_dW, (void*)l->h6_taps})
    if (p) (void)hipFree(p);
  for (TgLayer* L : {&l->op.fwd, &l->op.bwd}) {
    free_schedules(*L);
    if (L->d_w) (void)hipFree(L->d_w);
    if (L->d_wsplit) (void)hipFree(L->d_wsplit);
    if (L->d_classes) (void)hipFree(L->d_classes);
    if (L->d_taps) (void)hipFree(L->d_taps);
  }
  for (auto& kv : l->wsched)
    if (kv.second.d_items) (void)hipFree(kv.second.d_items);
  for (void* p : {(void*)l->d_rt_tab[0], (void*)l->d_rt_tab[1], (void*)l->d_rt_tab[2], (void*)l->d_rt_tab[3]})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)l->d_fwd_map, (void*)l->d_bwd_map, (void*)l->d_inv_map, (void*)l->d_partial, (void*)l->d_dS,
                  (void*)l->ctx.d_slab, (void*)l->ctx.head.d_itab, (void*)l->ctx.head.d_ftab, (void*)l->ctx.head.d_comp})
    if (p) (void)hipFree(p);
  delete l;
}

}  // extern "C"

