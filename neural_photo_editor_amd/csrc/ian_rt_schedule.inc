// ian_rt_schedule.inc -- tapgemm scheduling: tile shape, row order and split policy per launch; the item list itself is ian_tg_plan.h's.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
namespace {

// ----- scheduling: tiles, split-K, heavy-first + XCD-aware item order ---------------------------------
static int count_tiles(const TgLayer& L, int M, int cfg) {
  const TgShape sh = tg_shape(cfg);
  return ((M + sh.bm - 1) / sh.bm) * ((L.Cout + sh.bn - 1) / sh.bn) * (int)L.classes.size();
}

int pick_config(const ian_handle* h, const TgLayer& L, int M) {
  if (h->opt.tg_cfg >= 0 && h->opt.tg_cfg < TG_NCONFIG) {
    const TgShape s = tg_shape(h->opt.tg_cfg);
    if (L.CoutPad % s.bn == 0) return h->opt.tg_cfg;
  }
  if (L.Cout <= 32) return TG_128x32;
  if (M <= 32) return TG_32x128;
  if (M <= 64) return TG_64x64;
  // Large output maps: a smaller tile that fills the chip WITHOUT split-K beats 128x128 + slabs (the slab
  // write + reduce pass moves the whole output several times).  Small-M / huge-K layers keep 128x128 + split-K.
  if (h->opt.tg_prefer_nosplit) {
    const int order[3] = {TG_128x128, TG_128x64, TG_64x64};
    for (int c : order)
      if (count_tiles(L, M, c) >= h->opt.tg_no_split_items) return c;
    if ((long long)M * L.Cout >= (long long)h->opt.tg_nosplit_min_out) return TG_64x64;
  }
  return TG_128x128;
}

// does the opt-in split-bf16 kernel take a launch of M rows over nimg images? (the tile must be one it is instantiated for as well)
static inline bool bf16x3_applies(const ian_handle* h, int M, int nimg) {
  return h->opt.tg_bf16x3 && M >= h->opt.tg_bf16x3_min_m && nimg >= h->opt.tg_bf16x3_min_images;
}

// Workgroups of a tile shape one CU holds at once (LDS of the two staging buffers, 160 KB per CU; waves per SIMD <= 8 is never the
// limit for these shapes): what "one round" of a launch is.
static int tg_slots(int cfg) {
  const TgShape sh = tg_shape(cfg);
  const size_t lds = (size_t)2 * (sh.bm + sh.bn) * 36 * sizeof(float);
  int per_cu = (int)((160u << 10) / lds);
  const int waves = (cfg == TG_128x128W8 || cfg == TG_128x64W8) ? 8 : 4;
  per_cu = std::min(per_cu, 32 / waves);
  return 256 * std::max(1, per_cu);
}

// the planner's view of a layer at one batch, tile shape and split limit (ian_tg_plan.h)
static TgPlanIn plan_input(const ian_handle* h, const TgLayer& L, int nimg, int cfg, int max_steps, int pos_major) {
  const TgShape sh = tg_shape(cfg);
  TgPlanIn in;
  in.nimg = nimg; in.QH = L.QH; in.QW = L.QW; in.IH = L.IH; in.IW = L.IW; in.si = L.si; in.by = L.by; in.bx = L.bx;
  in.Cin = L.Cin; in.Cout = L.Cout;
  in.classes = L.classes.data(); in.ncls = (int)L.classes.size(); in.taps = L.taps.data(); in.ntaps_total = (int)L.taps.size();
  in.bm = sh.bm; in.bn = sh.bn; in.pos_major = pos_major; in.max_steps = max_steps;
  in.opt_split = h->opt.tg_split; in.opt_no_split_items = h->opt.tg_no_split_items; in.opt_target_items = h->opt.tg_target_items;
  in.opt_min_steps = h->opt.tg_min_steps; in.xcd_group = h->opt.tg_xcd_group; in.xcd_spatial = h->opt.tg_xcd_spatial;
  return in;
}

// May a launch of this layer over nimg images take position-major rows (option tg_pos_major)?  2: always (tests: any batch, ragged rows
// of a position are padding).  1: batches that are a power of two >= 64 -- a tile then covers at most two positions -- unless the
// split-bf16 kernel (image-major only) takes the launch or a statistics request is waiting: the statistics' chunk boundaries are defined
// in the image-major row order (TgStats), and a request that meets a position-major schedule later is declined like one that meets a
// split one (run_tapgemm).
static bool pos_major_allowed(const ian_handle* h, const TgLayer& L, int nimg) {
  if (bf16x3_applies(h, nimg * L.QH * L.QW, nimg) || ilog2_exact(L.QH * L.QW) < 0) return false;
  if (h->opt.tg_pos_major == 2) return true;
  return h->opt.tg_pos_major == 1 && nimg >= 64 && ilog2_exact(nimg) >= 0 && h->stats_next.mode == 0;
}

void build_schedule(const ian_handle* h, const TgLayer& L, int nimg, Schedule& S, const TgChoice& ch) {
  const int M = nimg * L.QH * L.QW;
  S.cfg = (ch.cfg >= 0 && ch.cfg < TG_NCONFIG && L.CoutPad % tg_shape(ch.cfg).bn == 0) ? ch.cfg : pick_config(h, L, M);
  S.variant = ch.variant;
  S.fused = ch.fused >= 0 ? ch.fused : (M <= h->opt.tg_fuse_max_m ? h->opt.tg_fuse : 0);
  if (!tg_fuse_supported(S.cfg) || S.fused < 0 || S.fused > 2) S.fused = 0;   // the large tiles are compiled without the in-launch combine; anything out of range = reduce launch
  S.bf16x3 = bf16x3_applies(h, M, nimg) && tg_bf16x3_supported(S.cfg);
  if (S.bf16x3) S.fused = 0;   // the split-bf16 kernel writes plain slabs: always the reduce launch
  // row order: forced by the option, the tuner's choice, or -- untuned -- position-major where the launch model predicts a shorter launch
  const bool allowed = pos_major_allowed(h, L, nimg) && !S.bf16x3;
  TgPlan P;
  if (allowed && h->opt.tg_pos_major != 2 && ch.pos_major < 0) {
    TgPlan Q;
    tg_plan(plan_input(h, L, nimg, S.cfg, ch.max_steps, 0), P);
    tg_plan(plan_input(h, L, nimg, S.cfg, ch.max_steps, 1), Q);
    auto makespan = [&](const TgPlan& pl) {
      std::vector<int> lens;
      for (auto& it : pl.items)
        if (it.ks1 > it.ks0) lens.push_back(it.ks1 - it.ks0);
      return tg_model_makespan(lens, 0, tg_slots(S.cfg));
    };
    if (Q.steps < P.steps && makespan(Q) < makespan(P)) P = std::move(Q);
  } else {
    tg_plan(plan_input(h, L, nimg, S.cfg, ch.max_steps, allowed && (h->opt.tg_pos_major == 2 || ch.pos_major == 1) ? 1 : 0), P);
  }
  S.pos_major = P.b_shift >= 0;
  if (S.pos_major) S.fused = 0;   // the in-launch combine skips row quads beyond M: an image-major notion
  S.M = P.M;
  S.b_shift = P.b_shift;
  S.steps = P.steps;
  S.steps_full = P.steps_full;
  S.max_nsplit = P.max_nsplit;
  S.h_items = std::move(P.items);
  S.h_tiles = std::move(P.tiles);
  S.h_ttaps = std::move(P.taptab);
  S.nitems = (int)S.h_items.size();
  S.ntiles = P.split ? (int)S.h_tiles.size() : 0;
  S.slab_tiles = P.slab_tiles;
}

int get_schedule(ian_handle* h, TgLayer& L, int nimg, Schedule** out) {
  auto it = L.sched.find(nimg);
  if (it == L.sched.end()) {
    Schedule S;
    auto chit = L.choice.find(nimg);
    build_schedule(h, L, nimg, S, chit == L.choice.end() ? TgChoice() : chit->second);
    int rc;
    if ((rc = upload(h, S.h_items, &S.d_items))) return rc;
    if ((rc = upload(h, S.h_tiles, &S.d_tiles))) return rc;
    if ((rc = upload(h, S.h_ttaps, &S.d_ttaps))) return rc;
    if (S.ntiles > 0) {
      HIPCHK(h, hipMalloc((void**)&S.d_counters, S.ntiles * sizeof(int)));
      HIPCHK(h, hipMemset(S.d_counters, 0, S.ntiles * sizeof(int)));
      if (S.fused == 2) {
        const TgShape rs = tg_shape(S.cfg);
        HIPCHK(h, hipMalloc((void**)&S.d_raw, (size_t)S.ntiles * rs.bm * rs.bn * sizeof(float)));
        HIPCHK(h, hipMemset(S.d_raw, 0, (size_t)S.ntiles * rs.bm * rs.bn * sizeof(float)));
      }
    }
    const TgShape sh = tg_shape(S.cfg);
    const size_t need = S.slab_tiles * sh.bm * sh.bn;
    if (need > h->slab_cap) {
      if (h->d_slab) HIPCHK(h, hipFree(h->d_slab));
      HIPCHK(h, hipMalloc((void**)&h->d_slab, need * sizeof(float)));
      h->slab_cap = need;
      ++h->alloc_epoch;
    }
    it = L.sched.emplace(nimg, std::move(S)).first;
  }
  *out = &it->second;
  return 0;
}

void free_schedule_for(TgLayer& L, int nimg) {
  auto it = L.sched.find(nimg);
  if (it == L.sched.end()) return;
  if (it->second.d_items) (void)hipFree(it->second.d_items);
  if (it->second.d_tiles) (void)hipFree(it->second.d_tiles);
  if (it->second.d_ttaps) (void)hipFree(it->second.d_ttaps);
  if (it->second.d_counters) (void)hipFree(it->second.d_counters);
  if (it->second.d_raw) (void)hipFree(it->second.d_raw);
  L.sched.erase(it);
}

void free_schedules(TgLayer& L) {
  for (auto& kv : L.sched) {
    if (kv.second.d_items) (void)hipFree(kv.second.d_items);
    if (kv.second.d_tiles) (void)hipFree(kv.second.d_tiles);
    if (kv.second.d_ttaps) (void)hipFree(kv.second.d_ttaps);
    if (kv.second.d_counters) (void)hipFree(kv.second.d_counters);
    if (kv.second.d_raw) (void)hipFree(kv.second.d_raw);
  }
  L.sched.clear();
}

}  // namespace
