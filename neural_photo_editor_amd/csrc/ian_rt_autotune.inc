// ian_rt_autotune.inc -- autotuner and its cache.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
namespace {

// ----- autotuner: per (layer, batch) pick tile shape x split-K policy by timing the real launch ------------
// The 9/6/6/4-tap parity classes, the 4^2..64^2 spatial extents and batch sizes from 1 to 1024 make the best
// (tile, K-range) decomposition layer specific; candidates are timed with HIP events on the caller's stream.
struct TuneCand {
  TgChoice ch;
  float ms;
};

// Split limits worth timing for one tile shape come from a model instead of powers of two only (round 6; tg_model_split_limits,
// ian_tg_plan.h): for every limit 8 .. max the item list the planner would build -- from the real K-steps of every tile, which differ
// between tiles once a position-major plan skips taps -- is dealt longest-first onto tg_slots machines, and the limits with the
// shortest makespans are timed.  conv4 at batch 64 is the case that motivated it: 64 tiles x 400 K-steps fill the 512 slots of the
// 8-wave 128x128 tile exactly with limit 50 -- 64 gives 448 items, 32 gives 832 (1.6 rounds) -- and the tuner never saw 50.
std::vector<TgChoice> tune_candidates(const ian_handle* h, const TgLayer& L, int nimg) {
  const int M = nimg * L.QH * L.QW;
  std::vector<int> cfgs;
  if (L.Cout <= 32) cfgs = {TG_128x32};
  else if (M <= 32) cfgs = {TG_32x128, TG_64x64};
  else if (M <= 64) cfgs = {TG_64x64, TG_32x128, TG_128x64};
  else {
    cfgs = {TG_128x128, TG_128x64, TG_64x64};
    if (bf16x3_applies(h, M, nimg)) {   // the split-bf16 kernel: its own tiles only, one K-loop schedule
      if (M >= 512 && L.Cout >= 128) cfgs.push_back(TG_128x128W8);
    } else
    if (M >= 512 && L.Cout >= 128) cfgs.push_back(TG_256x128);
    if (!(bf16x3_applies(h, M, nimg))) {
      if (M >= 512 && L.Cout >= 128) cfgs.push_back(TG_128x128W8);
      if (M >= 512 && L.Cout >= 64) cfgs.push_back(TG_128x64W8);
    }
  }
  int max_ksteps = 0;
  for (auto& c : L.classes) max_ksteps = std::max(max_ksteps, c.ntaps * (L.Cin / 32));
  const bool pm_allowed = pos_major_allowed(h, L, nimg);
  std::vector<TgChoice> out;
  for (int cfg : cfgs) {
    const TgShape sh = tg_shape(cfg);
    // image-major rows, then -- where the option admits it and the planner's list is shorter than the full one -- position-major rows
    for (int pm = 0; pm < (pm_allowed && !(bf16x3_applies(h, M, nimg) && tg_bf16x3_supported(cfg)) ? 2 : 1); ++pm) {
    std::vector<int> tile_ks;
    long long steps_full = 0, steps = 0;
    tg_tile_ksteps(plan_input(h, L, nimg, cfg, 0, pm), tile_ks, &steps_full);
    for (int k : tile_ks) steps += k;
    if (pm && (steps >= steps_full || h->opt.tg_pos_major == 2)) continue;   // nothing to skip; forced mode: the first pass is position-major already
    const long long tiles = (long long)tile_ks.size() / (long long)L.classes.size();   // per class
    std::vector<int> limits = {0, 4, 8, 16, 32, 64, 128, 256};
    if (h->opt.tg_tune_model && M > 64 && tiles * (long long)L.classes.size() < 2ll * tg_slots(cfg))   // enough tiles: nothing to split
      for (int ms : tg_model_split_limits(tile_ks, tg_slots(cfg), max_ksteps, 3))
        if (std::find(limits.begin(), limits.end(), ms) == limits.end()) limits.push_back(ms);
    for (int ms : limits) {
      if (ms > 0 && ms >= max_ksteps) continue;  // would not split anything
      if (ms > 0) {
        long long slabs = 0;
        for (int k : tile_ks) slabs += (k + ms - 1) / ms;
        if (slabs * sh.bm * sh.bn * 4 > (512ll << 20)) continue;  // slab workspace cap
        if (slabs > 16384) continue;
      }
      // how a split schedule's partials are combined: small launches (the batch-1 chains) may fold the combine into the tapgemm
      // launch (kernels_tapgemm.hip, fused 1 / 2) instead of paying a reduce launch that costs as much as their K loop
      const int nfuse = (ms > 0 && M <= h->opt.tg_fuse_max_m && tg_fuse_supported(cfg)) ? 1 + h->opt.tg_fuse_tune : 1;
      for (int fu = 0; fu < nfuse; ++fu)
        for (int var : {TG_SCHED_SPLIT, TG_SCHED_ROTATED, TG_SCHED_QUEUE3, TG_SCHED_ROTATED_PIN, TG_SCHED_AHEAD2, TG_SCHED_AHEAD3}) {   // DMA staging measured 5 % slower on every 5x5 layer: selectable, not a candidate
          if (!tg_schedule_valid(var)) continue;   // AHEAD3: libian_ablation.so only
          if (var != TG_SCHED_SPLIT && bf16x3_applies(h, M, nimg) && tg_bf16x3_supported(cfg)) continue;   // one schedule there
          if (var == TG_SCHED_ROTATED_PIN && !h->opt.tg_tune_pin) continue;   // A/B switch: the pinned form of schedule 2 as a candidate (round 6)
          if (var == TG_SCHED_QUEUE3 && (M > 1024 || cfg == TG_256x128)) continue;
          if (var == TG_SCHED_AHEAD3 && (h->opt.tg_tune_deep < 2 || tg_shape(cfg).bm * tg_shape(cfg).bn > 128 * 64)) continue;   // three K-steps in flight: the small tiles
          if (var == TG_SCHED_AHEAD2 && (!h->opt.tg_tune_deep || cfg == TG_256x128)) continue;   // two K-steps of loads in flight in the rotated schedule (round 6)   // the three-deep load queue is for latency-bound items (few images)
          TgChoice c;
          c.cfg = cfg;
          c.max_steps = ms;
          c.variant = var;
          c.fused = fu;
          c.pos_major = pm_allowed ? pm : -1;
          out.push_back(c);
        }
    }
    }
  }
  return out;
}

template <typename F>
int time_launches(ian_handle* h, hipStream_t st, int reps, F&& fn, float* ms) {
  hipEvent_t a, b;
  HIPCHK(h, hipEventCreate(&a));
  HIPCHK(h, hipEventCreate(&b));
  int rc = fn();  // warm-up (also builds + uploads the schedule)
  if (!rc) {
    (void)hipEventRecord(a, st);
    for (int r = 0; r < reps && !rc; ++r) rc = fn();
    (void)hipEventRecord(b, st);
    (void)hipEventSynchronize(b);
    float t = 0;
    (void)hipEventElapsedTime(&t, a, b);
    *ms = t / reps;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return rc;
}

template <typename F>
int tune_layer(ian_handle* h, TgLayer& L, int nimg, hipStream_t st, F&& run, TgChoice* best_out, float* best_ms) {
  TgChoice best;
  float bms = 1e30f;
  // IAN_TUNE_LOG=<file>: every candidate's time, appended as "<M> <Cin> <Cout> <classes> <cfg> <max_steps> <variant> <fused> <pos_major> <us>" (a measurement
  // aid: which tile / split / schedule loses by how much on which layer; the choice itself is unaffected)
  const char* logp = getenv("IAN_TUNE_LOG");
  FILE* logf = logp ? fopen(logp, "a") : nullptr;
  std::vector<TuneCand> timed;
  for (const TgChoice& c : tune_candidates(h, L, nimg)) {
    L.choice[nimg] = c;
    free_schedule_for(L, nimg);
    float ms = 0;
    int rc = time_launches(h, st, 5, run, &ms);
    if (logf) fprintf(logf, "%d %d %d %d %d %d %d %d %d %.2f%s\n", nimg * L.QH * L.QW, L.Cin, L.Cout, (int)L.classes.size(), c.cfg, c.max_steps, c.variant, c.fused, c.pos_major, ms * 1000.f, rc ? " FAILED" : "");
    if (rc) { if (logf) fclose(logf); return rc; }
    timed.push_back({c, ms});
    if (ms < bms) {
      bms = ms;
      best = c;
    }
  }
  // second pass: five launches separate candidates that are 1-2 % apart only by luck (the same candidate moves by +-2 % between
  // runs on one box, and the box drifts while the candidates are walked) -- the N fastest are timed again in three interleaved
  // rounds of 12 launches each and the candidate with the best round wins
  if (h->opt.tg_tune_final > 0 && timed.size() > 1) {
    std::stable_sort(timed.begin(), timed.end(), [](const TuneCand& a, const TuneCand& b) { return a.ms < b.ms; });
    const size_t nf = std::min<size_t>(timed.size(), (size_t)h->opt.tg_tune_final);
    std::vector<float> best_round(nf, 1e30f);
    for (int round = 0; round < 3; ++round)
      for (size_t k = 0; k < nf; ++k) {
        L.choice[nimg] = timed[k].ch;
        free_schedule_for(L, nimg);
        float ms = 0;
        int rc = time_launches(h, st, 12, run, &ms);
        if (rc) { if (logf) fclose(logf); return rc; }
        best_round[k] = std::min(best_round[k], ms);
      }
    bms = 1e30f;
    for (size_t k = 0; k < nf; ++k) {
      if (logf) fprintf(logf, "%d %d %d %d %d %d %d %d %d %.2f final\n", nimg * L.QH * L.QW, L.Cin, L.Cout, (int)L.classes.size(), timed[k].ch.cfg, timed[k].ch.max_steps, timed[k].ch.variant, timed[k].ch.fused, timed[k].ch.pos_major, best_round[k] * 1000.f);
      if (best_round[k] < bms) {
        bms = best_round[k];
        best = timed[k].ch;
      }
    }
  }
  if (logf) fclose(logf);
  L.choice[nimg] = best;
  free_schedule_for(L, nimg);
  if (best_out) *best_out = best;
  if (best_ms) *best_ms = bms;
  return 0;
}

// ----- autotune cache: IAN_TUNE_CACHE=<file> makes ian_autotune reuse / record its per-(batch, direction, layer)
// choices, so that repeated processes (e.g. the rocprofv3 passes of one profile) run the very same kernels.
typedef std::map<std::string, TgChoice> TuneCache;
std::string tune_key(int n, const char* dir, const std::string& name) { return std::to_string(n) + " " + dir + " " + name; }
// File format: first line "ian-tune-cache <format version>", then "<batch> <dir> <layer> <cfg> <max_steps> <variant> <fused> <pos_major>" per line (format 3 added the row order).  A
// file without that header (an older 6-field format would shift every later field by one) or with another version is IGNORED, and
// every field is range-checked: a stale or corrupt cache must never reach a kernel as an out-of-range schedule (ADVICE r5).
constexpr int TUNE_CACHE_FORMAT = 3;
void tune_cache_load(TuneCache& c) {
  const char* path = getenv("IAN_TUNE_CACHE");
  if (!path) return;
  FILE* f = fopen(path, "r");
  if (!f) return;
  char magic[32];
  int ver = 0;
  if (fscanf(f, "%31s %d", magic, &ver) != 2 || strcmp(magic, "ian-tune-cache") != 0 || ver != TUNE_CACHE_FORMAT) {
    fclose(f);
    return;
  }
  char dir[16], name[256];
  int n, cfg, ms, var, fu, pm;
  while (fscanf(f, "%d %15s %255s %d %d %d %d %d", &n, dir, name, &cfg, &ms, &var, &fu, &pm) == 8) {
    if (n <= 0 || cfg < 0 || cfg >= TG_NCONFIG || ms < 0 || fu < 0 || fu > 2 || pm < -1 || pm > 1 || !tg_schedule_shipped(var)) continue;
    TgChoice ch;
    ch.cfg = cfg;
    ch.max_steps = ms;
    ch.variant = var;
    ch.fused = fu;
    ch.pos_major = pm;
    c[tune_key(n, dir, name)] = ch;
  }
  fclose(f);
}
void tune_cache_store(const TuneCache& c) {
  const char* path = getenv("IAN_TUNE_CACHE");
  if (!path) return;
  FILE* f = fopen(path, "w");
  if (!f) return;
  fprintf(f, "ian-tune-cache %d\n", TUNE_CACHE_FORMAT);
  for (auto& kv : c) fprintf(f, "%s %d %d %d %d %d\n", kv.first.c_str(), kv.second.cfg, kv.second.max_steps, kv.second.variant, kv.second.fused, kv.second.pos_major);
  fclose(f);
}

// stage a caller buffer (host or device) into a device pointer; returns pointer to use

}  // namespace
