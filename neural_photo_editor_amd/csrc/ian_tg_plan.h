// ian_tg_plan.h -- the planner of a tap-GEMM launch: tiles, per-tile tap lists, K ranges, split-K slabs, heavy-first + XCD-aware
// item order, and the launch model the tuner ranks split limits with.
// Plain C++: no HIP, no handle types (ian_rt_schedule.inc calls it; tests/tg_plan_main.cpp runs it on the CPU by brute force).
//
// Image-major plans (pos_major == 0) are the item lists this runtime has always built: every tile lists every tap of its class.
// Position-major plans (ian_tg_types.h) give a tile the taps that are inside the image for at least one of its valid rows: a tap
// that is outside for all of them contributes exact zeros (the gather reads zeros for such rows), so leaving it out changes no bit
// of an unsplit tile's result.  K ranges and split counts come per TILE from the tile's own K-steps, so that a border tile is one
// short item and not several, and the launch -- about one round of workgroups, as long as its longest item -- gets shorter.
#ifndef IAN_TG_PLAN_H
#define IAN_TG_PLAN_H

#include <algorithm>
#include <functional>
#include <map>
#include <queue>
#include <utility>
#include <vector>

#include "ian_tg_types.h"

namespace ian {

struct TgPlanIn {
  int nimg = 1;
  int QH = 1, QW = 1;                  // class grid (powers of two)
  int IH = 1, IW = 1, si = 1, by = 0, bx = 0, Cin = 32, Cout = 1;
  const TgClass* classes = nullptr;
  int ncls = 0;
  const TgTap* taps = nullptr;         // the layer's tap list, indexed by TgClass::tap0
  int ntaps_total = 0;
  int bm = 64, bn = 64;                // tile shape
  int pos_major = 0;
  int max_steps = -1;                  // TgChoice::max_steps: -1 = heuristic below, 0 = never split K, > 0 = no item longer than this
  int opt_split = 1, opt_no_split_items = 384, opt_target_items = 768, opt_min_steps = 16;   // the heuristic's options (Options, ian_rt_types.h)
  int xcd_group = 8, xcd_spatial = 0;
};

struct TgPlan {
  int M = 0;                  // rows of the launch (TgParams::M)
  int b_shift = -1;           // position-major: log2(Bp); -1 = image-major
  int tiles_m = 0, tiles_n = 0;
  bool split = false;
  int max_nsplit = 1;
  size_t slab_tiles = 0;
  long long steps = 0;        // K-steps the launch executes, summed over tiles
  long long steps_full = 0;   // ... and with every tile listing every tap of its class
  std::vector<TgItem> items;
  std::vector<TgTile> tiles;  // split plans: one entry per output tile, tile-major
  std::vector<TgTapE> taptab;
  std::vector<int> tile_ksteps;   // per output tile (class, row tile, column tile): its K-steps
};

static inline int tg_ceil_log2(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return s;
}

// rows of a launch and the row-order shift
static inline void tg_plan_rows(const TgPlanIn& in, int* M, int* b_shift) {
  *b_shift = in.pos_major ? tg_ceil_log2(in.nimg) : -1;
  *M = in.pos_major ? (in.QH * in.QW) << *b_shift : in.nimg * in.QH * in.QW;
}

// [class][row tile] -> the class-local indices of the taps the tile keeps, in class order.  Never empty: a tile none of whose
// valid rows sees any tap inside the image keeps the class's first tap, so that its epilogue still writes act(shift).
static inline void tg_tile_taps(const TgPlanIn& in, std::vector<std::vector<std::vector<int>>>& out) {
  int M, b_shift;
  tg_plan_rows(in, &M, &b_shift);
  const int tiles_m = (M + in.bm - 1) / in.bm;
  out.assign((size_t)in.ncls, std::vector<std::vector<int>>((size_t)tiles_m));
  for (int c = 0; c < in.ncls; ++c) {
    const TgClass& cl = in.classes[c];
    for (int mt = 0; mt < tiles_m; ++mt) {
      std::vector<int>& v = out[(size_t)c][(size_t)mt];
      if (b_shift < 0) {
        for (int t = 0; t < cl.ntaps; ++t) v.push_back(t);
        continue;
      }
      const int m0 = mt * in.bm, m1 = std::min(M, m0 + in.bm) - 1;
      for (int t = 0; t < cl.ntaps; ++t) {
        const TgTap& tp = in.taps[cl.tap0 + t];
        bool any = false;
        for (int pos = m0 >> b_shift; pos <= (m1 >> b_shift) && !any; ++pos) {
          const int first_n = std::max(m0, pos << b_shift) - (pos << b_shift);   // first image index of this position inside the tile
          if (first_n >= in.nimg) continue;                                     // padding rows only
          const int iy = (pos / in.QW) * in.si + in.by + tp.dy, ix = (pos % in.QW) * in.si + in.bx + tp.dx;
          any = iy >= 0 && iy < in.IH && ix >= 0 && ix < in.IW;
        }
        if (any) v.push_back(t);
      }
      if (v.empty() && cl.ntaps > 0) v.push_back(0);
    }
  }
}

// the K-steps of every output tile (class, row tile, column tile) of a plan, without choosing a split
static inline void tg_tile_ksteps(const TgPlanIn& in, std::vector<int>& ks, long long* steps_full = nullptr) {
  std::vector<std::vector<std::vector<int>>> lists;
  tg_tile_taps(in, lists);
  const int tiles_n = (in.Cout + in.bn - 1) / in.bn, kpt = in.Cin / 32;
  ks.clear();
  long long full = 0;
  for (int c = 0; c < in.ncls; ++c)
    for (auto& l : lists[(size_t)c])
      for (int nt = 0; nt < tiles_n; ++nt) {
        ks.push_back((int)l.size() * kpt);
        full += (long long)in.classes[c].ntaps * kpt;
      }
  if (steps_full) *steps_full = full;
}

// how a tile of `ks` K-steps is cut under the limit `ms` (0 = not at all): `per` K-steps per slice, the slice count returned
static inline int tg_slices(int ks, int ms, int* per) {
  int ns = ms > 0 ? std::max(1, (ks + ms - 1) / ms) : 1;
  *per = std::max(1, (ks + ns - 1) / ns);
  return std::max(1, (ks + *per - 1) / *per);
}

// The launch model: the items the scheduler builds from `tile_ks` under the limit `ms`, dealt longest-first onto `slots` machines;
// an item costs its K-steps + a fixed prologue / epilogue allowance.  Returns the makespan; *nitems the number of items.
static inline double tg_model_makespan(const std::vector<int>& tile_ks, int ms, int slots, long long* nitems = nullptr) {
  std::vector<int> lens;
  for (int ks : tile_ks) {
    int per;
    const int ns = tg_slices(ks, ms, &per);
    for (int k = 0; k < ns; ++k) lens.push_back(std::min(per, ks - k * per));
  }
  if (nitems) *nitems = (long long)lens.size();
  std::sort(lens.begin(), lens.end(), std::greater<int>());
  std::priority_queue<double, std::vector<double>, std::greater<double>> load;
  for (int k = 0; k < slots; ++k) load.push(0.0);
  double makespan = 0;
  for (int len : lens) {
    const double v = load.top() + len + 4.0;
    load.pop();
    load.push(v);
    makespan = std::max(makespan, v);
  }
  return makespan;
}

// Split limits worth timing for one tile shape, from the model instead of powers of two only: the `keep` limits in 8 .. max_ksteps
// with the shortest makespans (ties: fewer slabs; the same item list under another limit is listed once).
static inline std::vector<int> tg_model_split_limits(const std::vector<int>& tile_ks, int slots, int max_ksteps, int keep) {
  std::vector<std::pair<double, int>> scored;
  for (int ms = 8; ms < max_ksteps; ++ms) {
    long long nitems = 0;
    for (int ks : tile_ks) {
      int per;
      nitems += tg_slices(ks, ms, &per);
    }
    if (nitems > 8192) continue;
    const double makespan = tg_model_makespan(tile_ks, ms, slots);
    scored.push_back({makespan + 0.002 * (double)nitems / slots, ms});
  }
  std::sort(scored.begin(), scored.end());
  std::vector<int> out;
  double last = -1;
  for (auto& sc : scored) {
    if ((int)out.size() >= keep) break;
    if (sc.first == last) continue;
    last = sc.first;
    out.push_back(sc.second);
  }
  return out;
}

// the K-step limit per item of a plan: the forced one, or the heuristic's (aim at opt_target_items workgroups when the tiles alone
// give fewer than opt_no_split_items); 1 << 30 = no limit
static inline int tg_plan_step_limit(const TgPlanIn& in, long long total_steps, int total_tiles) {
  if (in.max_steps > 0) return in.max_steps;
  if (in.max_steps < 0 && in.opt_split && total_tiles < in.opt_no_split_items) {
    const long long spi = (total_steps + in.opt_target_items - 1) / in.opt_target_items;
    return (int)std::max<long long>(spi, in.opt_min_steps);
  }
  return 1 << 30;
}

static inline void tg_plan(const TgPlanIn& in, TgPlan& P) {
  tg_plan_rows(in, &P.M, &P.b_shift);
  const int tiles_m = (P.M + in.bm - 1) / in.bm, tiles_n = (in.Cout + in.bn - 1) / in.bn, kpt = in.Cin / 32, ncls = in.ncls;
  P.tiles_m = tiles_m; P.tiles_n = tiles_n;
  std::vector<std::vector<std::vector<int>>> lists;
  tg_tile_taps(in, lists);

  // ---- the tap table: identical lists stored once; an image-major plan's table is the layer's list, entry for entry
  P.taptab.clear();
  std::vector<std::vector<int>> list_off((size_t)ncls, std::vector<int>((size_t)tiles_m, 0));
  if (!in.pos_major) {
    P.taptab.resize((size_t)in.ntaps_total);
    for (int i = 0; i < in.ntaps_total; ++i) P.taptab[(size_t)i] = TgTapE{in.taps[i].dy, in.taps[i].dx, 0, 0};
    for (int c = 0; c < ncls; ++c) {
      for (int t = 0; t < in.classes[c].ntaps; ++t) P.taptab[(size_t)(in.classes[c].tap0 + t)].slab = t;
      for (int mt = 0; mt < tiles_m; ++mt) list_off[(size_t)c][(size_t)mt] = in.classes[c].tap0;
    }
  } else {
    std::map<std::pair<int, std::vector<int>>, int> seen;
    for (int c = 0; c < ncls; ++c)
      for (int mt = 0; mt < tiles_m; ++mt) {
        const std::vector<int>& l = lists[(size_t)c][(size_t)mt];
        auto key = std::make_pair(c, l);
        auto f = seen.find(key);
        if (f == seen.end()) {
          f = seen.emplace(key, (int)P.taptab.size()).first;
          for (int t : l) {
            const TgTap& tp = in.taps[in.classes[c].tap0 + t];
            P.taptab.push_back(TgTapE{tp.dy, tp.dx, t, 0});
          }
        }
        list_off[(size_t)c][(size_t)mt] = f->second;
      }
  }

  // ---- K-steps per tile, the limit, whether anything is split
  P.tile_ksteps.clear();
  P.steps = P.steps_full = 0;
  int max_ks = 0;
  for (int c = 0; c < ncls; ++c)
    for (int mt = 0; mt < tiles_m; ++mt) {
      const int ks = (int)lists[(size_t)c][(size_t)mt].size() * kpt;
      max_ks = std::max(max_ks, ks);
      for (int nt = 0; nt < tiles_n; ++nt) P.tile_ksteps.push_back(ks);
      P.steps += (long long)ks * tiles_n;
      P.steps_full += (long long)in.classes[c].ntaps * kpt * tiles_n;
    }
  const int steps_per_item = tg_plan_step_limit(in, P.steps, ncls * tiles_m * tiles_n);
  const bool split = max_ks > steps_per_item;
  P.split = split;

  struct Group {
    std::vector<TgItem> items;
    int weight;
  };
  std::vector<Group> groups;
  // supergroups of gm x gn tiles go to one XCD.  Position-major: one row tile per group -- its neighbours have other tap lists and
  // other K ranges, and heavy-first order needs groups of one weight
  const int gm = in.pos_major ? 1 : std::max(1, in.xcd_group), gn = std::max(1, in.xcd_group);
  P.tiles.clear();
  P.max_nsplit = 1;
  size_t slab_next = 0;
  for (int c = 0; c < ncls; ++c) {
    // slices per row tile; slab indices tile-major so that the reduce pass reads contiguous slabs
    std::vector<int> ns_mt((size_t)tiles_m), per_mt((size_t)tiles_m);
    std::vector<int> slab0((size_t)tiles_m * tiles_n, -1), tile_id((size_t)tiles_m * tiles_n, -1);
    int ns_max = 1;
    for (int mt = 0; mt < tiles_m; ++mt) {
      const int ks = (int)lists[(size_t)c][(size_t)mt].size() * kpt;
      ns_mt[(size_t)mt] = tg_slices(ks, split ? steps_per_item : 0, &per_mt[(size_t)mt]);
      ns_max = std::max(ns_max, ns_mt[(size_t)mt]);
      if (split) {
        P.max_nsplit = std::max(P.max_nsplit, ns_mt[(size_t)mt]);
        for (int nt = 0; nt < tiles_n; ++nt) {
          slab0[(size_t)mt * tiles_n + nt] = (int)slab_next;
          tile_id[(size_t)mt * tiles_n + nt] = (int)P.tiles.size();
          P.tiles.push_back(TgTile{c, mt * in.bm, nt * in.bn, (int)slab_next, ns_mt[(size_t)mt], in.classes[c].py, in.classes[c].px, 0});
          slab_next += (size_t)ns_mt[(size_t)mt];
        }
      }
    }
    for (int s = 0; s < ns_max; ++s)
      for (int nb = 0; nb < tiles_n; nb += gn)
        for (int mb = 0; mb < tiles_m; mb += gm) {
          Group g;
          g.weight = 0;
          for (int nt = nb; nt < std::min(tiles_n, nb + gn); ++nt)
            for (int mt = mb; mt < std::min(tiles_m, mb + gm); ++mt) {
              if (s >= ns_mt[(size_t)mt]) continue;
              const int ks = (int)lists[(size_t)c][(size_t)mt].size() * kpt, per = per_mt[(size_t)mt];
              const int k0 = s * per, k1 = std::min(ks, (s + 1) * per);
              g.weight = std::max(g.weight, k1 - k0);
              TgItem it{c, mt * in.bm, nt * in.bn, k0, k1, split ? slab0[(size_t)mt * tiles_n + nt] + s : -1, tile_id[(size_t)mt * tiles_n + nt], 0, 0, 0, 0, 0, 0, 0, 0};
              g.items.push_back(it);
            }
          if (!g.items.empty()) groups.push_back(std::move(g));
        }
  }
  std::stable_sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) { return a.weight > b.weight; });
  // deal supergroups to the 8 XCDs (block b runs on XCD b%8; observed, used for speed only): always to the least-loaded list.
  // Groups arrive heavy first; inside a run of EQUAL weight they are in (class, K-slice, N block, M block) order.
  // xcd_spatial (round-4 experiment, default OFF): cut such a run into 8 CONTIGUOUS pieces, one per XCD, so that spatial
  // neighbours share an L2.  Measured at batch 64 (profiles/r04_*): step time unchanged (1.5137 vs 1.5122 ms), HBM fetch per
  // tapgemm launch UP from 85 to 122 MB -- round-robin dealing of 8x8-tile supergroups already keeps a group's halo and weight
  // slab in one L2, and contiguous pieces put all K-slices / N blocks of a piece on one XCD at the same time, which evicts more.
  // The order of items changes, no item's K range or summation order does: results are bitwise the same either way.
  std::vector<std::vector<TgItem>> xl(8);
  std::vector<long long> load(8, 0);
  for (size_t g0 = 0; g0 < groups.size();) {
    size_t g1 = g0 + 1;
    while (g1 < groups.size() && groups[g1].weight == groups[g0].weight && groups[g1].items.size() == groups[g0].items.size()) ++g1;
    const size_t run = g1 - g0;
    if (in.xcd_spatial && run >= 8) {
      // XCDs ordered by current load: the least loaded one takes the first (possibly one-longer) piece
      int order[8] = {0, 1, 2, 3, 4, 5, 6, 7};
      std::stable_sort(order, order + 8, [&](int a, int b) { return load[(size_t)a] < load[(size_t)b]; });
      for (size_t k = 0; k < run; ++k) {
        const int x = order[(k * 8) / run];
        Group& g = groups[g0 + k];
        for (auto& it : g.items) xl[(size_t)x].push_back(it);
        load[(size_t)x] += (long long)g.weight * (long long)g.items.size();
      }
    } else {
      for (size_t k = g0; k < g1; ++k) {
        Group& g = groups[k];
        int best = 0;
        for (int x = 1; x < 8; ++x)
          if (load[(size_t)x] < load[(size_t)best]) best = x;
        for (auto& it : g.items) xl[(size_t)best].push_back(it);
        load[(size_t)best] += (long long)g.weight * (long long)g.items.size();
      }
    }
    g0 = g1;
  }
  size_t longest = 0;
  for (auto& l : xl) longest = std::max(longest, l.size());
  P.items.clear();
  const TgItem empty{0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t k = 0; k < longest; ++k)
    for (size_t x = 0; x < 8; ++x) P.items.push_back(k < xl[x].size() ? xl[x][k] : empty);
  while (!P.items.empty() && P.items.back().ks0 >= P.items.back().ks1) P.items.pop_back();
  for (auto& it : P.items) {   // the item carries its class, its tile's tap list and the first tap of its K range (TgItem)
    const TgClass& c = in.classes[it.cls];
    const int mt = it.m0 / in.bm;
    it.ntaps = (int)lists[(size_t)it.cls][(size_t)mt].size();
    it.tap0 = list_off[(size_t)it.cls][(size_t)mt];
    it.py = c.py; it.px = c.px; it.w_off = c.w_off;
    const TgTapE& t = P.taptab[(size_t)(it.tap0 + std::min(std::max(it.ntaps - 1, 0), it.ks0 / std::max(1, kpt)))];
    it.dy0 = t.dy; it.dx0 = t.dx; it.slab0 = t.slab;
  }
  P.slab_tiles = slab_next;
}

}  // namespace ian

#endif
