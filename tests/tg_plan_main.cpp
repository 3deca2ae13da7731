// Stand-alone CPU driver of csrc/ian_tg_plan.h (tests/test_tg_plan_host.py builds it under AddressSanitizer + UBSan).
//   tg_plan_main <geometry> [tile]   plans the geometry for every tile shape (or the one given, 0 .. 7) x batch x Cin x split limit x row
//                               order and checks every plan by brute force over (valid row, tap); prints "ok <plans> <taps skipped> <one-position tiles> <kept-tap tiles>
//                               <unsplit border tiles>"
//   tg_plan_main model          prints the model's makespan ratio position-major / image-major for the batch-64 5x5 layers
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ian_tg_plan.h"

using namespace ian;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n  [%s]\n", g_ctx.c_str());        \
      exit(1);                                             \
    }                                                      \
  } while (0)

static std::string g_ctx;

struct Geo {
  int QH, QW, IH, IW, si, by, bx;
  std::vector<TgClass> classes;
  std::vector<TgTap> taps;
};

static void add_class(Geo& G, int py, int px, const std::vector<TgTap>& taps, long long w_off) {
  TgClass c;
  c.ntaps = (int)taps.size(); c.tap0 = (int)G.taps.size(); c.py = py; c.px = px; c.w_off = w_off;
  G.classes.push_back(c);
  for (auto& t : taps) G.taps.push_back(t);
}
static Geo conv5s2(int in) {   // 5x5 stride-2 convolution, in x in -> in/2 x in/2
  Geo G{in / 2, in / 2, in, in, 2, -2, -2, {}, {}};
  std::vector<TgTap> taps;
  for (int ky = 0; ky < 5; ++ky)
    for (int kx = 0; kx < 5; ++kx) taps.push_back({ky, kx});
  add_class(G, 0, 0, taps, 0);
  return G;
}
static Geo deconv5s2(int in) {   // transposed 5x5 stride-2, in x in -> 2 in x 2 in: four output-parity classes of 9 / 6 / 6 / 4 taps
  Geo G{in, in, in, in, 1, 0, 0, {}, {}};
  long long t_global = 0;
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px) {
      std::vector<TgTap> taps;
      for (int ky = py; ky < 5; ky += 2)
        for (int kx = px; kx < 5; kx += 2) taps.push_back({(py + 2 - ky) / 2, (px + 2 - kx) / 2});
      add_class(G, py, px, taps, t_global * 1000);
      t_global += (long long)taps.size();
    }
  return G;
}
// composite 3x3 stencil with dilations 1, 2, 4, 8: the centre and eight taps per dilation; ring_only: the eight taps of dilation 8 alone,
// which a 4x4 map never reaches -- every tile's list would be empty
static Geo dilated3(int in, bool ring_only = false) {
  Geo G{in, in, in, in, 1, 0, 0, {}, {}};
  std::vector<TgTap> taps;
  if (!ring_only) taps.push_back({0, 0});
  for (int d : {1, 2, 4, 8})
    if (!ring_only || d == 8)
    for (int p = -1; p <= 1; ++p)
      for (int q = -1; q <= 1; ++q)
        if (p || q) taps.push_back({p * d, q * d});
  add_class(G, 0, 0, taps, 0);
  return G;
}

static TgPlanIn plan_in(const Geo& G, int nimg, int Cin, int Cout, int bm, int bn, int pos_major, int limit) {
  TgPlanIn in;
  in.nimg = nimg; in.QH = G.QH; in.QW = G.QW; in.IH = G.IH; in.IW = G.IW; in.si = G.si; in.by = G.by; in.bx = G.bx;
  in.Cin = Cin; in.Cout = Cout; in.classes = G.classes.data(); in.ncls = (int)G.classes.size(); in.taps = G.taps.data();
  in.ntaps_total = (int)G.taps.size(); in.bm = bm; in.bn = bn; in.pos_major = pos_major; in.max_steps = limit;
  return in;
}

// ---- the item list as the runtime built it before the planner existed (image-major, every tile lists its class's taps) --------
struct OldItem { int cls, m0, n0, ks0, ks1, slab, tile, ntaps, tap0, py, px, dy0, dx0; long long w_off; };
static void old_schedule(const Geo& G, int nimg, int Cin, int Cout, int bm, int bn, int limit, std::vector<OldItem>& out, std::vector<TgTile>& tiles,
                         size_t* slab_tiles, int* max_nsplit, bool* split_out) {
  const int M = nimg * G.QH * G.QW, tiles_m = (M + bm - 1) / bm, tiles_n = (Cout + bn - 1) / bn, kpt = Cin / 32, ncls = (int)G.classes.size();
  int steps_per_item = limit > 0 ? limit : 1 << 30;
  bool split = false;
  for (auto& c : G.classes)
    if (c.ntaps * kpt > steps_per_item) split = true;
  struct Group { std::vector<OldItem> items; int weight; };
  std::vector<Group> groups;
  const int gm = 8, gn = 8;
  tiles.clear();
  *max_nsplit = 1;
  size_t slab_next = 0;
  for (int c = 0; c < ncls; ++c) {
    const int ksteps = G.classes[c].ntaps * kpt;
    int ns = 1;
    if (split) ns = std::max(1, (ksteps + steps_per_item - 1) / steps_per_item);
    const int per = (ksteps + ns - 1) / ns;
    ns = (ksteps + per - 1) / per;
    if (split) *max_nsplit = std::max(*max_nsplit, ns);
    std::vector<int> slab0((size_t)tiles_m * tiles_n, -1), tile_id((size_t)tiles_m * tiles_n, -1);
    if (split)
      for (int mt = 0; mt < tiles_m; ++mt)
        for (int nt = 0; nt < tiles_n; ++nt) {
          slab0[(size_t)mt * tiles_n + nt] = (int)slab_next;
          tile_id[(size_t)mt * tiles_n + nt] = (int)tiles.size();
          tiles.push_back(TgTile{c, mt * bm, nt * bn, (int)slab_next, ns, G.classes[c].py, G.classes[c].px, 0});
          slab_next += ns;
        }
    for (int s = 0; s < ns; ++s) {
      const int k0 = s * per, k1 = std::min(ksteps, (s + 1) * per);
      for (int nb = 0; nb < tiles_n; nb += gn)
        for (int mb = 0; mb < tiles_m; mb += gm) {
          Group g;
          g.weight = k1 - k0;
          for (int nt = nb; nt < std::min(tiles_n, nb + gn); ++nt)
            for (int mt = mb; mt < std::min(tiles_m, mb + gm); ++mt)
              g.items.push_back(OldItem{c, mt * bm, nt * bn, k0, k1, split ? slab0[(size_t)mt * tiles_n + nt] + s : -1, tile_id[(size_t)mt * tiles_n + nt], 0, 0, 0, 0, 0, 0, 0});
          groups.push_back(std::move(g));
        }
    }
  }
  std::stable_sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) { return a.weight > b.weight; });
  std::vector<std::vector<OldItem>> lists(8);
  std::vector<long long> load(8, 0);
  for (auto& g : groups) {
    int best = 0;
    for (int x = 1; x < 8; ++x)
      if (load[x] < load[best]) best = x;
    for (auto& it : g.items) lists[best].push_back(it);
    load[best] += (long long)g.weight * (long long)g.items.size();
  }
  size_t longest = 0;
  for (auto& l : lists) longest = std::max(longest, l.size());
  out.clear();
  const OldItem empty{0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t k = 0; k < longest; ++k)
    for (int x = 0; x < 8; ++x) out.push_back(k < lists[x].size() ? lists[x][k] : empty);
  while (!out.empty() && out.back().ks0 >= out.back().ks1) out.pop_back();
  for (auto& it : out) {
    const TgClass& c = G.classes[it.cls];
    it.ntaps = c.ntaps; it.tap0 = c.tap0; it.py = c.py; it.px = c.px; it.w_off = c.w_off;
    const TgTap& t = G.taps[c.tap0 + std::min(std::max(c.ntaps - 1, 0), it.ks0 / std::max(1, kpt))];
    it.dy0 = t.dy; it.dx0 = t.dx;
  }
  *slab_tiles = slab_next;
  *split_out = split;
}

struct Counts { long long plans = 0, skipped = 0, one_pos = 0, kept = 0, border_unsplit = 0; };

static void check_plan(const Geo& G, const TgPlanIn& in, const TgPlan& P, Counts& cnt) {
  const int QHW = G.QH * G.QW, kpt = in.Cin / 32, ncls = in.ncls;
  const int Bp = in.pos_major ? 1 << P.b_shift : 0;
  if (in.pos_major) {
    CHECK(P.b_shift >= 0 && Bp >= in.nimg && (Bp >> 1) < in.nimg, "Bp %d for %d images", Bp, in.nimg);
    CHECK(P.M == QHW * Bp, "M %d", P.M);
  } else {
    CHECK(P.b_shift == -1 && P.M == in.nimg * QHW, "M %d b_shift %d", P.M, P.b_shift);
  }
  const int tiles_m = (P.M + in.bm - 1) / in.bm, tiles_n = (in.Cout + in.bn - 1) / in.bn;
  CHECK(P.tiles_m == tiles_m && P.tiles_n == tiles_n, "tile counts");
  // per (class, position): which class taps read inside the image
  std::vector<std::vector<uint64_t>> inimg((size_t)ncls, std::vector<uint64_t>((size_t)QHW, 0));
  for (int c = 0; c < ncls; ++c) {
    CHECK(G.classes[c].ntaps <= 64, "the masks below hold 64 taps");
    for (int pos = 0; pos < QHW; ++pos)
      for (int t = 0; t < G.classes[c].ntaps; ++t) {
        const TgTap& tp = G.taps[G.classes[c].tap0 + t];
        const int iy = (pos / G.QW) * G.si + G.by + tp.dy, ix = (pos % G.QW) * G.si + G.bx + tp.dx;
        if (iy >= 0 && iy < G.IH && ix >= 0 && ix < G.IW) inimg[c][pos] |= 1ull << t;
      }
  }
  // ---- items: per output tile its tap list and the coverage of its K-steps
  struct TileRec { int tap0 = -1, ntaps = 0; std::vector<int> cover; std::vector<const TgItem*> items; };
  std::vector<TileRec> recs((size_t)ncls * tiles_m * tiles_n);   // tile-major: (class, row tile, column tile)
  std::vector<char> slab_used(P.slab_tiles, 0);
  size_t slabs = 0, tiles_seen = 0;
  for (const TgItem& it : P.items) {
    if (it.ks0 >= it.ks1) continue;   // padding item: the kernel returns at once
    CHECK(it.cls >= 0 && it.cls < ncls && it.m0 % in.bm == 0 && it.n0 % in.bn == 0 && it.m0 < P.M && it.n0 < in.Cout && it.m0 >= 0 && it.n0 >= 0, "item tile");
    const TgClass& cl = G.classes[it.cls];
    CHECK(it.py == cl.py && it.px == cl.px && it.w_off == cl.w_off, "item class copy");
    CHECK(it.ntaps >= 1 && it.tap0 >= 0 && it.tap0 + it.ntaps <= (int)P.taptab.size(), "item tap list [%d, +%d) of %zu", it.tap0, it.ntaps, P.taptab.size());
    CHECK(it.ks0 >= 0 && it.ks1 <= it.ntaps * kpt, "K range [%d, %d) of %d", it.ks0, it.ks1, it.ntaps * kpt);
    if (in.max_steps > 0) CHECK(it.ks1 - it.ks0 <= in.max_steps, "item of %d K-steps over the limit %d", it.ks1 - it.ks0, in.max_steps);
    const TgTapE& first = P.taptab[(size_t)(it.tap0 + std::min(it.ntaps - 1, it.ks0 / kpt))];
    CHECK(it.dy0 == first.dy && it.dx0 == first.dx && it.slab0 == first.slab, "first tap of the item");
    TileRec& r = recs[((size_t)it.cls * tiles_m + it.m0 / in.bm) * tiles_n + it.n0 / in.bn];
    if (r.tap0 < 0) { ++tiles_seen; r.tap0 = it.tap0; r.ntaps = it.ntaps; r.cover.assign((size_t)(it.ntaps * kpt), 0); }
    CHECK(r.tap0 == it.tap0 && r.ntaps == it.ntaps, "items of one tile disagree on its tap list");
    for (int k = it.ks0; k < it.ks1; ++k) ++r.cover[(size_t)k];
    r.items.push_back(&it);
    if (P.split) {
      CHECK(it.slab >= 0 && (size_t)it.slab < P.slab_tiles && !slab_used[(size_t)it.slab], "slab %d not unique / out of range", it.slab);
      slab_used[(size_t)it.slab] = 1;
      ++slabs;
      CHECK(it.tile >= 0 && it.tile < (int)P.tiles.size(), "tile index");
    } else {
      CHECK(it.slab == -1, "unsplit plan with a slab");
    }
  }
  CHECK(P.split || (P.tiles.empty() && P.slab_tiles == 0), "unsplit plan with a tile table");
  if (P.split) CHECK(slabs == P.slab_tiles, "%zu slabs used of %zu", slabs, P.slab_tiles);
  long long steps = 0;
  int max_ns = 1;
  size_t tile_index = 0;
  for (int c = 0; c < ncls; ++c)
    for (int mt = 0; mt < tiles_m; ++mt) {
      // the taps the tile's valid rows read inside the image, by brute force over its rows
      uint64_t want = 0;
      int npos = 0, last_pos = -1;   // distinct positions among the valid rows (position-major rows ascend in position)
      bool any_valid = false;
      for (int m = mt * in.bm; m < std::min(P.M, (mt + 1) * in.bm); ++m) {
        const int n = in.pos_major ? (m & (Bp - 1)) : m / QHW, pos = in.pos_major ? (m >> P.b_shift) : m % QHW;
        if (n >= in.nimg) continue;
        any_valid = true;
        if (pos != last_pos) { ++npos; last_pos = pos; }
        want |= inimg[c][pos];
      }
      if (!in.pos_major) want = G.classes[c].ntaps == 64 ? ~0ull : (1ull << G.classes[c].ntaps) - 1;   // image-major: every tap, as always
      if (npos == 1 && in.pos_major) ++cnt.one_pos;
      for (int nt = 0; nt < tiles_n; ++nt, ++tile_index) {
        const TileRec& r = recs[tile_index];
        CHECK(r.tap0 >= 0, "tile (%d, %d, %d)%s has no item", c, mt, nt, any_valid ? " with valid rows" : "");
        uint64_t got = 0;
        int prev = -1;
        for (int e = 0; e < r.ntaps; ++e) {
          const TgTapE& te = P.taptab[(size_t)(r.tap0 + e)];
          CHECK(te.slab > prev && te.slab < G.classes[c].ntaps, "tap list not in class order");
          prev = te.slab;
          const TgTap& tp = G.taps[G.classes[c].tap0 + te.slab];
          CHECK(te.dy == tp.dy && te.dx == tp.dx, "tap entry (%d, %d) is not class tap %d", te.dy, te.dx, te.slab);
          got |= 1ull << te.slab;
        }
        if (want == 0) {
          CHECK(r.ntaps == 1, "a tile with nothing inside the image keeps exactly one tap, not %d", r.ntaps);
          if (nt == 0) ++cnt.kept;
        } else {
          CHECK(got == want, "tile (%d, %d, %d): taps %llx listed, %llx inside the image for a valid row", c, mt, nt, (unsigned long long)got, (unsigned long long)want);
        }
        if (nt == 0) cnt.skipped += G.classes[c].ntaps - r.ntaps;
        for (size_t k = 0; k < r.cover.size(); ++k) CHECK(r.cover[k] == 1, "tile (%d, %d, %d): K-step %zu covered %d times", c, mt, nt, k, r.cover[k]);
        CHECK(tile_index < P.tile_ksteps.size() && P.tile_ksteps[tile_index] == r.ntaps * kpt, "tile_ksteps");
        steps += r.ntaps * kpt;
        if (in.max_steps > 0 && r.ntaps * kpt <= in.max_steps) {
          CHECK(r.items.size() == 1, "a tile of %d K-steps under the limit %d is cut into %zu", r.ntaps * kpt, in.max_steps, r.items.size());
          if (r.ntaps < G.classes[c].ntaps && G.classes[c].ntaps * kpt > in.max_steps && nt == 0) ++cnt.border_unsplit;
        }
        if (in.max_steps == 0) CHECK(r.items.size() == 1, "split without a limit");
        if (P.split) {
          const TgTile& tl = P.tiles[(size_t)r.items[0]->tile];
          CHECK(tl.cls == c && tl.m0 == mt * in.bm && tl.n0 == nt * in.bn && tl.py == G.classes[c].py && tl.px == G.classes[c].px, "tile table entry");
          CHECK(tl.nsplit == (int)r.items.size(), "tile of %zu items with nsplit %d", r.items.size(), tl.nsplit);
          CHECK(r.items[0]->tile == (int)tile_index, "the tile table is tile-major");
          max_ns = std::max(max_ns, tl.nsplit);
          std::vector<const TgItem*> by_k = r.items;
          std::sort(by_k.begin(), by_k.end(), [](const TgItem* a, const TgItem* b) { return a->ks0 < b->ks0; });
          for (size_t s = 0; s < by_k.size(); ++s) CHECK(by_k[s]->tile == r.items[0]->tile && by_k[s]->slab == tl.slab0 + (int)s, "slabs of a tile in slice order");
        }
      }
    }
  CHECK(tiles_seen == recs.size(), "tiles without items");
  CHECK(steps == P.steps && P.steps <= P.steps_full, "step counts %lld %lld %lld", steps, P.steps, P.steps_full);
  if (P.split) CHECK(max_ns == P.max_nsplit && P.tiles.size() == recs.size(), "max_nsplit / tile table size");
  if (!in.pos_major) CHECK(P.steps == P.steps_full, "image-major plans skip nothing");
  ++cnt.plans;
}

static void check_against_old(const Geo& G, const TgPlanIn& in, const TgPlan& P) {
  std::vector<OldItem> old;
  std::vector<TgTile> tiles;
  size_t slab_tiles;
  int max_nsplit;
  bool split;
  old_schedule(G, in.nimg, in.Cin, in.Cout, in.bm, in.bn, in.max_steps, old, tiles, &slab_tiles, &max_nsplit, &split);
  CHECK(old.size() == P.items.size() && split == P.split && slab_tiles == P.slab_tiles && max_nsplit == P.max_nsplit, "item list sizes %zu %zu", old.size(), P.items.size());
  for (size_t k = 0; k < old.size(); ++k) {
    const OldItem& a = old[k];
    const TgItem& b = P.items[k];
    CHECK(a.cls == b.cls && a.m0 == b.m0 && a.n0 == b.n0 && a.ks0 == b.ks0 && a.ks1 == b.ks1 && a.slab == b.slab && a.tile == b.tile && a.ntaps == b.ntaps &&
          a.tap0 == b.tap0 && a.py == b.py && a.px == b.px && a.dy0 == b.dy0 && a.dx0 == b.dx0 && a.w_off == b.w_off, "item %zu differs from the image-major list", k);
    CHECK(b.slab0 == std::min(b.ntaps - 1, b.ks0 / (in.Cin / 32)), "a full list's slab is the tap index");
  }
  CHECK(tiles.size() == (split ? P.tiles.size() : 0), "tile table");
  if (split)
    for (size_t k = 0; k < tiles.size(); ++k) CHECK(memcmp(&tiles[k], &P.tiles[k], sizeof(TgTile)) == 0, "tile %zu", k);
  CHECK(P.taptab.size() == G.taps.size(), "the image-major tap table is the layer's list");
  for (size_t k = 0; k < G.taps.size(); ++k) CHECK(P.taptab[k].dy == G.taps[k].dy && P.taptab[k].dx == G.taps[k].dx, "tap %zu", k);
}

static const int TILES[8][2] = {{128, 128}, {128, 64}, {64, 64}, {32, 128}, {256, 128}, {128, 32}, {128, 128}, {128, 64}};   // enum TgConfig, ian_internal.h

static int run_geometry(const char* name, int only_cfg) {
  Geo G;
  if (!strcmp(name, "conv8")) G = conv5s2(8);
  else if (!strcmp(name, "conv16")) G = conv5s2(16);
  else if (!strcmp(name, "conv64")) G = conv5s2(64);
  else if (!strcmp(name, "deconv4")) G = deconv5s2(4);
  else if (!strcmp(name, "deconv16")) G = deconv5s2(16);
  else if (!strcmp(name, "dil4")) G = dilated3(4);
  else if (!strcmp(name, "dil16")) G = dilated3(16);
  else if (!strcmp(name, "ring4")) G = dilated3(4, true);
  else return 2;
  Counts cnt;
  for (int cfg = 0; cfg < 8; ++cfg) {
    if (only_cfg >= 0 && cfg != only_cfg) continue;
    for (int nimg : {1, 5, 24, 32, 64, 256})
      for (int Cin : {32, 64, 512})
        for (int limit : {0, 8, 50})
          for (int pm = 0; pm < 2; ++pm) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s tile %dx%d images %d Cin %d limit %d %s", name, TILES[cfg][0], TILES[cfg][1], nimg, Cin, limit, pm ? "position-major" : "image-major");
            g_ctx = buf;
            const TgPlanIn in = plan_in(G, nimg, Cin, 96, TILES[cfg][0], TILES[cfg][1], pm, limit);
            TgPlan P;
            tg_plan(in, P);
            check_plan(G, in, P, cnt);
            if (!pm) check_against_old(G, in, P);
            std::vector<int> ks;
            long long full = 0;
            tg_tile_ksteps(in, ks, &full);
            CHECK(ks == P.tile_ksteps && full == P.steps_full, "tg_tile_ksteps disagrees with the plan");
          }
  }
  printf("ok %lld %lld %lld %lld %lld\n", cnt.plans, cnt.skipped, cnt.one_pos, cnt.kept, cnt.border_unsplit);
  return 0;
}

// the launch model on the batch-64 5x5 layers of IAN_simple: makespan of the best position-major limit / the best image-major one
static int run_model() {
  struct Layer { const char* name; Geo G; int Cin, Cout; };
  const Layer layers[] = {{"enc_conv2", conv5s2(32), 128, 256}, {"enc_conv3", conv5s2(16), 256, 512}, {"enc_conv4", conv5s2(8), 512, 1024},
                          {"dec_conv1", deconv5s2(4), 1024, 512}, {"dec_conv2", deconv5s2(8), 512, 256}, {"dec_conv3", deconv5s2(16), 256, 128}};
  const int shapes[3][3] = {{64, 64, 1024}, {128, 64, 512}, {128, 128, 512}};   // tile, workgroup slots (tg_slots, ian_rt_autotune.inc)
  for (const Layer& L : layers)
    for (auto& sh : shapes) {
      double best[2] = {1e30, 1e30};
      for (int pm = 0; pm < 2; ++pm) {
        std::vector<int> ks;
        tg_tile_ksteps(plan_in(L.G, 64, L.Cin, L.Cout, sh[0], sh[1], pm, 0), ks);
        int max_ks = 0;
        for (int k : ks) max_ks = std::max(max_ks, k);
        for (int ms = 0; ms <= max_ks; ms = ms ? ms + 1 : 8) best[pm] = std::min(best[pm], tg_model_makespan(ks, ms, sh[2]));
      }
      printf("%s %dx%d %.3f\n", L.name, sh[0], sh[1], best[1] / best[0]);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) return 2;
  if (!strcmp(argv[1], "model")) return run_model();
  return run_geometry(argv[1], argc == 3 ? atoi(argv[2]) : -1);
}
