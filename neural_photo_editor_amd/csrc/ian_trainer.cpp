// ian_trainer: the train_IAN.py step (make_training_functions, train_IAN.py:47-352: update_gen / update_discrim on the
// full IAN of IAN.py:67-228) behind ONE C entry, ian_train_step.  A C / C++ caller owns nothing but host or
// device buffers for the minibatch; the three Adam groups, every activation, the batch-norm running averages and the frozen
// MADE parameters live inside the object.
//
// This is the ONE sequencer of the training step (round 4: neural_photo_editor_amd/trainer.py is a thin ctypes caller of it,
// no second wiring exists).  It uses only the public C ABI of include/ian_train.h plus hipMalloc / hipMemcpy / streams / events.
//
// Data parallel (train_IAN.py has none): one process per GPU, the minibatch is sharded, losses are means over the
// GLOBAL batch.  The collectives arrive through a small callback table (ian_comm_ops: allreduce_sum / wait_all / allgather on
// device buffers and HIP streams) that the host fills -- from torch.distributed (backend "nccl" = RCCL over xGMI; gloo in the
// tests) in neural_photo_editor_amd/trainer.py -- so the same entry, ian_train_step, runs at world size 1 and N:
//   * gradient all-reduce OVERLAPPED with backward: a group's flat gradient buffer is cut into buckets (16 MB); the first
//     sweep of each update kind records the order of gradient writes; from then on a bucket is handed to allreduce_sum on a
//     side stream the moment its LAST writer kernel has been issued (events on the compute stream and on the weight-gradient
//     stream), while the compute stream goes on; the compute stream waits (wait_all) only before the regularisers and Adam;
//   * exact = 1 (SyncBN + MinibatchLayer all-gather): the float64 batch-statistics sums of every normalisation are
//     all-gathered and combined in RANK ORDER by the same pairwise tree the per-rank reduction uses (bitwise the
//     single-process statistics for power-of-two shards), the MinibatchLayer activations and their gradients are
//     all-gathered (layers.py:506-524 couples the whole minibatch), which makes the N-GPU step the same function of the
//     global minibatch as the reference's 1-GPU step;  exact = 0: local statistics, NOT the reference's arithmetic.
//
// Graph (train_IAN.py:116-149): encoder(X) -> z ~ N(mu, e^ls) -> IAF -> decoder -> X_hat; encoder(X_hat);
// decoder(IAF(Z)) -> X_gen; encoder(X_gen); every pass in batch-statistics batch-norm mode.
// Updates (train_IAN.py:253-276): three Adam groups -- encoder_params (update_discrim), decoder_params (update_gen),
// Z_params (both, ONE Adam instance).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <deque>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/ian_train.h"
#include "ian_guard.h"   // IAN_SANITIZE builds: guard bands around every device allocation (no-op otherwise)

namespace {

constexpr float BN_EPS = 1e-4f;
constexpr int ENC_WIDTHS[4] = {128, 256, 512, 1024};
struct DecStage {
  const char* dc;
  int ci, co, hw;
  const char* blk;
  std::vector<int> scales;
};
const std::vector<DecStage>& dec_stages() {  // (deconv, cin, cout, in_hw, block, scales) IAN.py:139-171
  static const std::vector<DecStage> s = {{"dec_conv1", 512, 512, 4, "dec_conv2a", {0, 2}},
                                          {"dec_conv2", 512, 256, 8, "dec_conv3a", {0, 2, 3}},
                                          {"dec_conv3", 256, 128, 16, "dec_conv4a", {0, 2, 3}}};
  return s;
}
const std::vector<int> HEAD_SCALES = {2, 3, 4};
const std::pair<const char*, int> HEADS[5] = {{"R", 128}, {"G_a", 128}, {"G_b", 2}, {"B_a", 128}, {"B_b", 4}};   // RGB-Beta head MDCLs: name, cin
inline int cs(int c) { return (c + 31) / 32 * 32; }

std::vector<std::string> mdcl_names(const std::string& name, const std::vector<int>& scales) {
  std::vector<std::string> v = {name + "W", name + "_coeff_base"};
  for (int s : scales) v.push_back(name + (s == 0 ? std::string("_coeff_1x1") : "_coeff_" + std::to_string(s)));
  return v;
}

struct Shape {
  std::vector<int64_t> d;
  int64_t numel() const {
    int64_t n = 1;
    for (auto v : d) n *= v;
    return n;
  }
};

enum GroupId { G_ENC = 0, G_Z = 1, G_DEC = 2, G_STATS = 3 };  // encoder_params, Z_params, decoder_params; batch-norm running averages

struct Group {  // flat device buffers in the reference (Theano) layouts; 0..2 are one Adam instance each, G_STATS is not trainable
  std::vector<int> params;  // indices into ian_trainer::params, in declaration order
  int64_t numel = 0;
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;
  int t = 0;
};
struct Param {
  std::string name;
  int group;
  int64_t off;
  Shape shape;
};
struct PRef {  // a parameter resolved by name at finalize: index into ian_trainer::params (mark, touched), value, gradient (null: running average)
  int id = -1;
  float *p = nullptr, *g = nullptr;
};

struct BN {  // Lasagne batch_norm in training mode: state of one normalisation in one pass
  int C = 0;
  double *sums = nullptr, *bsums = nullptr;   // float64 column sums (kernels_train.hip NUMERICS)
  float *mean = nullptr, *inv_std = nullptr, *scale = nullptr, *shift = nullptr;
  float count = 1.f;
};

struct LayerRef {
  std::string key;
  int kind = 0;
  ian_layer* l = nullptr;
  std::vector<int> ids;               // its parameters as mark() / ian_layer_set_params / ian_layer_backward_weight take them; empty:
  std::vector<const float*> values;   // weights are set elsewhere (the MinibatchLayer's normalised theta)
  std::vector<float*> grads;
};
struct Layers {  // every layer of IAN.py:67-228 by its Theano name (build_layers); enc_conv[1..4]; stage[i] = deconv, MDCL, MDCL2 of dec_stages()[i]
  LayerRef *enc_conv[5], *enc_fc1, *enc_mu, *enc_logsigma, *mb, *l_dec_fc2, *stage[3][3], *dec_conv4, *R, *G_a, *G_b, *B_a, *B_b;
};

// "linear layer + batch-norm + activation" of one pass -- Lasagne's batch_norm(layer) in training mode: built when the pass's buffers are
// allocated (make_unit), run by unit_forward / unit_backward
struct Unit {
  LayerRef* L = nullptr;
  BN bn;
  float *y = nullptr, *a = nullptr;     // the layer's raw output, the normalised and activated output
  float *dA = nullptr, *dy = nullptr;   // gradient wrt a (what the backward starts from), wrt y (dy == dA: in place)
  int64_t rows = 0;
  int C = 0, stride = 0, act = 0;
  int ld = 0;                           // pixel stride handed to the layer calls (0 = the layer's own round_up(cout, 32))
  bool epilogue = false;                // conv / deconv / MDCL: the GEMMs can carry the batch statistics in their epilogue (fused_stats)
  PRef gamma, beta, run_mean, run_inv_std;
};
struct EncPass {  // encoder(X | X_hat | X_gen) + discriminator head; a[1..4] / da[1..4]: lrelu outputs of enc_conv1..4 and their gradients
  float *x, *dx, *a[5], *da[5], *feat, *dfeat, *act, *dact, *mb, *dmb, *act_all, *dmb_all, *p, *loss, *dlogits;
  Unit u[5];      // u[2..4]: enc_conv<i> + bnorm<i> + lrelu
};
struct ZPass {
  Unit fc1, mu, ls;
  float *z0, *z, *dz0, *kl;
};
struct DecPass {  // decoder(z | IAF(Z_rand))
  float *h0, *dh0;
  Unit stage[3][3];   // per dec_stages() entry: deconv, MDCL, MDCL2 (+ the block's input), each + bnorm<j> + lrelu
  Unit u4;            // dec_conv4 + bnorm_dc4 + lrelu
  float *R, *G, *B, *Ga, *Ba, *RG, *gR, *gG, *gB, *dRG, *dRt, *xhat, *dxhat, *tmp_img, *dz;
};

struct Bucket {  // a slice of one group's flat gradient buffer = one all-reduce message
  int group;     // GroupId
  int64_t lo, hi;
  std::set<int> params;
  int ready;     // index (1-based) of the last gradient write that lands in [lo, hi); 0: nothing writes it
  bool fired;
};
struct OverlapRec { int which, group; int64_t lo, bytes; int issued_at_write, writes_in_backward; };

}  // namespace

struct ian_trainer {
  ian_train_config cfg;
  int n = 0;
  std::string err;
  bool finalized = false;
  std::map<std::string, Shape> shapes;             // every parameter the graph owns
  std::map<std::string, std::vector<float>> host;  // values loaded before finalize
  Group grp[4];                                    // by GroupId
  std::vector<Param> params;                       // every parameter that lives in a group
  std::map<std::string, int> pindex;               // name -> index into params (the caller-facing entries and finalize only)
  std::deque<LayerRef> layers;                     // in creation order
  Layers L;
  struct { PRef enc_conv1_b, mb_theta, mb_lws, mb_b, discrimi_W, l_dec_fc2_b; } pr;   // parameters the passes touch outside a layer or unit
  std::string unresolved;                          // first name finalize could not resolve (finalize fails with it)
  std::vector<float*> allocs;
  std::map<const void*, size_t> alloc_floats;      // size of every allocation (ian_trainer_buffer)
  std::vector<float> masks[3];
  int made_n = 0;
  float *made_w = nullptr, *made_b = nullptr;
  int32_t *fc2_perm = nullptr, *fc2_inv = nullptr;
  float *fc2_bias = nullptr, *fc2_db = nullptr, *fc2_tmp = nullptr;
  double *ws_stats = nullptr, *tmp_vals = nullptr, *tmp_big = nullptr, *gbuf = nullptr;   // float64 statistics workspaces
  float *ws_loss = nullptr, *scalars = nullptr, *mb_W = nullptr, *mb_dW = nullptr, *mb_colscale = nullptr, *ortho_vals = nullptr;
  size_t ws_stats_cap = 0, gbuf_cap = 0;
  bool oom = false;                                 // a device allocation failed (checked at the end of finalize)
  bool dirty[3] = {false, false, false};            // groups whose packed weights are stale (refresh_weights)
  std::vector<char> touched;                        // per parameter: its gradient has been written in this sweep (the next write accumulates)
  EncPass EX, EH, EG;
  ZPass ZS;
  DecPass DZ, DG;
  std::map<std::string, float*> bufs;               // "<pass>.<name>" -> buffer and "<pass>.<bn>" -> statistics, filled by the *_alloc
  std::map<std::string, BN*> bns;                   // functions: what ian_trainer_buffer serves (the step path does not look names up)
  float *zgen = nullptr, *zgen0 = nullptr, *xin = nullptr, *zin = nullptr, *epsin = nullptr;
  const float* X = nullptr;
  const float* eps = nullptr;
  int head6 = 1, update_running = 1;
  // batch statistics in the epilogue of the GEMM that produces the normalised tensor (ian_layer_stats_next) instead of a colstats
  // pass that re-reads it; single-process step only: the data-parallel `exact` step keeps the per-image chunks of ian_k_colstats,
  // whose partition does not depend on the tile shape the autotuner picks per batch size (bitwise rank-order invariance).
  // OFF, and effective in libian_ablation.so only (the product's GEMMs answer every request with 0 chunks): measured on MI355X at
  // 128 images, in-process A/B, 103.9 vs 99.7 ms per G+D pair -- the colstats passes are HBM-bound kernels that already run under
  // the weight-gradient GEMMs of the second stream; folded into the epilogue the same bytes sit on the MFMA-bound critical path
  int fused_stats = 0;
  hipStream_t st = nullptr;
  // weight-gradient GEMMs (ian_layer_backward_weight: 19 % of the step) are off the critical path -- nothing reads a gradient
  // before the regularisers -- so they are issued on a second stream behind an event on the compute stream (their dy operand
  // is final at that point and is not written again in the same sweep) and overlap the element-wise kernels of the
  // backward-data chain; the compute stream joins before the regularisers.  Same launches, same per-parameter order.
  int overlap_wgrad = 1;
  int wgrad_priority = 0;                           // weight-gradient stream created with the lowest stream priority (make_wgrad_stream)
  hipStream_t st2 = nullptr;
  // TIMING-ONLY experiment (IAN_DUAL_CHAIN_TIMING=1, libian_ablation.so only; RESULTS ARE WRONG): the (Z_rand -> decoder -> encoder) chain of
  // forward and backward on its own stream next to the (X -> encoder -> decoder -> encoder) chain, ignoring that both chains use the SAME
  // layer objects' split-K / statistics workspaces and accumulate into the same gradient buffers -- what a real two-chain step (per-chain
  // layer clones, private gradient accumulators) could gain at most
  int dual_timing = 0;
  hipStream_t stB = nullptr;
  std::vector<hipEvent_t> events;
  size_t ev_used = 0;
  hipStream_t last_stream = nullptr;               // stream of the previous entry: a different one is synchronised first
  bool have_last_stream = false;
  // ---- data parallel ------------------------------------------------------------------------------------------------
  ian_comm_ops comm;
  int world = 1, rank = 0, exact = 0, N = 0;        // N = global batch (losses are means over it)
  int overlap = 1;                                  // hand gradient buckets to the all-reduce while backward still runs
  int64_t bucket_bytes = 16 << 20;                  // xGMI is point-to-point: a few large messages
  hipStream_t st_comm = nullptr;                    // side stream the buckets are handed over on
  std::map<int, std::vector<Bucket>> plans;         // per update kind (0 gen, 1 discrim)
  std::map<int, int> plan_key;
  std::vector<Bucket>* buckets = nullptr;           // the plan this sweep follows (nullptr: record, reduce at the end)
  std::vector<std::vector<int>> evlog;              // gradient writes of this sweep (parameter indices), in issue order
  int which_now = 0, nfired = 0;
  std::deque<OverlapRec> overlap_log;               // last few sweeps (tests/test_gpu_dp.py, bench.py)
  int measure_exposed = 0;
  hipEvent_t ex0 = nullptr, ex1 = nullptr;
  bool ex_pending = false;
  int ex_which = 0;
  double exposed_ms[2] = {0, 0};
  int exposed_n[2] = {0, 0};
  // measure_exposed: time the compute stream spends inside the exact-mode all-gathers (event pairs around every comm.allgather).
  // Two pools used by alternate steps: a pool is folded (its events completed a whole step ago) right before it is reused.
  std::vector<std::pair<hipEvent_t, hipEvent_t>> gev[2];
  size_t gev_used[2] = {0, 0};
  int gev_which[2] = {0, 0}, gpar = 0;
  double gather_ms[2] = {0, 0}, gather_calls[2] = {0, 0};
  int gather_n[2] = {0, 0};
  const float *xhat_override = nullptr, *xgen_override = nullptr;   // test hook of ian_trainer_forward
};

namespace {

int tfail(ian_trainer* t, int code, const char* fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (t) t->err = buf;
  return code;
}
#define TK(expr)                                                                                      \
  do {                                                                                                \
    const int rc_ = (expr);                                                                           \
    if (rc_) return tfail(t, rc_, "%s failed (%d): %s", #expr, rc_, ian_k_last_error() ? ian_k_last_error() : "?"); \
  } while (0)
#define TL(layer, expr)                                                                               \
  do {                                                                                                \
    const int rc_ = (expr);                                                                           \
    if (rc_) return tfail(t, rc_, "%s failed (%d): %s", #expr, rc_, ian_layer_last_error(layer) ? ian_layer_last_error(layer) : "?"); \
  } while (0)
#define LCALL(L, fn, ...) TL((L)->l, fn((L)->l, __VA_ARGS__))   // a call on a LayerRef*: the line names its layer once
#define THIP(expr)                                                                                    \
  do {                                                                                                \
    const hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return tfail(t, -20, "%s: %s", #expr, hipGetErrorString(e_));              \
  } while (0)

float* dalloc(ian_trainer* t, size_t floats) {   // zero-filled device floats; a failure sets t->oom (finalize reports it)
  float* p = nullptr;
  const size_t bytes = (floats ? floats : 1) * sizeof(float);
  if (hipMalloc((void**)&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    t->oom = true;
    return nullptr;
  }
  if (hipMemset(p, 0, bytes) != hipSuccess) {
    (void)hipGetLastError();
    t->oom = true;
  }
  t->allocs.push_back(p);
  t->alloc_floats[p] = floats;
  return p;
}
double* dalloc64(ian_trainer* t, size_t doubles) { return reinterpret_cast<double*>(dalloc(t, 2 * doubles)); }

void add_param(ian_trainer* t, int group, const std::string& name, std::vector<int64_t> shape) {
  Group& g = t->grp[group];
  Shape s{shape};
  t->shapes[name] = s;
  t->pindex[name] = (int)t->params.size();
  g.params.push_back((int)t->params.size());
  t->params.push_back({name, group, g.numel, s});
  g.numel += (s.numel() + 3) / 4 * 4;  // keep every tensor 16-byte aligned
}
// Names are resolved here, once, while ian_trainer_finalize wires the graph (the groups' buffers exist by then): a name that is not
// declared is remembered and makes finalize fail; the step path holds PRef / LayerRef* / Unit and never looks a name up.
PRef param(ian_trainer* t, const std::string& name) {
  PRef r;
  auto it = t->pindex.find(name);
  if (it == t->pindex.end()) {
    if (t->unresolved.empty()) t->unresolved = name;
    return r;
  }
  const Param& q = t->params[it->second];
  const Group& g = t->grp[q.group];
  r.id = it->second;
  r.p = g.p + q.off;
  r.g = g.g ? g.g + q.off : nullptr;
  return r;
}
void declare_parameters(ian_trainer* t) {
  const int Z = t->cfg.num_latents;
  add_param(t, G_ENC, "enc_conv1.W", {128, 3, 5, 5});
  add_param(t, G_ENC, "enc_conv1.b", {128});
  for (int i = 2; i <= 4; ++i) {
    const std::string s = std::to_string(i);
    add_param(t, G_ENC, "enc_conv" + s + ".W", {ENC_WIDTHS[i - 1], ENC_WIDTHS[i - 2], 5, 5});
    add_param(t, G_ENC, "bnorm" + s + ".beta", {ENC_WIDTHS[i - 1]});
    add_param(t, G_ENC, "bnorm" + s + ".gamma", {ENC_WIDTHS[i - 1]});
  }
  add_param(t, G_ENC, "minibatch_discrim.theta", {1024, 500, 5});
  add_param(t, G_ENC, "minibatch_discrim.log_weight_scale", {500, 5});
  add_param(t, G_ENC, "minibatch_discrim.b", {500});
  add_param(t, G_ENC, "discrimi.W", {1524, 3});
  add_param(t, G_Z, "enc_fc1.W", {16384, 1000});
  add_param(t, G_Z, "bnorm_enc_fc1.beta", {1000});
  add_param(t, G_Z, "bnorm_enc_fc1.gamma", {1000});
  for (const char* nm : {"enc_mu", "enc_logsigma"}) {
    const std::string bn = std::string(nm) == "enc_mu" ? "mu_bnorm" : "ls_bnorm";
    add_param(t, G_Z, std::string(nm) + ".W", {1000, Z});
    add_param(t, G_Z, bn + ".beta", {Z});
    add_param(t, G_Z, bn + ".gamma", {Z});
  }
  add_param(t, G_DEC, "l_dec_fc2.W", {Z, 8192});
  add_param(t, G_DEC, "l_dec_fc2.b", {8192});
  auto add_mdcl = [&](const std::string& name, int co, int ci, const std::vector<int>& sc) {
    auto names = mdcl_names(name, sc);
    add_param(t, G_DEC, names[0], {co, ci, 3, 3});
    for (size_t i = 1; i < names.size(); ++i) add_param(t, G_DEC, names[i], {co});
  };
  for (const DecStage& s : dec_stages()) {
    const std::string blk = s.blk;
    add_param(t, G_DEC, std::string(s.dc) + ".W", {s.ci, s.co, 5, 5});
    add_param(t, G_DEC, blk + "bnorm0.beta", {s.co});
    add_param(t, G_DEC, blk + "bnorm0.gamma", {s.co});
    add_mdcl(blk, s.co, s.co, s.scales);
    add_param(t, G_DEC, blk + "bnorm1.beta", {s.co});
    add_param(t, G_DEC, blk + "bnorm1.gamma", {s.co});
    add_mdcl(blk + "2", s.co, s.co, s.scales);
    add_param(t, G_DEC, blk + "bnorm2.beta", {s.co});
    add_param(t, G_DEC, blk + "bnorm2.gamma", {s.co});
  }
  add_param(t, G_DEC, "dec_conv4.W", {128, 128, 5, 5});
  add_param(t, G_DEC, "bnorm_dc4.beta", {128});
  add_param(t, G_DEC, "bnorm_dc4.gamma", {128});
  for (auto& h : HEADS) add_mdcl(h.first, 2, h.second, HEAD_SCALES);
  // batch-norm running averages (not trainable; Lasagne BatchNormLayer alpha = 0.1): what the deterministic graphs of
  // API.py / sample_IAN.py normalise with after training
  std::vector<std::pair<std::string, int>> bns = {{"bnorm2", 256}, {"bnorm3", 512}, {"bnorm4", 1024}, {"bnorm_enc_fc1", 1000},
                                                  {"mu_bnorm", Z}, {"ls_bnorm", Z}, {"bnorm_dc4", 128}};
  for (const DecStage& s : dec_stages())
    for (int j = 0; j < 3; ++j) bns.push_back({std::string(s.blk) + "bnorm" + std::to_string(j), s.co});
  for (auto& b : bns)
    for (const char* sfx : {".mean", ".inv_std"}) add_param(t, G_STATS, b.first + sfx, {b.second});
  // frozen MADE parameters (never trained: train_IAN.py:184-194)
  for (const char* m : {"l_IAF_mu", "l_IAF_ls"})
    for (const char* l : {"_input", "_output_W", "_output_D"}) {
      t->shapes[std::string(m) + l + ".W"] = Shape{{Z, Z}};
      t->shapes[std::string(m) + l + ".b"] = Shape{{Z}};
    }
}

int make_layer(ian_trainer* t, LayerRef** out, const std::string& key, int kind, int cin, int cout, int in_h, int in_w, const std::vector<int>& scales,
               const int* flat, const int* unflat, const std::vector<std::string>& pnames) {
  ian_op_desc d;
  memset(&d, 0, sizeof d);
  d.kind = kind; d.cin = cin; d.cout = cout; d.in_h = in_h; d.in_w = in_w;
  d.src = d.dst = 0; d.src2 = d.src3 = -1;
  if (flat) { d.flat_c = flat[0]; d.flat_h = flat[1]; d.flat_w = flat[2]; }
  if (unflat) { d.unflat_c = unflat[0]; d.unflat_h = unflat[1]; d.unflat_w = unflat[2]; }
  d.n_scales = (int)scales.size();
  for (size_t i = 0; i < scales.size(); ++i) d.scales[i] = scales[i];
  LayerRef r;
  r.key = key;
  r.kind = kind;
  const int rc = ian_layer_create(&d, t->cfg.deconv_flip ? 1 : 0, &r.l);
  if (rc) return tfail(t, rc, "ian_layer_create(%s) failed (%d)%s", key.c_str(), rc, rc == -10 ? ": no HIP device, libian has no CPU fallback" : "");
  for (auto& nme : pnames) {
    const PRef p = param(t, nme);
    r.ids.push_back(p.id); r.values.push_back(p.p); r.grads.push_back(p.g);
  }
  t->layers.push_back(r);
  *out = &t->layers.back();
  return 0;
}

int build_layers(ian_trainer* t) {
  const int Z = t->cfg.num_latents;
  Layers& L = t->L;
  int cin = 3, rc;
  for (int i = 0; i < 4; ++i) {
    const std::string nm = "enc_conv" + std::to_string(i + 1);
    if ((rc = make_layer(t, &L.enc_conv[i + 1], nm, IAN_OP_CONV5S2, cin, ENC_WIDTHS[i], 64 >> i, 64 >> i, {}, nullptr, nullptr, {nm + ".W"}))) return rc;
    cin = ENC_WIDTHS[i];
  }
  const int flat[3] = {1024, 4, 4}, unflat[3] = {512, 4, 4};
  if ((rc = make_layer(t, &L.enc_fc1, "enc_fc1", IAN_OP_DENSE, 16384, 1000, 1, 1, {}, flat, nullptr, {"enc_fc1.W"}))) return rc;
  if ((rc = make_layer(t, &L.enc_mu, "enc_mu", IAN_OP_DENSE, 1000, Z, 1, 1, {}, nullptr, nullptr, {"enc_mu.W"}))) return rc;
  if ((rc = make_layer(t, &L.enc_logsigma, "enc_logsigma", IAN_OP_DENSE, 1000, Z, 1, 1, {}, nullptr, nullptr, {"enc_logsigma.W"}))) return rc;
  if ((rc = make_layer(t, &L.mb, "mb", IAN_OP_DENSE, 1024, 2500, 1, 1, {}, nullptr, nullptr, {}))) return rc;  // weights = normalised theta (layers.py:494)
  if ((rc = make_layer(t, &L.l_dec_fc2, "l_dec_fc2", IAN_OP_DENSE, Z, 8192, 1, 1, {}, nullptr, unflat, {"l_dec_fc2.W"}))) return rc;
  for (size_t si = 0; si < dec_stages().size(); ++si) {
    const DecStage& s = dec_stages()[si];
    const std::string blk = s.blk;
    LayerRef** l = t->L.stage[si];
    if ((rc = make_layer(t, &l[0], s.dc, IAN_OP_DECONV5S2, s.ci, s.co, s.hw, s.hw, {}, nullptr, nullptr, {std::string(s.dc) + ".W"}))) return rc;
    if ((rc = make_layer(t, &l[1], blk, IAN_OP_MDC3, s.co, s.co, 2 * s.hw, 2 * s.hw, s.scales, nullptr, nullptr, mdcl_names(blk, s.scales)))) return rc;
    if ((rc = make_layer(t, &l[2], blk + "2", IAN_OP_MDC3, s.co, s.co, 2 * s.hw, 2 * s.hw, s.scales, nullptr, nullptr, mdcl_names(blk + "2", s.scales)))) return rc;
  }
  if ((rc = make_layer(t, &L.dec_conv4, "dec_conv4", IAN_OP_DECONV5S2, 128, 128, 32, 32, {}, nullptr, nullptr, {"dec_conv4.W"}))) return rc;
  LayerRef** heads[5] = {&L.R, &L.G_a, &L.G_b, &L.B_a, &L.B_b};
  for (int i = 0; i < 5; ++i)
    if ((rc = make_layer(t, heads[i], HEADS[i].first, IAN_OP_MDC3, HEADS[i].second, 2, 64, 64, HEAD_SCALES, nullptr, nullptr, mdcl_names(HEADS[i].first, HEAD_SCALES))))
      return rc;
  return 0;
}

BN make_bn(ian_trainer* t, int C) {
  BN b;
  b.C = C;
  b.sums = dalloc64(t, 2 * C); b.bsums = dalloc64(t, 2 * C);
  b.mean = dalloc(t, C); b.inv_std = dalloc(t, C); b.scale = dalloc(t, C); b.shift = dalloc(t, C);
  return b;
}
float* buf(ian_trainer* t, const std::string& pass, const std::string& name, size_t floats) {  // allocate and enter in the registry
  return t->bufs[pass + "." + name] = dalloc(t, floats);
}
// u.y / u.a / u.dA / u.dy are set by the caller; `bnorm`: Theano name of the normalisation (<bnorm>.gamma | beta | mean | inv_std),
// `key`: its name in ian_trainer_buffer
void make_unit(ian_trainer* t, Unit& u, const std::string& pass, const std::string& key, LayerRef* L, const std::string& bnorm, int64_t rows, int C,
               int stride, int ld, int act) {
  u.L = L;
  u.bn = make_bn(t, C);
  t->bns[pass + "." + key] = &u.bn;
  u.rows = rows; u.C = C; u.stride = stride; u.ld = ld; u.act = act;
  u.epilogue = L->kind != IAN_OP_DENSE;
  u.gamma = param(t, bnorm + ".gamma"); u.beta = param(t, bnorm + ".beta");
  u.run_mean = param(t, bnorm + ".mean"); u.run_inv_std = param(t, bnorm + ".inv_std");
}

void enc_alloc(ian_trainer* t, EncPass& E, const std::string& pass) {
  const size_t n = t->n;
  E.x = buf(t, pass, "x", n * 64 * 64 * 32); E.dx = buf(t, pass, "dx", n * 64 * 64 * 32);
  for (int i = 1; i <= 4; ++i) {
    const int hw = 64 >> i, w = ENC_WIDTHS[i - 1];
    const std::string s = std::to_string(i);
    E.a[i] = buf(t, pass, "a" + s, n * hw * hw * w); E.da[i] = buf(t, pass, "da" + s, n * hw * hw * w);
    if (i > 1) {
      Unit& u = E.u[i];
      u.y = buf(t, pass, "y" + s, n * hw * hw * w); u.a = E.a[i]; u.dA = u.dy = E.da[i];
      make_unit(t, u, pass, "bn" + s, t->L.enc_conv[i], "bnorm" + s, (int64_t)n * hw * hw, w, w, 0, IAN_ACT_LRELU);
    }
  }
  E.feat = buf(t, pass, "feat", n * 1024); E.dfeat = buf(t, pass, "dfeat", n * 1024);
  E.act = buf(t, pass, "act", n * cs(2500)); E.dact = buf(t, pass, "dact", n * cs(2500));
  E.mb = buf(t, pass, "mb", n * cs(1524)); E.dmb = buf(t, pass, "dmb", n * cs(1524));
  if (t->exact) {  // MinibatchLayer over the GLOBAL minibatch (layers.py:506-524): all ranks' activations / feature gradients
    E.act_all = buf(t, pass, "act_all", (size_t)t->N * cs(2500));
    E.dmb_all = buf(t, pass, "dmb_all", (size_t)t->N * cs(1524));
  }
  E.p = buf(t, pass, "p", n * 3); E.loss = buf(t, pass, "loss", n * 4); E.dlogits = buf(t, pass, "dlogits", n * 4);
}
void z_alloc(ian_trainer* t) {
  const size_t n = t->n;
  const int Zd = t->cfg.num_latents;
  ZPass& S = t->ZS;
  S.fc1.y = buf(t, "ZS", "y_fc1", n * 1024); S.fc1.a = buf(t, "ZS", "f", n * 1024); S.fc1.dA = S.fc1.dy = buf(t, "ZS", "df", n * 1024);
  make_unit(t, S.fc1, "ZS", "bn_fc1", t->L.enc_fc1, "bnorm_enc_fc1", n, 1000, 1024, 1024, IAN_ACT_RELU);
  const struct { Unit* u; const char* nm; LayerRef* L; const char* bnorm; } lat[2] = {{&S.mu, "mu", t->L.enc_mu, "mu_bnorm"},
                                                                                   {&S.ls, "ls", t->L.enc_logsigma, "ls_bnorm"}};
  for (auto& l : lat) {
    const std::string nm = l.nm;
    l.u->y = buf(t, "ZS", "y_" + nm, n * 128); l.u->a = buf(t, "ZS", nm, n * 128); l.u->dA = l.u->dy = buf(t, "ZS", "d" + nm, n * 128);
    make_unit(t, *l.u, "ZS", "bn_" + nm, l.L, l.bnorm, n, Zd, 128, 128, 0);
  }
  {  // the two latent normalisations read the same input in the same stage: their float64 sums lie side by side so that the
     // data-parallel `exact` step combines both with ONE all-gather per direction (z_forward / z_backward)
    double *js = dalloc64(t, 4 * Zd), *jb = dalloc64(t, 4 * Zd);
    S.mu.bn.sums = js; S.ls.bn.sums = js ? js + 2 * Zd : nullptr;
    S.mu.bn.bsums = jb; S.ls.bn.bsums = jb ? jb + 2 * Zd : nullptr;
  }
  S.z0 = buf(t, "ZS", "z0", n * 128); S.z = buf(t, "ZS", "z", n * 128); S.dz0 = buf(t, "ZS", "dz0", n * 128); S.kl = buf(t, "ZS", "kl", n * 100);
}
void dec_alloc(ian_trainer* t, DecPass& D, const std::string& pass) {
  const size_t n = t->n;
  D.h0 = buf(t, pass, "h0", n * 16 * 512); D.dh0 = buf(t, pass, "dh0", n * 16 * 512);
  for (size_t si = 0; si < dec_stages().size(); ++si) {
    const DecStage& s = dec_stages()[si];
    const int64_t rows = (int64_t)n * (2 * s.hw) * (2 * s.hw);
    const std::string blk = s.blk;
    Unit* u = D.stage[si];   // x = deconv(h); a = lrelu(bn0(x)); c = lrelu(bn1(b = MDCL(a))); h = lrelu(bn2(e = x + MDCL2(c)))
    const std::pair<const char*, float**> slots[10] = {{"x", &u[0].y}, {"a", &u[0].a}, {"b", &u[1].y}, {"c", &u[1].a}, {"e", &u[2].y},
                                                       {"h", &u[2].a}, {"dx", &u[0].dy}, {"da", &u[0].dA}, {"dc", &u[1].dA}, {"dh", &u[2].dA}};
    for (auto& sl : slots) *sl.second = buf(t, pass, blk + "_" + sl.first, (size_t)rows * s.co);
    u[1].dy = u[1].dA; u[2].dy = u[2].dA;
    for (int j = 0; j < 3; ++j)
      make_unit(t, u[j], pass, blk + "_bn" + std::to_string(j), t->L.stage[si][j], blk + "bnorm" + std::to_string(j), rows, s.co, s.co, 0, IAN_ACT_LRELU);
  }
  D.u4.y = buf(t, pass, "y4", n * 4096 * 128); D.u4.a = buf(t, pass, "h4", n * 4096 * 128); D.u4.dA = D.u4.dy = buf(t, pass, "dh4", n * 4096 * 128);
  make_unit(t, D.u4, pass, "bn4", t->L.dec_conv4, "bnorm_dc4", (int64_t)n * 4096, 128, 128, 0, IAN_ACT_LRELU);
  const std::pair<const char*, float**> maps[11] = {{"R", &D.R}, {"G", &D.G}, {"B", &D.B}, {"Ga", &D.Ga}, {"Ba", &D.Ba}, {"RG", &D.RG},
                                                    {"gR", &D.gR}, {"gG", &D.gG}, {"gB", &D.gB}, {"dRG", &D.dRG}, {"dRt", &D.dRt}};
  for (auto& m : maps) *m.second = buf(t, pass, m.first, n * 4096 * 32);
  D.xhat = buf(t, pass, "xhat", n * 3 * 4096); D.dxhat = buf(t, pass, "dxhat", n * 3 * 4096); D.tmp_img = buf(t, pass, "tmp_img", n * 3 * 4096);
  D.dz = buf(t, pass, "dz", n * 128);
}

// ---- parameter refresh (after every optimiser update): reference layout -> kernel layouts -------------------------
int refresh_weights(ian_trainer* t) {
  if (!t->dirty[G_ENC] && !t->dirty[G_Z] && !t->dirty[G_DEC]) return 0;
  for (LayerRef& r : t->layers) {
    if (r.ids.empty() || !t->dirty[t->params[r.ids[0]].group]) continue;
    LCALL(&r, ian_layer_set_params, r.values.data(), (int)r.values.size(), t->st);
  }
  if (t->dirty[G_ENC]) {
    TK(ian_k_mb_weight(t->pr.mb_theta.p, t->pr.mb_lws.p, t->mb_W, t->mb_colscale, 1024, 2500, t->st));
    const float* w = t->mb_W;
    LCALL(t->L.mb, ian_layer_set_params, &w, 1, t->st);
  }
  if (t->dirty[G_DEC]) TK(ian_k_gather(t->pr.l_dec_fc2_b.p, t->fc2_perm, t->fc2_bias, 8192, t->st));
  t->dirty[G_ENC] = t->dirty[G_Z] = t->dirty[G_DEC] = false;
  return 0;
}
// ---- building blocks ------------------------------------------------------------------------------------------------
int chunks(const ian_trainer* t, int64_t rows) {
  // chunk SIZE depends on the per-image extent only (one image, or 512 rows of one): include/ian_train.h, ian_k_colstats
  const int64_t rpi = rows / t->n > 0 ? rows / t->n : 1;
  if (rows == (int64_t)t->n * rpi) return (int)(t->n * (rpi / 512 > 0 ? rpi / 512 : 1));
  return (int)(rows < 256 ? rows : 256);
}
int ws_for(ian_trainer* t, int64_t rows, int C, double** out) {
  const size_t need = (size_t)chunks(t, rows) * 2 * C;
  if (t->ws_stats_cap < need) {
    double* p = dalloc64(t, need);
    if (!p) return tfail(t, -20, "out of device memory (statistics workspace)");
    t->ws_stats = p;
    t->ws_stats_cap = need;
  }
  *out = t->ws_stats;
  return 0;
}
int next_event(ian_trainer* t, hipEvent_t* e) {
  if (t->ev_used == t->events.size()) {
    hipEvent_t ne;
    THIP(hipEventCreateWithFlags(&ne, hipEventDisableTiming));
    t->events.push_back(ne);
  }
  *e = t->events[t->ev_used++];
  return 0;
}

// ---- gradient all-reduce overlapped with backward ----------------------------------------------------------
// encoder_params receive contributions from three encoder passes, decoder_params from two decoder passes, so the "last" writer
// of a bucket is a property of the whole backward sweep of an update kind: every gradient write is reported through mark();
// the first sweep of a kind records the order, later sweeps fire a bucket right after its last write.
int fire(ian_trainer* t, Bucket& b) {
  Group& g = t->grp[b.group];
  hipEvent_t e;
  int rc;
  if ((rc = next_event(t, &e))) return rc;
  THIP(hipEventRecord(e, t->st));                  // after the bucket's last writer on the compute stream ...
  THIP(hipStreamWaitEvent(t->st_comm, e, 0));
  if (t->overlap_wgrad && t->st2) {                // ... and on the weight-gradient stream
    if ((rc = next_event(t, &e))) return rc;
    THIP(hipEventRecord(e, t->st2));
    THIP(hipStreamWaitEvent(t->st_comm, e, 0));
  }
  rc = t->comm.allreduce_sum(t->comm.ctx, g.g + b.lo, b.hi - b.lo, t->st_comm);
  if (rc) return tfail(t, -30, "comm.allreduce_sum failed (%d) on a gradient bucket of group %d", rc, b.group);
  b.fired = true;
  ++t->nfired;
  t->overlap_log.push_back({t->which_now, b.group, b.lo, 4 * (b.hi - b.lo), (int)t->evlog.size(), 0});
  while (t->overlap_log.size() > 256) t->overlap_log.pop_front();
  return 0;
}
int mark(ian_trainer* t, const std::vector<int>& ids) {  // the gradients of these parameters have just been written (issued)
  for (int id : ids) t->touched[id] = 1;
  t->evlog.push_back(ids);
  if (!t->buckets) return 0;
  const int ev = (int)t->evlog.size();
  for (Bucket& b : *t->buckets) {
    if (b.fired) {
      for (int id : ids)
        if (b.params.count(id)) {
          t->plans.erase(t->which_now);            // stale plan: the next sweep of this kind re-records it
          t->buckets = nullptr;
          return tfail(t, -31, "gradient of %s written after its bucket was handed to the all-reduce (write order changed since the "
                               "plan was recorded; plan dropped)", t->params[id].name.c_str());
        }
    } else if (b.ready == ev) {
      int rc = fire(t, b);
      if (rc) return rc;
    }
  }
  return 0;
}
std::vector<Bucket> make_plan(ian_trainer* t, int which) {  // buckets of the groups this update kind moves, with their last writes
  std::vector<int> last(t->params.size(), 0);
  for (size_t i = 0; i < t->evlog.size(); ++i)
    for (int id : t->evlog[i]) last[id] = (int)i + 1;
  const int64_t step = t->bucket_bytes / 4 > 0 ? t->bucket_bytes / 4 : 1;
  std::vector<Bucket> plan;
  for (int gi : {which == 0 ? G_DEC : G_ENC, G_Z}) {
    const Group& g = t->grp[gi];
    for (int64_t o = 0; o < g.numel; o += step) {
      Bucket b;
      b.group = gi; b.lo = o; b.hi = o + step < g.numel ? o + step : g.numel; b.ready = 0; b.fired = false;
      for (int id : g.params) {
        const int64_t po = t->params[id].off, cnt = t->params[id].shape.numel();
        if (po < b.hi && po + cnt > b.lo) {
          b.params.insert(id);
          if (last[id] > b.ready) b.ready = last[id];
        }
      }
      plan.push_back(b);
    }
  }
  return plan;
}
int join_side_stream(ian_trainer* t);
int begin_backward(ian_trainer* t, int which) {
  // every event handed out so far has been consumed by a hipStreamWaitEvent already issued: the pool restarts here whether or not
  // the weight-gradient stream is in use (with overlap_wgrad = 0 nothing else reset it and a data-parallel run grew it by one
  // event per bucket per step)
  int jrc = join_side_stream(t);
  if (jrc) return jrc;
  t->ev_used = 0;
  t->gev_which[t->gpar] = which;
  t->touched.assign(t->params.size(), 0);
  t->evlog.clear();
  t->which_now = which;
  t->nfired = 0;
  t->buckets = nullptr;
  if (t->world == 1) return 0;
  // the recorded write order depends on these switches: a plan made under other settings is discarded
  const int key = (t->head6 ? 1 : 0) | (t->exact ? 2 : 0) | (t->update_running ? 4 : 0) | (t->overlap_wgrad ? 8 : 0);
  if (!t->plan_key.count(which) || t->plan_key[which] != key) {
    t->plans.erase(which);
    t->plan_key[which] = key;
  }
  if (!t->overlap || !t->plans.count(which)) return 0;
  t->buckets = &t->plans[which];
  for (Bucket& b : *t->buckets) b.fired = false;
  for (Bucket& b : *t->buckets)
    if (b.ready == 0) {
      int rc = fire(t, b);
      if (rc) return rc;
    }
  return 0;
}
void fold_exposed(ian_trainer* t) {   // fold a pending exposed-time measurement in (the caller knows that its events have completed or waits)
  if (!t->ex_pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(t->ex1) == hipSuccess && hipEventElapsedTime(&ms, t->ex0, t->ex1) == hipSuccess) {
    t->exposed_ms[t->ex_which] += ms;
    t->exposed_n[t->ex_which] += 1;
  }
  (void)hipGetLastError();
  t->ex_pending = false;
}
int finish_allreduce(ian_trainer* t, int which) {  // after backward: reduce what has not been handed over yet, then the compute stream waits
  int rc;
  if ((rc = join_side_stream(t))) return rc;
  if (t->world == 1) return 0;
  if (!t->buckets) {                               // first sweep of this kind (or overlap off): plan, then reduce everything
    t->plans[which] = make_plan(t, which);
    t->buckets = &t->plans[which];
    for (Bucket& b : *t->buckets) b.fired = false;
  }
  for (Bucket& b : *t->buckets)
    if (!b.fired && (rc = fire(t, b))) return rc;
  const int writes = (int)t->evlog.size();
  for (size_t i = t->overlap_log.size() >= (size_t)t->nfired ? t->overlap_log.size() - t->nfired : 0; i < t->overlap_log.size(); ++i)
    t->overlap_log[i].writes_in_backward = writes;
  // how long the COMPUTE stream stalls on communication = the part of the all-reduce backward did not hide
  if (t->measure_exposed) fold_exposed(t);   // the previous measurement: its events have completed long ago
  if (t->measure_exposed) {
    if (!t->ex0) { THIP(hipEventCreate(&t->ex0)); THIP(hipEventCreate(&t->ex1)); }
    THIP(hipEventRecord(t->ex0, t->st));
  }
  rc = t->comm.wait_all(t->comm.ctx, t->st);
  if (rc) return tfail(t, -30, "comm.wait_all failed (%d)", rc);
  if (t->measure_exposed) {
    THIP(hipEventRecord(t->ex1, t->st));
    t->ex_pending = true;
    t->ex_which = which;
  }
  t->buckets = nullptr;
  return 0;
}
// every exact-mode all-gather goes through here (batch statistics, MinibatchLayer activations / gradients): issued on the COMPUTE
// stream, whose next kernel reads the result.  measure_exposed: an event pair around it, folded a step later (fold_gathers).
int gather(ian_trainer* t, const float* src, float* dst, int64_t count, const char* what) {
  std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;
  if (t->measure_exposed) {
    auto& pool = t->gev[t->gpar];
    if (t->gev_used[t->gpar] == pool.size()) {
      hipEvent_t a, b;
      THIP(hipEventCreate(&a));
      THIP(hipEventCreate(&b));
      pool.push_back({a, b});
    }
    ev = &pool[t->gev_used[t->gpar]++];
    THIP(hipEventRecord(ev->first, t->st));
  }
  const int rc = t->comm.allgather(t->comm.ctx, src, dst, count, t->st);
  if (rc) return tfail(t, -30, "comm.allgather failed (%d) on %s", rc, what);
  if (ev) THIP(hipEventRecord(ev->second, t->st));
  return 0;
}
void fold_gathers(ian_trainer* t, int par) {   // events of pool `par` completed long ago (a whole step), or the caller synchronised
  double ms_total = 0.0;
  const size_t n = t->gev_used[par];
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(t->gev[par][i].second) == hipSuccess && hipEventElapsedTime(&ms, t->gev[par][i].first, t->gev[par][i].second) == hipSuccess)
      ms_total += ms;
  }
  (void)hipGetLastError();
  if (n) {
    const int w = t->gev_which[par];
    t->gather_ms[w] += ms_total;
    t->gather_calls[w] += (double)n;
    t->gather_n[w] += 1;
  }
  t->gev_used[par] = 0;
}

// sums (float64 [width]) <- sum over ranks, combined in RANK ORDER by the pairwise tree of ian_k_tree_sum: the result does not depend
// on the collective's internal algorithm and, for power-of-two shards, equals the single-process reduction bit for bit (SyncBN)
int allreduce_ordered(ian_trainer* t, double* sums, int width) {
  if (t->world == 1) return 0;
  const size_t need = (size_t)width * t->world;
  if (t->gbuf_cap < need) {
    double* p = dalloc64(t, need);
    if (!p) return tfail(t, -20, "out of device memory (statistics gather buffer)");
    t->gbuf = p;
    t->gbuf_cap = need;
  }
  const int rc = gather(t, reinterpret_cast<const float*>(sums), reinterpret_cast<float*>(t->gbuf), 2 * (int64_t)width, "batch statistics");
  if (rc) return rc;
  TK(ian_k_tree_sum(t->gbuf, t->world, width, sums, t->st));
  return 0;
}

int acc(ian_trainer* t, const PRef& p, const float* src, int64_t count, float alpha = 1.f) {  // grad[p] (+)= alpha * src
  TK(ian_k_axpy(alpha, src, p.g, count, t->touched[p.id] ? 1 : 0, t->st));
  return mark(t, {p.id});
}
int acc64(ian_trainer* t, const PRef& p, const double* src, int64_t count, double alpha = 1.0) {  // from float64 column sums
  TK(ian_k_axpy_f64(alpha, src, p.g, count, t->touched[p.id] ? 1 : 0, t->st));
  return mark(t, {p.id});
}
// ---- GEMM-epilogue statistics (include/ian_train.h ian_layer_stats_next) ------------------------------------------------
bool fuse_stats(const ian_trainer* t) { return t->fused_stats && !t->exact; }
int arm_fwd_stats(ian_trainer* t, LayerRef* L) {      // the layer's next forward also sums v, v*v per row tile
  if (!fuse_stats(t)) return 0;
  LCALL(L, ian_layer_stats_next, 1, nullptr, nullptr, nullptr, nullptr, 0, t->ws_stats, (int64_t)t->ws_stats_cap);
  return 0;
}
int arm_bwd_stats(ian_trainer* t, LayerRef* L, const Unit& below) {
  if (!fuse_stats(t)) return 0;   // the layer's next backward-data also sums g = dA act'(a) and g xhat of the gradient it stores
  LCALL(L, ian_layer_stats_next, 2, below.a, below.y, below.bn.mean, below.bn.inv_std, below.act, t->ws_stats, (int64_t)t->ws_stats_cap);
  return 0;
}
int armed_chunks(ian_trainer* t, LayerRef* L) { return fuse_stats(t) ? ian_layer_stats_chunks(L->l) : 0; }

// ---- the unit: linear layer + batch-norm + activation -----------------------------------------------------------------------
// exact mode, after the per-rank sums have been combined over the ranks: affine, apply, running averages (same running_math as the
// fused single-process second stage: data-parallel checkpoints carry bit-identical running averages)
int bn_forward_finish(ian_trainer* t, Unit& u, bool running) {
  BN& bn = u.bn;
  bn.count = (float)(u.rows * t->world);
  TK(ian_k_bn_make_affine(bn.sums, bn.count, BN_EPS, u.gamma.p, u.beta.p, u.C, bn.mean, bn.inv_std, bn.scale, bn.shift, t->st));
  TK(ian_k_affine(u.y, u.a, bn.scale, bn.shift, u.rows, u.C, u.stride, u.act, t->st));
  if (running && t->update_running) TK(ian_k_bn_running(u.run_mean.p, bn.mean, u.run_inv_std.p, bn.inv_std, u.C, 0.9f, 0.1f, t->st));
  return 0;
}
// a = act(bn(y)).  pre > 0: the producing GEMM already left `pre` chunk partials in the statistics workspace (arm_fwd_stats)
int bn_forward(ian_trainer* t, Unit& u, bool running, int pre) {
  BN& bn = u.bn;
  double* ws = t->ws_stats;
  int rc;
  if (pre <= 0 && (rc = ws_for(t, u.rows, u.C, &ws))) return rc;   // (pre > 0: the partials are already in the workspace -- it must not move)
  const bool upd = running && t->update_running;  // r = (1 - alpha) r + alpha * batch   (Lasagne BatchNormLayer alpha = 0.1)
  float *rm = upd ? u.run_mean.p : nullptr, *ri = upd ? u.run_inv_std.p : nullptr;
  if (!t->exact) {  // no collective between the two stages: one fused second stage
    bn.count = (float)u.rows;
    if (pre > 0)
      TK(ian_k_bn_finish(t->ws_stats, pre, u.C, bn.sums, bn.count, BN_EPS, u.gamma.p, u.beta.p, bn.mean, bn.inv_std, bn.scale, bn.shift, rm, ri, 0.9f, 0.1f,
                         t->st));
    else
      TK(ian_k_bn_stats_affine(u.y, u.rows, u.C, u.stride, ws, chunks(t, u.rows), bn.sums, bn.count, BN_EPS, u.gamma.p, u.beta.p, bn.mean, bn.inv_std,
                               bn.scale, bn.shift, rm, ri, 0.9f, 0.1f, t->st));
    TK(ian_k_affine(u.y, u.a, bn.scale, bn.shift, u.rows, u.C, u.stride, u.act, t->st));
    return 0;
  }
  TK(ian_k_colstats(0, u.y, nullptr, nullptr, nullptr, nullptr, u.rows, u.C, u.stride, 0, ws, chunks(t, u.rows), bn.sums, t->st));
  if ((rc = allreduce_ordered(t, bn.sums, 2 * u.C))) return rc;
  return bn_forward_finish(t, u, running);
}
int unit_forward(ian_trainer* t, Unit& u, const float* x, bool running, const float* res = nullptr) {  // y = L(x) (+ res); a = act(bn(y))
  int rc;
  if (u.epilogue && (rc = arm_fwd_stats(t, u.L))) return rc;
  LCALL(u.L, ian_layer_forward, x, t->n, u.y, u.ld, nullptr, res, 0, t->st);
  return bn_forward(t, u, running, u.epilogue ? armed_chunks(t, u.L) : 0);
}

const float* act_input(const Unit& u) { return u.act ? u.a : nullptr; }   // what act' is evaluated on (no activation: nothing)
// exact mode, after the gradient statistics have been combined over the ranks
int bn_backward_finish(ian_trainer* t, Unit& u, bool want_w) {
  BN& bn = u.bn;
  int rc;
  if (want_w) {
    // with exact statistics every rank already holds the GLOBAL dbeta / dgamma: pre-divide so that the gradient all-reduce
    // (a sum over ranks) restores them
    const double sc = 1.0 / t->world;
    if ((rc = acc64(t, u.beta, bn.bsums, u.C, sc))) return rc;
    if ((rc = acc64(t, u.gamma, bn.bsums + u.C, u.C, sc))) return rc;
  }
  TK(ian_k_bn_bwd(u.dA, act_input(u), u.y, bn.mean, bn.inv_std, bn.scale, bn.bsums, bn.count, u.dy, u.rows, u.C, u.stride, u.act, t->st));
  return 0;
}
// dy = d loss / dy from dA; want_w: dbeta, dgamma.  pre > 0: partials from the GEMM that stored dA (arm_bwd_stats)
int bn_backward(ian_trainer* t, Unit& u, bool want_w, int pre) {
  BN& bn = u.bn;
  const float* a = act_input(u);
  double* ws = t->ws_stats;
  int rc;
  if (pre <= 0 && (rc = ws_for(t, u.rows, u.C, &ws))) return rc;
  if (!t->exact) {
    float *gb = nullptr, *gg = nullptr;
    int ab = 0, ag = 0;
    if (want_w) {
      gb = u.beta.g; gg = u.gamma.g;
      ab = t->touched[u.beta.id] ? 1 : 0; ag = t->touched[u.gamma.id] ? 1 : 0;
    }
    if (pre > 0) TK(ian_k_bn_bwd_finish(t->ws_stats, pre, u.C, bn.bsums, gb, ab, gg, ag, t->st));
    else TK(ian_k_bn_bwd_stats(u.dA, a, u.y, bn.mean, bn.inv_std, u.rows, u.C, u.stride, u.act, ws, chunks(t, u.rows), bn.bsums, gb, ab, gg, ag, t->st));
    if (want_w && (rc = mark(t, {u.beta.id, u.gamma.id}))) return rc;
    TK(ian_k_bn_bwd(u.dA, a, u.y, bn.mean, bn.inv_std, bn.scale, bn.bsums, bn.count, u.dy, u.rows, u.C, u.stride, u.act, t->st));
    return 0;
  }
  TK(ian_k_colstats(1, u.dA, a, u.y, bn.mean, bn.inv_std, u.rows, u.C, u.stride, u.act, ws, chunks(t, u.rows), bn.bsums, t->st));
  if ((rc = allreduce_ordered(t, bn.bsums, 2 * u.C))) return rc;
  return bn_backward_finish(t, u, want_w);
}
// The weight-gradient stream.  wgrad_priority = 1: created with the LOWEST stream priority the device offers, so that the dispatcher
// prefers the compute stream's workgroups whenever both streams have some ready: a data-path GEMM then keeps the whole chip, and
// the weight-gradient GEMMs -- which nothing downstream reads before the optimiser -- queue up and fill the chip while the
// compute stream runs its HBM-bound element-wise passes (batch-statistics sums, batch-norm backward, head gathers) instead of
// being consumed earlier at half rate next to a data-path GEMM (profiles/r05_train_ian_b128.md: the second stream was busy 82 of
// the 200 ms four updates span, the matrix pipe idle during most element-wise passes).  Same launches, same operands, same
// stream-order dependencies: bitwise the unprioritised step.
int make_wgrad_stream(ian_trainer* t) {
  if (t->st2) {
    (void)hipStreamSynchronize(t->st2);
    (void)hipStreamDestroy(t->st2);
    t->st2 = nullptr;
  }
  hipError_t e;
  if (t->wgrad_priority) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);      // numerically: least >= greatest (lower number = higher priority)
    e = hipStreamCreateWithPriority(&t->st2, hipStreamNonBlocking, least);
  } else {
    e = hipStreamCreateWithFlags(&t->st2, hipStreamNonBlocking);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    t->st2 = nullptr;
    return 1;
  }
  return 0;
}
int side_stream(ian_trainer* t, hipStream_t* out) {  // the stream a weight-gradient launch goes to, ordered behind what is on t->st now
  *out = t->st;
  if (!t->overlap_wgrad || !t->st2) return 0;
  hipEvent_t e;
  int rc;
  if ((rc = next_event(t, &e))) return rc;
  THIP(hipEventRecord(e, t->st));
  THIP(hipStreamWaitEvent(t->st2, e, 0));
  *out = t->st2;
  return 0;
}
int join_side_stream(ian_trainer* t) {  // the compute stream waits for every weight gradient issued so far
  if (!t->overlap_wgrad || !t->st2 || !t->ev_used) return 0;
  hipEvent_t e;
  int rc;
  if ((rc = next_event(t, &e))) return rc;
  THIP(hipEventRecord(e, t->st2));
  THIP(hipStreamWaitEvent(t->st, e, 0));
  t->ev_used = 0;
  return 0;
}
int wgrad(ian_trainer* t, LayerRef* r, const float* x, const float* dy) {
  hipStream_t ws;
  int rc_ = side_stream(t, &ws);
  if (rc_) return rc_;
  LCALL(r, ian_layer_backward_weight, x, dy, t->n, r->grads.data(), (int)r->grads.size(), t->touched[r->ids[0]] ? 1 : 0, ws);
  return mark(t, r->ids);
}
// the layer of a unit, from u.dy: weight gradients (want_w; x = the layer's input), then dx (+)= dy (*) W^T (dx null: not needed).
// `below`: the unit whose dA this writes -- with fused_stats the statistics of its batch-norm backward ride on the launch; pre: their chunk count
int layer_backward(ian_trainer* t, Unit& u, const float* x, bool want_w, int& pre, float* dx, int accumulate, Unit* below) {
  int rc;
  pre = 0;
  if (want_w && (rc = wgrad(t, u.L, x, u.dy))) return rc;
  if (!dx) return 0;
  const bool ride = below && u.epilogue;
  if (ride && (rc = arm_bwd_stats(t, u.L, *below))) return rc;
  LCALL(u.L, ian_layer_backward_data, u.dy, t->n, dx, below ? below->ld : 0, accumulate, t->st);
  if (ride) pre = armed_chunks(t, u.L);
  return 0;
}
// backward of the whole unit from u.dA.  pre: in, chunk partials the launch that stored u.dA left (0: none); out, the same for `below`.
// dskip: gradient of a second reader of y (the residual edge of an MD block), added to dy before the layer's backward
int unit_backward(ian_trainer* t, Unit& u, const float* x, bool want_w, int& pre, float* dx, int accumulate, Unit* below, const float* dskip = nullptr) {
  int rc;
  if ((rc = bn_backward(t, u, want_w, pre))) return rc;
  if (dskip) TK(ian_k_axpy(1.f, dskip, u.dy, u.rows * u.C, 1, t->st));
  return layer_backward(t, u, x, want_w, pre, dx, accumulate, below);
}
// R, G_a, B_a from their three seeds -> D.u4.dA; *pre: chunk partials for bnorm_dc4's backward, which ride on the GEMM that stores it
int head_backward(ian_trainer* t, DecPass& D, bool want_w, int* pre) {
  *pre = 0;
  LayerRef* hl[3] = {t->L.R, t->L.G_a, t->L.B_a};
  const float *x = D.u4.a, *dys[3] = {D.gR, D.gG, D.gB};
  float* dx = D.u4.dA;
  bool accs[3];
  for (int i = 0; i < 3; ++i) accs[i] = t->touched[hl[i]->ids[0]] != 0;
  if (t->head6 && accs[0] == accs[1] && accs[1] == accs[2]) {
    int rc = arm_bwd_stats(t, hl[0], D.u4);
    if (rc) return rc;
    rc = ian_layer_head6_backward(hl[0]->l, hl[1]->l, hl[2]->l, x, dys[0], dys[1], dys[2], t->n, 32, dx, 128, 0, want_w ? hl[0]->grads.data() : nullptr,
                                  want_w ? hl[1]->grads.data() : nullptr, want_w ? hl[2]->grads.data() : nullptr,
                                  want_w ? (int)hl[0]->grads.size() : 0, accs[0] ? 1 : 0, t->st);
    if (rc == 0) {
      *pre = armed_chunks(t, hl[0]);
      if (want_w)
        for (int i = 0; i < 3; ++i) {
          const int mrc = mark(t, hl[i]->ids);
          if (mrc) return mrc;
        }
      return 0;
    }
    (void)ian_layer_stats_next(hl[0]->l, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0);   // the per-layer fallback accumulates dx in three launches
    if (rc != -4) return tfail(t, rc, "ian_layer_head6_backward failed (%d): %s", rc, ian_layer_last_error(hl[0]->l));
  }
  for (int i = 0; i < 3; ++i) {
    int rc;
    if (want_w && (rc = wgrad(t, hl[i], x, dys[i]))) return rc;
    LCALL(hl[i], ian_layer_backward_data, dys[i], t->n, dx, 0, i > 0 ? 1 : 0, t->st);
  }
  return 0;
}

// ---- encoder pass (IAN.py:71-110 + discriminator head :209-216), training mode ------------------------------------------
int enc_forward(ian_trainer* t, EncPass& E, const float* x_nchw, int t0, int t1, int acc_target, bool running) {
  const int n = t->n;
  int rc;
  TK(ian_k_nchw_to_nhwc(x_nchw, E.x, n, 4096, 3, 32, t->st));
  LCALL(t->L.enc_conv[1], ian_layer_forward, E.x, n, E.a[1], 0, t->pr.enc_conv1_b.p, nullptr, IAN_ACT_LRELU, t->st);   // bias, no batch-norm (:71-80)
  for (int i = 2; i <= 4; ++i)
    if ((rc = unit_forward(t, E.u[i], E.a[i - 1], running))) return rc;
  TK(ian_k_globalpool(E.a[4], E.feat, n, 16, 1024, 1024, 1024, t->st));
  LCALL(t->L.mb, ian_layer_forward, E.feat, n, E.act, cs(2500), nullptr, nullptr, 0, t->st);
  const float* act_all = E.act;
  int nall = n, row0 = 0;
  if (t->exact) {  // the kernel features couple every sample with every other one of the GLOBAL minibatch (layers.py:506-520)
    if ((rc = gather(t, E.act, E.act_all, (int64_t)n * cs(2500), "the MinibatchLayer activations"))) return rc;
    act_all = E.act_all; nall = t->N; row0 = t->rank * n;
  }
  TK(ian_k_mb_forward(act_all, nall, cs(2500), row0, n, 500, 5, t->pr.mb_b.p, E.feat, 1024, 1024, E.mb, cs(1524), t->st));
  TK(ian_k_disc_head(E.mb, cs(1524), 1524, t->pr.discrimi_W.p, n, t0, t1, acc_target, E.p, E.loss, t->st));
  return 0;
}
// ce = (target0, w0, target1, w1): dlogits = sum w_t (p - onehot(target_t)).  feature_seeded: da1..da4 already hold the
// feature-loss seeds (train_IAN.py:244).  want_w: accumulate encoder_params gradients.
int enc_backward(ian_trainer* t, EncPass& E, int t0, float w0, int t1, float w1, bool feature_seeded, bool want_w, bool want_dx) {
  const int n = t->n;
  const auto& pr = t->pr;
  int rc;
  TK(ian_k_disc_head_bwd(E.p, pr.discrimi_W.p, 1524, n, t0, w0, t1, w1, E.dlogits, E.dmb, cs(1524), t->st));
  if (want_w) {
    TK(ian_k_disc_head_wgrad(E.mb, cs(1524), 1524, n, E.dlogits, pr.discrimi_W.g, t->touched[pr.discrimi_W.id] ? 1 : 0, t->st));
    if ((rc = mark(t, {pr.discrimi_W.id}))) return rc;
    // db[k] = sum_b df[b,k] : column sums of dmb[:, 1024:1524]
    TK(ian_k_colstats(2, E.dmb + 1024, nullptr, nullptr, nullptr, nullptr, n, 500, cs(1524), 0, t->ws_stats, n < 256 ? n : 256, t->tmp_vals, t->st));
    if ((rc = acc64(t, pr.mb_b, t->tmp_vals, 500))) return rc;
  }
  {
    const float *act_all = E.act, *dmb_all = E.dmb;
    int nall = n, row0 = 0;
    if (t->exact) {  // a sample's activations feed every other sample's kernel features: their gradients come from all ranks
      if ((rc = gather(t, E.dmb, E.dmb_all, (int64_t)n * cs(1524), "the MinibatchLayer gradients"))) return rc;
      act_all = E.act_all; dmb_all = E.dmb_all; nall = t->N; row0 = t->rank * n;
    }
    TK(ian_k_mb_backward(act_all, nall, cs(2500), row0, n, 500, 5, dmb_all + 1024, cs(1524), E.dact, cs(2500), t->st));
  }
  TK(ian_k_grad_pass(E.dmb, cs(1524), 0, E.dfeat, nullptr, 1024, n, 1024, 0, 0, t->st));  // direct path of the concat (layers.py:524)
  LCALL(t->L.mb, ian_layer_backward_data, E.dact, n, E.dfeat, 1024, 1, t->st);
  if (want_w) {
    float* dW = t->mb_dW;
    LCALL(t->L.mb, ian_layer_backward_weight, E.feat, E.dact, n, &dW, 1, 0, t->st);
    TK(ian_k_mb_weight_bwd(pr.mb_theta.p, t->mb_colscale, t->mb_dW, pr.mb_theta.g, pr.mb_lws.g, 1024, 2500, t->touched[pr.mb_theta.id] ? 1 : 0, t->st));
    if ((rc = mark(t, {pr.mb_theta.id, pr.mb_lws.id}))) return rc;
  }
  TK(ian_k_globalpool_bwd(E.dfeat, E.da[4], n, 16, 1024, 1024, 1024, feature_seeded ? 1 : 0, t->st));
  int pre = 0;   // chunk partials the previous backward-data GEMM left for the next batch-norm backward (0: run colstats)
  for (int i = 4; i >= 2; --i)   // the gradient enc_conv<i> stores is the input of the next normalisation down (bnorm<i-1>); enc_conv1 has none
    if ((rc = unit_backward(t, E.u[i], E.a[i - 1], want_w, pre, E.da[i - 1], feature_seeded ? 1 : 0, i > 2 ? &E.u[i - 1] : nullptr))) return rc;
  // enc_conv1: bias + lrelu, no batch-norm (IAN.py:71-80)
  if (want_w) {
    TK(ian_k_colstats(2, E.da[1], E.a[1], nullptr, nullptr, nullptr, (int64_t)n * 1024, 128, 128, IAN_ACT_LRELU, t->ws_stats, 256, t->tmp_vals, t->st));
    if ((rc = acc64(t, pr.enc_conv1_b, t->tmp_vals, 128))) return rc;
  }
  TK(ian_k_bn_bwd(E.da[1], E.a[1], nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, E.da[1], (int64_t)n * 1024, 128, 128, IAN_ACT_LRELU, t->st));
  if (want_w && (rc = wgrad(t, t->L.enc_conv[1], E.x, E.da[1]))) return rc;
  if (want_dx) LCALL(t->L.enc_conv[1], ian_layer_backward_data, E.da[1], n, E.dx, 0, 0, t->st);
  return 0;
}

// ---- latent path (IAN.py:114-128): enc_fc1 -> (mu, logsigma) -> z0 = mu + e^ls * eps -> IAF ------------------------------
int z_forward(ian_trainer* t, const float* a4, const float* eps) {
  const int n = t->n, Z = t->cfg.num_latents;
  ZPass& S = t->ZS;
  int rc;
  if ((rc = unit_forward(t, S.fc1, a4, true))) return rc;
  if (!t->exact) {
    for (Unit* u : {&S.mu, &S.ls})
      if ((rc = unit_forward(t, *u, S.fc1.a, true))) return rc;
  } else {  // both layers, both per-rank statistics, ONE all-gather of the adjacent sums, then both normalisations
    double* ws;
    if ((rc = ws_for(t, n, Z, &ws))) return rc;
    for (Unit* u : {&S.mu, &S.ls}) {
      LCALL(u->L, ian_layer_forward, S.fc1.a, n, u->y, u->ld, nullptr, nullptr, 0, t->st);
      TK(ian_k_colstats(0, u->y, nullptr, nullptr, nullptr, nullptr, n, Z, u->stride, 0, ws, chunks(t, n), u->bn.sums, t->st));
    }
    if ((rc = allreduce_ordered(t, S.mu.bn.sums, 4 * Z))) return rc;
    for (Unit* u : {&S.mu, &S.ls})
      if ((rc = bn_forward_finish(t, *u, true))) return rc;
  }
  TK(ian_k_sample(S.mu.a, S.ls.a, eps, S.z0, S.kl, n, Z, 128, Z, t->st));
  TK(ian_k_made_iaf(S.z0, S.z, t->made_w, t->made_b, n, Z, 128, t->st));
  return 0;
}
// dz = dL/dz (from the decoder) -> gradients of Z_params, including KL and (later) the L2 penalty
int z_backward(ian_trainer* t, const float* dz, const float* a4) {
  const int n = t->n, Z = t->cfg.num_latents;
  ZPass& S = t->ZS;
  int rc, pre = 0;
  TK(ian_k_made_iaf_bwd(S.z0, dz, S.dz0, t->made_w, t->made_b, n, Z, 128, t->st));
  const float klw = 1.f / ((float)t->N * 100.f);  // d(-0.5*mean(...)) over the GLOBAL batch: factor folded in the kernel's formula
  TK(ian_k_sample_bwd(S.mu.a, S.ls.a, t->eps, S.dz0, S.mu.dA, S.ls.dA, n, Z, 128, Z, klw, t->st));
  if (t->exact) {  // both gradient statistics, ONE all-gather (the sums are adjacent: z_alloc)
    double* ws;
    if ((rc = ws_for(t, n, Z, &ws))) return rc;
    for (Unit* u : {&S.mu, &S.ls})
      TK(ian_k_colstats(1, u->dA, nullptr, u->y, u->bn.mean, u->bn.inv_std, n, Z, u->stride, 0, ws, chunks(t, n), u->bn.bsums, t->st));
    if ((rc = allreduce_ordered(t, S.mu.bn.bsums, 4 * Z))) return rc;
  }
  for (Unit* u : {&S.mu, &S.ls}) {   // both write df = S.fc1.dA: the second accumulates
    if ((rc = t->exact ? bn_backward_finish(t, *u, true) : bn_backward(t, *u, true, 0))) return rc;
    if ((rc = layer_backward(t, *u, S.fc1.a, true, pre, S.fc1.dA, u == &S.ls ? 1 : 0, &S.fc1))) return rc;
  }
  return unit_backward(t, S.fc1, a4, true, pre, nullptr, 0, nullptr);   // the encoder is not trained through the latent path
}

// ---- decoder pass (IAN.py:129-207), training mode -----------------------------------------------------------------------
int dec_forward(ian_trainer* t, DecPass& D, const float* zbuf, bool running) {
  const int n = t->n;
  int rc;
  LCALL(t->L.l_dec_fc2, ian_layer_forward, zbuf, n, D.h0, 8192, t->fc2_bias, nullptr, IAN_ACT_LRELU, t->st);
  const float* h = D.h0;
  for (auto& u : D.stage) {   // IAN.py:139-171: x = deconv(h), then the MD block h = lrelu(bn2(x + MDCL2(lrelu(bn1(MDCL(lrelu(bn0(x))))))))
    if ((rc = unit_forward(t, u[0], h, running))) return rc;
    if ((rc = unit_forward(t, u[1], u[0].a, running))) return rc;
    if ((rc = unit_forward(t, u[2], u[1].a, running, u[0].y))) return rc;  // ElemwiseSum (layers.py:415)
    h = u[2].a;
  }
  if ((rc = unit_forward(t, D.u4, h, running))) return rc;
  const int64_t rows = (int64_t)n * 4096;
  const float* h4 = D.u4.a;
  const int sg = IAN_ACT_SIGMOID;
  const Layers& L = t->L;
  // R = sigmoid(MDCL(h4)), G_a, B_a (IAN.py:183-199): the three layers that read the 128-channel map, one pass over it
  int h6 = -4;
  if (t->head6) h6 = ian_layer_head6_forward(L.R->l, L.G_a->l, L.B_a->l, h4, n, D.R, D.Ga, D.Ba, 32, sg, 0, 0, t->st);
  if (h6 == -4) {
    LCALL(L.R, ian_layer_forward, h4, n, D.R, 0, nullptr, nullptr, sg, t->st);  // IAN.py:183-186
    LCALL(L.G_a, ian_layer_forward, h4, n, D.Ga, 0, nullptr, nullptr, 0, t->st);
    LCALL(L.B_a, ian_layer_forward, h4, n, D.Ba, 0, nullptr, nullptr, 0, t->st);
  } else if (h6) {
    return tfail(t, h6, "ian_layer_head6_forward failed (%d): %s", h6, ian_layer_last_error(L.R->l));
  }
  LCALL(L.G_b, ian_layer_forward, D.R, n, D.G, 0, nullptr, D.Ga, sg, t->st);   // :187-196
  TK(ian_k_concat2(D.R, 2, 32, D.G, 2, 32, D.RG, 32, rows, t->st));            // :201
  LCALL(L.B_b, ian_layer_forward, D.RG, n, D.B, 0, nullptr, D.Ba, sg, t->st);  // :197-206
  TK(ian_k_beta(D.R, D.G, D.B, D.xhat, n, 4096, 32, t->st));                   // :207
  return 0;
}
// D.dxhat (NCHW) -> gradients of decoder_params (want_w) and D.dz (want_dz)
int dec_backward(ian_trainer* t, DecPass& D, const float* zbuf, bool want_w, bool want_dz) {
  const int n = t->n;
  const int64_t rows = (int64_t)n * 4096;
  const int sg = IAN_ACT_SIGMOID;
  const Layers& L = t->L;
  int rc;
  TK(ian_k_beta_bwd(D.dxhat, D.R, D.G, D.B, D.gR, D.gG, D.gB, n, 4096, 32, sg, t->st));
  // B = sigmoid(B_a(h4) + B_b([R,G]))
  if (want_w && (rc = wgrad(t, L.B_b, D.RG, D.gB))) return rc;
  LCALL(L.B_b, ian_layer_backward_data, D.gB, n, D.dRG, 0, 0, t->st);
  TK(ian_k_grad_pass(D.dRG, 32, 0, D.gR, D.R, 32, rows, 2, sg, 1, t->st));
  TK(ian_k_grad_pass(D.dRG, 32, 2, D.gG, D.G, 32, rows, 2, sg, 1, t->st));
  // G = sigmoid(G_a(h4) + G_b(R))
  if (want_w && (rc = wgrad(t, L.G_b, D.R, D.gG))) return rc;
  LCALL(L.G_b, ian_layer_backward_data, D.gG, n, D.dRt, 0, 0, t->st);
  TK(ian_k_grad_pass(D.dRt, 32, 0, D.gR, D.R, 32, rows, 2, sg, 1, t->st));
  // R = sigmoid(R(h4)): all three seeds are final here
  int pre = 0;   // chunk partials the GEMM that stored a gradient left for the batch-norm backward that consumes it (0: colstats)
  if ((rc = head_backward(t, D, want_w, &pre))) return rc;
  // dec_conv4 + bnorm_dc4 + lrelu: its gradient enters the last stage's bnorm2 backward
  Unit* top = &D.stage[2][2];
  if ((rc = unit_backward(t, D.u4, top->a, want_w, pre, top->dA, 0, top))) return rc;
  for (int si = 2; si >= 0; --si) {
    Unit* u = D.stage[si];
    Unit* prev = si > 0 ? &D.stage[si - 1][2] : nullptr;   // the previous stage's output unit (stage 0 reads h0 = l_dec_fc2's output)
    // h = lrelu(bn2(x + d)),  d = MDCL2(c),  c = lrelu(bn1(MDCL(a))),  a = lrelu(bn0(x)),  x = deconv(previous h)
    if ((rc = unit_backward(t, u[2], u[1].a, want_w, pre, u[1].dA, 0, &u[1]))) return rc;
    if ((rc = unit_backward(t, u[1], u[0].a, want_w, pre, u[0].dA, 0, &u[0]))) return rc;
    if ((rc = unit_backward(t, u[0], prev ? prev->a : D.h0, want_w, pre, prev ? prev->dA : D.dh0, 0, prev, u[2].dy))) return rc;  // residual edge: dx += d(x+d)
  }
  // l_dec_fc2: bias + lrelu
  TK(ian_k_bn_bwd(D.dh0, D.h0, nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, D.dh0, n, 8192, 8192, IAN_ACT_LRELU, t->st));
  if (want_w) {
    if ((rc = wgrad(t, L.l_dec_fc2, zbuf, D.dh0))) return rc;
    TK(ian_k_colstats(2, D.dh0, nullptr, nullptr, nullptr, nullptr, n, 8192, 8192, 0, t->ws_stats, n < 256 ? n : 256, t->tmp_big, t->st));
    TK(ian_k_axpy_f64(1.0, t->tmp_big, t->fc2_tmp, 8192, 0, t->st));   // float64 column sums -> float32, (H,W,C) order
    TK(ian_k_gather(t->fc2_tmp, t->fc2_inv, t->fc2_db, 8192, t->st));
    if ((rc = acc(t, t->pr.l_dec_fc2_b, t->fc2_db, 8192))) return rc;
  }
  if (want_dz) LCALL(L.l_dec_fc2, ian_layer_backward_data, D.dh0, n, D.dz, 128, 0, t->st);
  return 0;
}

// ---- timing-only two-chain experiment (see ian_trainer::dual_timing): all three are inert unless dual_timing is set ----------------
int chain_fork(ian_trainer* t) {   // stream B starts behind everything issued to the compute stream so far
  if (!t->dual_timing) return 0;
  if (!t->stB) THIP(hipStreamCreateWithFlags(&t->stB, hipStreamNonBlocking));
  hipEvent_t e;
  THIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  THIP(hipEventRecord(e, t->st));
  THIP(hipStreamWaitEvent(t->stB, e, 0));
  THIP(hipEventDestroy(e));
  return 0;
}
int chain_join(ian_trainer* t) {   // the compute stream waits for stream B
  if (!t->dual_timing) return 0;
  hipEvent_t e;
  THIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  THIP(hipEventRecord(e, t->stB));
  THIP(hipStreamWaitEvent(t->st, e, 0));
  THIP(hipEventDestroy(e));
  return 0;
}
struct OnStreamB {                 // everything issued while this object lives goes to stream B
  ian_trainer* t;
  hipStream_t keep;
  explicit OnStreamB(ian_trainer* tt) : t(tt), keep(tt->st) { if (t->dual_timing) t->st = t->stB; }
  ~OnStreamB() { t->st = keep; }
};

// ---- the step -----------------------------------------------------------------------------------------------------------
// TIMING ONLY with dual_timing: the (Z_rand -> decoder -> encoder) chain concurrently on stream B, workspaces shared without protection
int forward(ian_trainer* t, const float* X, const float* Zr, const float* eps) {  // the three passes of train_IAN.py:116-149
  const int n = t->n, Z = t->cfg.num_latents;
  int rc;
  if (t->measure_exposed && t->world > 1) {   // this step's all-gather events go to the pool of two steps ago: fold it first
    t->gpar ^= 1;
    fold_gathers(t, t->gpar);
  }
  if ((rc = refresh_weights(t))) return rc;
  t->X = X;
  t->eps = eps;
  if ((rc = chain_fork(t))) return rc;
  if ((rc = enc_forward(t, t->EX, X, 0, -1, 0, true))) return rc;           // p_X vs p1
  if ((rc = z_forward(t, t->EX.a[4], eps))) return rc;
  if ((rc = dec_forward(t, t->DZ, t->ZS.z, true))) return rc;               // X_hat
  if ((rc = enc_forward(t, t->EH, t->xhat_override ? t->xhat_override : t->DZ.xhat, 0, 1, 1, false))) return rc;  // p_X_hat
  {
    OnStreamB b(t);
    TK(ian_k_grad_pass(Zr, Z, 0, t->zgen0, nullptr, 128, n, Z, 0, 0, t->st));       // (n,100) -> padded rows
    TK(ian_k_made_iaf(t->zgen0, t->zgen, t->made_w, t->made_b, n, Z, 128, t->st));  // {l_Z_IAF: Z} (train_IAN.py:149)
    if ((rc = dec_forward(t, t->DG, t->zgen, false))) return rc;            // X_gen
    if ((rc = enc_forward(t, t->EG, t->xgen_override ? t->xgen_override : t->DG.xhat, 0, 2, 2, false))) return rc;  // p_X_gen
  }
  return chain_join(t);
}

// all scalar losses of train_IAN.py:169-250,279: partial sums on the device (+ their all-reduce: issued on EVERY data-parallel step,
// with or without a reader, so that ranks that disagree on `metrics` keep identical collective sequences), then one device->host copy
int metrics_device(ian_trainer* t) {
  const int n = t->n;
  const float N = (float)t->N;   // means are over the GLOBAL batch
  float* s = t->scalars;
  THIP(hipMemsetAsync(s, 0, 64 * sizeof(float), t->st));
  TK(ian_k_sum_rows(t->EX.loss, n, 4, 1.f / N, s + 0, t->st));   // [0] discrim_d_loss, [2] acc(p_X)
  TK(ian_k_sum_rows(t->EH.loss, n, 4, 1.f / N, s + 4, t->st));   // [4] gen_recon_loss, [5] CE(p_X_hat,p2), [6] acc
  TK(ian_k_sum_rows(t->EG.loss, n, 4, 1.f / N, s + 8, t->st));   // [8] gen_sample_loss, [9] CE(p_X_gen,p3), [10] acc
  TK(ian_k_sum_rows(t->ZS.kl, n * 100, 1, -0.5f / (N * 100.f), s + 12, t->st));
  TK(ian_k_pair_loss(t->DZ.xhat, t->X, nullptr, (int64_t)n * 3 * 4096, 1, 1, 0, 0.f, 0, t->ws_loss, 1024, 1.f / (N * 3.f * 4096.f), s + 16, t->st));
  for (int i = 1; i <= 4; ++i) {
    const float cnt = (float)((64 >> i) * (64 >> i) * ENC_WIDTHS[i - 1]);
    TK(ian_k_pair_loss(t->EH.a[i], t->EX.a[i], nullptr, (int64_t)n * (int64_t)cnt, 1, 1, 1, 0.f, 0, t->ws_loss, 1024, 1.f / (N * cnt * 4.f), s + 18 + 2 * i, t->st));
  }
  if (t->world > 1) {  // per-rank partial means add up to the global ones
    int rc = t->comm.allreduce_sum(t->comm.ctx, s, 64, t->st);
    if (!rc) rc = t->comm.wait_all(t->comm.ctx, t->st);
    if (rc) return tfail(t, -30, "comm all-reduce of the metrics failed (%d)", rc);
  }
  return 0;
}
int metrics_read(ian_trainer* t, float* out9) {
  float* s = t->scalars;
  float v[32];
  THIP(hipMemcpyAsync(v, s, sizeof v, hipMemcpyDeviceToHost, t->st));
  THIP(hipStreamSynchronize(t->st));
  out9[0] = v[0];                             // discrim_d_loss
  out9[1] = v[4];                             // gen_recon_loss
  out9[2] = v[8];                             // gen_sample_loss
  out9[3] = v[5] + v[9];                      // discrim_g_loss
  out9[4] = (v[2] + v[6] + v[10]) / 3.f;      // discrim_acc
  out9[5] = v[12];                            // kl_div
  out9[6] = v[16];                            // pixel_loss
  out9[7] = 1.f - v[17];                      // pixel_acc
  out9[8] = v[20] + v[22] + v[24] + v[26];    // feature_loss
  return 0;
}
int metrics(ian_trainer* t, float* out9) {
  const int rc = metrics_device(t);
  return rc ? rc : metrics_read(t, out9);
}

int backward(ian_trainer* t, bool gen) {  // gradients of the update rules of train_IAN.py:253-273 (Z_params always)
  const int n = t->n;
  const float N = (float)t->N;   // loss means are over the GLOBAL batch: summing per-rank gradients gives the 1-GPU gradient
  const ian_train_config& c = t->cfg;
  int rc;
  if ((rc = begin_backward(t, gen ? 0 : 1))) return rc;
  // ---- shared generator-side loss S = adv_gen + recon_weight*pixel + feature_weight*feature ---------------------------------
  for (int i = 1; i <= 4; ++i) {  // feature_loss seeds (train_IAN.py:244)
    const float cnt = (float)((64 >> i) * (64 >> i) * ENC_WIDTHS[i - 1]);
    TK(ian_k_pair_loss(t->EH.a[i], t->EX.a[i], t->EH.da[i], (int64_t)n * (int64_t)cnt, 1, 1, 1, c.feature_weight / (4.f * N * cnt), 0, t->ws_loss, 1024, 0.f,
                       t->scalars + 40, t->st));
  }
  if ((rc = enc_backward(t, t->EH, 0, c.agr_weight / N, -1, 0.f, true, false, true))) return rc;  // gen_recon_loss (:247)
  TK(ian_k_pair_loss(t->DZ.xhat, t->X, t->DZ.dxhat, (int64_t)n * 3 * 4096, 1, 1, 0, c.recon_weight / (N * 3.f * 4096.f), 0, t->ws_loss, 1024, 0.f,
                     t->scalars + 40, t->st));  // pixel_loss (:169)
  TK(ian_k_nhwc_to_nchw(t->EH.dx, 32, t->DZ.tmp_img, n, 4096, 3, t->st));
  TK(ian_k_axpy(1.f, t->DZ.tmp_img, t->DZ.dxhat, (int64_t)n * 3 * 4096, 1, t->st));
  if ((rc = chain_fork(t))) return rc;   // TIMING ONLY with dual_timing (see forward): the X_gen chain's sweeps run on stream B
  if ((rc = dec_backward(t, t->DZ, t->ZS.z, gen, true))) return rc;
  if ((rc = z_backward(t, t->DZ.dz, t->EX.a[4]))) return rc;
  if (gen) {
    OnStreamB b(t);
    if ((rc = enc_backward(t, t->EG, 0, c.ags_weight / N, -1, 0.f, false, false, true))) return rc;  // gen_sample_loss (:248)
    TK(ian_k_nhwc_to_nchw(t->EG.dx, 32, t->DG.dxhat, n, 4096, 3, t->st));
    if ((rc = dec_backward(t, t->DG, t->zgen, true, false))) return rc;
  } else {
    // ---- discriminator loss, X_hat and X_gen constant (consider_constant, train_IAN.py:253) ----------------------------------
    if ((rc = enc_backward(t, t->EX, 0, c.dd_weight / N, -1, 0.f, false, true, false))) return rc;  // discrim_d_loss (:234)
    if ((rc = enc_backward(t, t->EH, 1, c.dg_weight / N, -1, 0.f, false, true, false))) return rc;  // p_X_hat vs p2 (:228)
    OnStreamB b(t);
    if ((rc = enc_backward(t, t->EG, 2, c.dg_weight / N, -1, 0.f, false, true, false))) return rc;  // p_X_gen vs p3
  }
  return chain_join(t);
}

int regularizers(ian_trainer* t, bool gen) {  // train_IAN.py:211-221: L2 on the Z parameters, orthogonal penalty on the 4-D weights
  const ian_train_config& c = t->cfg;
  const Group& zp = t->grp[G_Z];
  for (int id : zp.params) {
    const Param& q = t->params[id];
    if (q.name.size() >= 5 && q.name.compare(q.name.size() - 5, 5, ".beta") == 0) continue;
    TK(ian_k_axpy(2.f * c.reg, zp.p + q.off, zp.g + q.off, q.shape.numel(), 1, t->st));
  }
  if (c.ortho < 0.f) return 0;
  const Group& grp = t->grp[gen ? G_DEC : G_ENC];
  for (int id : grp.params) {
    const Param& q = t->params[id];
    const Shape& s = q.shape;
    if (q.name.back() == 'W' && s.d.size() == 4)
      TK(ian_k_ortho(grp.p + q.off, grp.g + q.off, (int)s.d[0], (int)s.d[1], (int)s.d[2], c.ortho, t->ortho_vals, t->st));
  }
  return 0;
}

int adam(ian_trainer* t, int group) {  // lasagne.updates.adam (App. B.7): one (t, m, v) per group
  Group& g = t->grp[group];
  g.t += 1;
  const double b1 = t->cfg.beta1, b2 = 0.999;
  const double a_t = t->cfg.learning_rate * sqrt(1.0 - pow(b2, g.t)) / (1.0 - pow(b1, g.t));
  TK(ian_k_adam(g.p, g.g, g.m, g.v, g.numel, (float)a_t, (float)b1, (float)b2, 1e-8f, t->st));
  t->dirty[group] = true;
  return 0;
}
int adam_both(ian_trainer* t, bool gen) {  // update_gen: decoder_params, update_discrim: encoder_params; Z_params in both (train_IAN.py:274-276)
  const int rc = adam(t, gen ? G_DEC : G_ENC);
  return rc ? rc : adam(t, G_Z);
}

bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace

extern "C" {

int ian_trainer_create(const ian_train_config* cfg, ian_trainer** out) {
  if (!cfg || !out || cfg->batch <= 0 || cfg->num_latents != 100) return -1;  // the wired graph is IAN.py's: 100 latents
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return -10;  // no HIP device: libian has no CPU fallback
  }
  ian_trainer* t = new ian_trainer();
  t->cfg = *cfg;
  t->n = cfg->batch;
  t->N = cfg->batch;
  memset(&t->comm, 0, sizeof t->comm);
  declare_parameters(t);
  *out = t;
  return 0;
}

int ian_trainer_load_param(ian_trainer* t, const char* name, const float* data, int64_t numel) {
  if (!t || !name || !data) return -1;
  if (t->finalized) return tfail(t, -6, "trainer already finalized");
  auto it = t->shapes.find(name);
  if (it == t->shapes.end()) return tfail(t, -2, "unknown parameter '%s'", name);
  if (it->second.numel() != numel) return tfail(t, -3, "parameter '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)it->second.numel());
  t->host[name].assign(data, data + numel);
  return 0;
}

int ian_trainer_set_made_masks(ian_trainer* t, const float* m0, const float* m1, const float* md, int32_t n) {
  if (!t || !m0 || !m1 || !md || n != t->cfg.num_latents) return tfail(t, -1, "bad argument to ian_trainer_set_made_masks");
  const float* src[3] = {m0, m1, md};
  for (int k = 0; k < 3; ++k) {
    t->masks[k].assign(src[k], src[k] + (size_t)n * n);
    for (float v : t->masks[k])
      if (v != 0.f && v != 1.f) return tfail(t, -3, "MADE mask %d is not 0/1 valued", k);
  }
  t->made_n = n;
  return 0;
}

int ian_trainer_finalize(ian_trainer* t) {
  if (!t) return -1;
  if (t->finalized) return tfail(t, -6, "trainer already finalized");
  const int Z = t->cfg.num_latents;
  if (t->made_n != Z) return tfail(t, -3, "MADE masks not set (ian_trainer_set_made_masks)");
  for (auto& kv : t->shapes)
    if (!t->host.count(kv.first)) return tfail(t, -2, "missing parameter '%s'", kv.first.c_str());
  int rc;
  for (int gi = 0; gi < 4; ++gi) {
    Group* g = &t->grp[gi];
    g->p = dalloc(t, g->numel);
    if (gi != G_STATS) { g->g = dalloc(t, g->numel); g->m = dalloc(t, g->numel); g->v = dalloc(t, g->numel); }
    if (!g->p) return tfail(t, -20, "out of device memory (parameter groups)");
    std::vector<float> flat((size_t)g->numel, 0.f);
    for (int id : g->params) {
      const std::vector<float>& v = t->host[t->params[id].name];
      memcpy(flat.data() + t->params[id].off, v.data(), v.size() * sizeof(float));
    }
    THIP(hipMemcpy(g->p, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  t->touched.assign(t->params.size(), 0);
  t->pr.enc_conv1_b = param(t, "enc_conv1.b"); t->pr.mb_theta = param(t, "minibatch_discrim.theta");
  t->pr.mb_lws = param(t, "minibatch_discrim.log_weight_scale"); t->pr.mb_b = param(t, "minibatch_discrim.b");
  t->pr.discrimi_W = param(t, "discrimi.W"); t->pr.l_dec_fc2_b = param(t, "l_dec_fc2.b");
  {  // MADE x2: never trained -> pre-masked constants (layers.py:671,703)
    std::vector<float> w((size_t)6 * Z * Z), b((size_t)6 * Z);
    int k = 0;
    for (const char* m : {"l_IAF_mu", "l_IAF_ls"}) {
      int j = 0;
      for (const char* l : {"_input", "_output_W", "_output_D"}) {
        const std::vector<float>& W = t->host[std::string(m) + l + ".W"];
        for (int i = 0; i < Z * Z; ++i) w[(size_t)k * Z * Z + i] = W[i] * t->masks[j][i];
        memcpy(b.data() + (size_t)k * Z, t->host[std::string(m) + l + ".b"].data(), Z * sizeof(float));
        ++k; ++j;
      }
    }
    t->made_w = dalloc(t, w.size()); t->made_b = dalloc(t, b.size());
    THIP(hipMemcpy(t->made_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    THIP(hipMemcpy(t->made_b, b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  {  // l_dec_fc2 output is stored (H,W,C) while its bias is indexed (C,H,W) (App. B.6)
    const int Cc = 512, Hh = 4, Ww = 4;
    std::vector<int32_t> perm(Cc * Hh * Ww), inv(Cc * Hh * Ww);
    for (int hh = 0; hh < Hh; ++hh)
      for (int ww = 0; ww < Ww; ++ww)
        for (int c = 0; c < Cc; ++c) perm[(hh * Ww + ww) * Cc + c] = (c * Hh + hh) * Ww + ww;  // hwc position -> chw index
    for (size_t i = 0; i < perm.size(); ++i) inv[perm[i]] = (int32_t)i;                         // chw index -> hwc position
    t->fc2_perm = (int32_t*)dalloc(t, perm.size()); t->fc2_inv = (int32_t*)dalloc(t, inv.size());
    THIP(hipMemcpy(t->fc2_perm, perm.data(), perm.size() * 4, hipMemcpyHostToDevice));
    THIP(hipMemcpy(t->fc2_inv, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
  }
  t->fc2_bias = dalloc(t, 8192); t->fc2_db = dalloc(t, 8192); t->fc2_tmp = dalloc(t, 8192); t->tmp_big = dalloc64(t, 2 * 8192);
  t->ws_stats_cap = (size_t)256 * 2 * 8192;
  t->ws_stats = dalloc64(t, t->ws_stats_cap);
  t->ws_loss = dalloc(t, 1024 * 2); t->scalars = dalloc(t, 64);
  t->mb_W = dalloc(t, (size_t)1024 * 2500); t->mb_dW = dalloc(t, (size_t)1024 * 2500); t->mb_colscale = dalloc(t, 2500);
  t->tmp_vals = dalloc64(t, 2048); t->ortho_vals = dalloc(t, 2048);
  if ((rc = build_layers(t))) return rc;
  enc_alloc(t, t->EX, "EX"); enc_alloc(t, t->EH, "EH"); enc_alloc(t, t->EG, "EG");
  z_alloc(t);
  dec_alloc(t, t->DZ, "DZ"); dec_alloc(t, t->DG, "DG");
  if (!t->unresolved.empty()) return tfail(t, -2, "the training graph names a parameter that is not declared: '%s'", t->unresolved.c_str());
  t->zgen = dalloc(t, (size_t)t->n * 128); t->zgen0 = dalloc(t, (size_t)t->n * 128);
  t->xin = dalloc(t, (size_t)t->n * 3 * 4096); t->zin = dalloc(t, (size_t)t->n * 100); t->epsin = dalloc(t, (size_t)t->n * 100);
  if (t->oom) return tfail(t, -20, "out of device memory while allocating the training step's buffers (batch %d per GPU)", t->n);
  if (const char* e = getenv("IAN_WGRAD_PRIORITY")) t->wgrad_priority = atoi(e);
#ifdef IAN_ABLATION
  if (const char* e = getenv("IAN_DUAL_CHAIN_TIMING")) t->dual_timing = atoi(e);   // timing-only, results wrong: libian_ablation.so only
#endif
  if (make_wgrad_stream(t) != 0) t->st2 = nullptr;   // no second stream: weight gradients stay on the compute stream
  if (t->world > 1) THIP(hipStreamCreateWithFlags(&t->st_comm, hipStreamNonBlocking));
  if (t->exact && ((t->n & (t->n - 1)) || (t->world & (t->world - 1))))
    fprintf(stderr, "libian: per-rank batch %d x world %d is not a power of two: the partial-sum tree of the batch statistics associates "
                    "differently on N ranks and in one process, so the data-parallel step is NOT guaranteed bit-identical to the "
                    "single-process step (float64 sums: the float32 statistics can differ in the last bit); train_IAN.py's "
                    "semantics are unaffected\n", t->n, t->world);
  t->dirty[G_ENC] = t->dirty[G_Z] = t->dirty[G_DEC] = true;
  t->host.clear();
  t->finalized = true;
  return 0;
}

int ian_trainer_set_comm(ian_trainer* t, const ian_comm_ops* ops, int32_t exact) {
  if (!t || !ops) return -1;
  if (t->finalized) return tfail(t, -6, "ian_trainer_set_comm must be called before ian_trainer_finalize (buffer sizes depend on the world size)");
  if (ops->world < 1 || ops->rank < 0 || ops->rank >= ops->world) return tfail(t, -1, "ian_trainer_set_comm: bad world / rank (%d / %d)", ops->world, ops->rank);
  if (ops->world > 1 && (!ops->allreduce_sum || !ops->wait_all || !ops->allgather)) return tfail(t, -1, "ian_trainer_set_comm: a callback is NULL");
  t->comm = *ops;
  t->world = ops->world;
  t->rank = ops->rank;
  t->exact = (exact && ops->world > 1) ? 1 : 0;
  t->N = t->n * t->world;
  return 0;
}

}  // extern "C"

namespace {
// entry bookkeeping shared by ian_train_step and the piecewise entries: stream hand-over guard + host -> device staging
int enter(ian_trainer* t, void* stream) {
  if (!t) return -1;
  if (!t->finalized) return tfail(t, -6, "ian_trainer_finalize has not been called");
  hipStream_t st = (hipStream_t)stream;
  if (t->have_last_stream && t->last_stream != st) THIP(hipStreamSynchronize(t->last_stream));  // buffers are shared between calls
  t->st = st;
  t->last_stream = st;
  t->have_last_stream = true;
  return 0;
}
int stage_inputs(ian_trainer* t, const float** x, const float** zrand, const float** eps, int n) {
  const std::pair<const float**, std::pair<float*, size_t>> ins[3] = {{x, {t->xin, (size_t)n * 3 * 4096}}, {zrand, {t->zin, (size_t)n * 100}},
                                                                      {eps, {t->epsin, (size_t)n * 100}}};
  for (auto& in : ins)
    if (!is_device_ptr(*in.first)) {
      THIP(hipMemcpyAsync(in.second.first, *in.first, in.second.second * sizeof(float), hipMemcpyHostToDevice, t->st));
      *in.first = in.second.first;
    }
  return 0;
}
int check_step_args(ian_trainer* t, const float* x, const float* zrand, const float* eps, int n, const char* who) {
  if (!x || !zrand || !eps) return tfail(t, -1, "null pointer passed to %s", who);
  if (n != t->n) return tfail(t, -7, "%s: batch %d, the trainer was created for %d per GPU (batch statistics are per minibatch)", who, n, t->n);
  return 0;
}
int step_body(ian_trainer* t, bool gen, const float* x, const float* zrand, const float* eps, float* metrics9) {
  int rc;
  if ((rc = forward(t, x, zrand, eps))) return rc;
  if ((metrics9 || t->world > 1) && (rc = metrics_device(t))) return rc;
  if (metrics9 && (rc = metrics_read(t, metrics9))) return rc;
  if ((rc = backward(t, gen))) return rc;
  if ((rc = finish_allreduce(t, gen ? 0 : 1))) return rc;
  if ((rc = regularizers(t, gen))) return rc;
  return adam_both(t, gen);
}
// error path of any entry that may have issued work on the trainer's own streams: nothing of it may still be running (and
// writing the shared buffers) when the caller sees the error code
void quiesce(ian_trainer* t) {
  const std::string keep = t->err;
  if (t->st2) (void)hipStreamSynchronize(t->st2);
  if (t->st_comm) (void)hipStreamSynchronize(t->st_comm);
  (void)hipStreamSynchronize(t->st);
  (void)hipGetLastError();
  t->ev_used = 0;
  t->buckets = nullptr;
  t->err = keep;
}
}  // namespace

extern "C" {

/* One update of train_IAN.py:309-329.  which: 0 = update_gen, 1 = update_discrim.  x (n,3,64,64) in [-1,1], zrand (n,100),
   eps (n,100): host or device pointers; n = the PER-RANK batch.  metrics: NULL or 9 HOST floats = discrim_d_loss, gen_recon_loss,
   gen_sample_loss, discrim_g_loss, discrim_acc, kl_div, pixel_loss, pixel_acc, feature_loss of THIS (global) minibatch before the
   update (reading them synchronises the stream). */
int ian_train_step(ian_trainer* t, int32_t which, const float* x, const float* zrand, const float* eps, int32_t n, float* metrics9, void* stream) {
  int rc;
  if ((rc = enter(t, stream))) return rc;
  if ((rc = check_step_args(t, x, zrand, eps, n, "ian_train_step"))) return rc;
  if (which != 0 && which != 1) return tfail(t, -7, "ian_train_step: which must be 0 (update_gen) or 1 (update_discrim)");
  t->xhat_override = t->xgen_override = nullptr;
  if ((rc = stage_inputs(t, &x, &zrand, &eps, n))) return rc;
  rc = step_body(t, which == 0, x, zrand, eps, metrics9);
  if (rc) quiesce(t);
  return rc;
}

/* ---- the same step in pieces (tests, diagnostics): forward / metrics / backward / all-reduce / regularizers / Adam --------- */
int ian_trainer_forward(ian_trainer* t, const float* x, const float* zrand, const float* eps, int32_t n, const float* xhat_override,
                        const float* xgen_override, void* stream) {
  int rc;
  if ((rc = enter(t, stream))) return rc;
  if ((rc = check_step_args(t, x, zrand, eps, n, "ian_trainer_forward"))) return rc;
  if ((xhat_override && !is_device_ptr(xhat_override)) || (xgen_override && !is_device_ptr(xgen_override)))
    return tfail(t, -1, "ian_trainer_forward: the override images must be device buffers");
  if ((rc = stage_inputs(t, &x, &zrand, &eps, n))) return rc;
  t->xhat_override = xhat_override;
  t->xgen_override = xgen_override;
  rc = forward(t, x, zrand, eps);
  t->xhat_override = t->xgen_override = nullptr;
  if (rc) quiesce(t);
  return rc;
}
int ian_trainer_metrics(ian_trainer* t, float* metrics9) {
  if (!t || !t->finalized || !metrics9) return -1;
  if (!t->X) return tfail(t, -6, "ian_trainer_metrics: no forward pass has run");
  return metrics(t, metrics9);
}
int ian_trainer_backward(ian_trainer* t, int32_t which) {
  if (!t || !t->finalized || (which != 0 && which != 1)) return -1;
  if (!t->X) return tfail(t, -6, "ian_trainer_backward: no forward pass has run");
  const int rc = backward(t, which == 0);
  if (rc) quiesce(t);
  return rc;
}
int ian_trainer_finish_allreduce(ian_trainer* t, int32_t which) {
  if (!t || !t->finalized || (which != 0 && which != 1)) return -1;
  const int rc = finish_allreduce(t, which);
  if (rc) quiesce(t);
  return rc;
}
int ian_trainer_regularizers(ian_trainer* t, int32_t which) {
  if (!t || !t->finalized || (which != 0 && which != 1)) return -1;
  int rc = join_side_stream(t);
  return rc ? rc : regularizers(t, which == 0);
}
int ian_trainer_apply_adam(ian_trainer* t, int32_t which) {
  if (!t || !t->finalized || (which != 0 && which != 1)) return -1;
  int rc = join_side_stream(t);
  if (rc) return rc;
  return adam_both(t, which == 0);
}
/* One encoder backward sweep of pass 0 = encoder(X), 1 = encoder(X_hat), 2 = encoder(X_gen) with cross-entropy seeds
   dlogits = w0 (p - onehot(t0)) + w1 (p - onehot(t1)) (t < 0: none); reset != 0 starts a fresh gradient sweep first. */
int ian_trainer_enc_backward(ian_trainer* t, int32_t pass, int32_t t0, float w0, int32_t t1, float w1, int32_t feature_seeded, int32_t want_w,
                             int32_t want_dx, int32_t reset) {
  if (!t || !t->finalized || pass < 0 || pass > 2) return -1;
  if (reset) {
    int rc = join_side_stream(t);
    if (rc) return rc;
    t->touched.assign(t->params.size(), 0);
    t->evlog.clear();
    t->buckets = nullptr;
  }
  int rc = enc_backward(t, pass == 0 ? t->EX : (pass == 1 ? t->EH : t->EG), t0, w0, t1, w1, feature_seeded != 0, want_w != 0, want_dx != 0);
  if (!rc) rc = join_side_stream(t);
  if (rc) quiesce(t);
  return rc;
}
/* Device address of an internal buffer: "<pass>.<name>" with pass in EX EH EG ZS DZ DG (activations and gradients, NHWC with the
   channel stride rounded up to 32; images NCHW), "<pass>.<bn>.<mean|inv_std|scale|shift>" (float32 [C]),
   "<pass>.<bn>.<sums|bsums>" (float64 [2][C]; numel counts doubles), "scalars", "ws_loss".  Tests / diagnostics only. */
int ian_trainer_buffer(ian_trainer* t, const char* name, void** ptr, int64_t* numel) {
  if (!t || !t->finalized || !name || !ptr) return -1;
  const std::string s = name;
  if (s == "scalars") { *ptr = t->scalars; if (numel) *numel = 64; return 0; }
  if (s == "ws_loss") { *ptr = t->ws_loss; if (numel) *numel = 2048; return 0; }
  auto it = t->bufs.find(s);
  if (it != t->bufs.end()) {
    *ptr = it->second;
    if (numel) {
      auto sz = t->alloc_floats.find(it->second);
      *numel = sz != t->alloc_floats.end() ? (int64_t)sz->second : -1;
    }
    return 0;
  }
  const size_t d = s.rfind('.');
  auto bi = d == std::string::npos ? t->bns.end() : t->bns.find(s.substr(0, d));
  if (bi != t->bns.end()) {
    const std::string f = s.substr(d + 1);
    BN& b = *bi->second;
    void* p = f == "mean" ? (void*)b.mean : f == "inv_std" ? (void*)b.inv_std : f == "scale" ? (void*)b.scale : f == "shift" ? (void*)b.shift
              : f == "sums" ? (void*)b.sums : f == "bsums" ? (void*)b.bsums : nullptr;
    if (p) {
      *ptr = p;
      if (numel) *numel = (f == "sums" || f == "bsums") ? 2 * b.C : b.C;
      return 0;
    }
  }
  return tfail(t, -2, "unknown buffer '%s'", name);
}
/* group 0 encoder_params, 1 Z_params, 2 decoder_params, 3 batch-norm running averages: the flat device buffers (reference layouts). */
int ian_trainer_group(ian_trainer* t, int32_t group, float** p, float** g, float** m, float** v, int64_t* numel) {
  if (!t || !t->finalized || group < 0 || group > 3) return -1;
  Group& gr = t->grp[group];
  if (p) *p = gr.p;
  if (g) *g = gr.g;
  if (m) *m = gr.m;
  if (v) *v = gr.v;
  if (numel) *numel = gr.numel;
  return 0;
}
int ian_trainer_param_info(ian_trainer* t, const char* name, int32_t* group, int64_t* offset, int64_t* numel) {
  if (!t || !name) return -1;
  auto it = t->pindex.find(name);
  if (it == t->pindex.end()) return tfail(t, -2, "unknown parameter '%s'", name);
  const Param& q = t->params[it->second];
  if (group) *group = q.group;
  if (offset) *offset = q.off;
  if (numel) *numel = q.shape.numel();
  return 0;
}
/* Parameters of `group` were written behind the trainer's back (tests, checkpoint loading): repack before the next forward. */
int ian_trainer_mark_dirty(ian_trainer* t, int32_t group) {
  if (!t || group < 0 || group > 2) return -1;
  t->dirty[group] = true;
  return 0;
}
/* "exposed_ms_gen" / "exposed_ms_discrim": mean stall of the compute stream on the gradient all-reduce per update of that kind
   (option measure_exposed = 1; synchronises); "plan_buckets_gen|discrim"; "overlap_log" (entries kept); "world", "rank", "exact",
   "global_batch". */
int ian_trainer_stat(ian_trainer* t, const char* key, double* out) {
  if (!t || !key || !out) return -1;
  const std::string k = key;
  if (k == "exposed_ms_gen" || k == "exposed_ms_discrim") {
    fold_exposed(t);
    const int w = k == "exposed_ms_gen" ? 0 : 1;
    *out = t->exposed_n[w] ? t->exposed_ms[w] / t->exposed_n[w] : 0.0;
  } else if (k == "gather_ms_gen" || k == "gather_ms_discrim" || k == "gathers_gen" || k == "gathers_discrim") {
    THIP(hipDeviceSynchronize());
    fold_gathers(t, 0);
    fold_gathers(t, 1);
    const int w = (k == "gather_ms_gen" || k == "gathers_gen") ? 0 : 1;
    const double d = t->gather_n[w] ? (double)t->gather_n[w] : 1.0;
    *out = (k.compare(0, 10, "gather_ms_") == 0 ? t->gather_ms[w] : t->gather_calls[w]) / d;
  } else if (k == "plan_buckets_gen") *out = t->plans.count(0) ? (double)t->plans[0].size() : 0.0;
  else if (k == "plan_buckets_discrim") *out = t->plans.count(1) ? (double)t->plans[1].size() : 0.0;
  else if (k == "overlap_log") *out = (double)t->overlap_log.size();
  else if (k == "world") *out = t->world;
  else if (k == "rank") *out = t->rank;
  else if (k == "exact") *out = t->exact;
  else if (k == "global_batch") *out = t->N;
  else return tfail(t, -1, "unknown statistic '%s'", key);
  return 0;
}
/* rec[6] = which, group, first element, bytes, index of the gradient write after which the bucket was handed over, number of
   gradient writes of that backward sweep (0 while the sweep is still open) */
int ian_trainer_overlap_log(ian_trainer* t, int32_t index, int64_t* rec) {
  if (!t || !rec || index < 0 || (size_t)index >= t->overlap_log.size()) return -1;
  const OverlapRec& r = t->overlap_log[index];
  rec[0] = r.which; rec[1] = r.group; rec[2] = r.lo; rec[3] = r.bytes; rec[4] = r.issued_at_write; rec[5] = r.writes_in_backward;
  return 0;
}

int ian_trainer_autotune(ian_trainer* t, void* stream) {
  int rc;
  if ((rc = enter(t, stream))) return rc;
  const size_t need = (size_t)t->n * 64 * 64 * 128;  // the largest activation of IAN.py (dec_conv4 output)
  std::vector<float> rnd(need);
  unsigned s = 12345u;
  for (auto& v : rnd) {
    s = s * 1664525u + 1013904223u;
    v = ((s >> 8) & 0xFFFF) / 32768.f - 1.f;
  }
  float *a = nullptr, *b = nullptr;
  THIP(hipMalloc((void**)&a, need * sizeof(float)));
  if (hipMalloc((void**)&b, need * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(a);
    return tfail(t, -20, "out of device memory (autotune operands)");
  }
  rc = 0;
  if (hipMemcpy(a, rnd.data(), need * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(b, rnd.data(), need * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    rc = tfail(t, -20, "hipMemcpy of the autotune operands failed");
  }
  if (!rc) rc = refresh_weights(t);
  for (LayerRef& r : t->layers) {
    if (rc) break;
    rc = ian_layer_autotune(r.l, t->n, a, b, (int64_t)need, t->st);
    if (rc) tfail(t, rc, "ian_layer_autotune(%s) failed (%d): %s", r.key.c_str(), rc, ian_layer_last_error(r.l));
  }
  (void)hipStreamSynchronize(t->st);
  (void)hipFree(a);
  (void)hipFree(b);
  return rc;
}

/* Copy a parameter (trainable, batch-norm running average) or, grad != 0, its gradient of the last step to the host. */
int ian_trainer_read_param(ian_trainer* t, const char* name, int32_t grad, float* out, int64_t numel) {
  if (!t || !t->finalized || !name || !out) return -1;
  auto it = t->pindex.find(name);
  if (it == t->pindex.end()) return tfail(t, -2, "unknown parameter '%s'", name);
  const Param& q = t->params[it->second];
  const Group* g = &t->grp[q.group];
  if (grad && !g->g) return tfail(t, -2, "'%s' has no gradient (not trainable)", name);
  if (q.shape.numel() != numel) return tfail(t, -3, "parameter '%s' has %lld elements", name, (long long)q.shape.numel());
  THIP(hipDeviceSynchronize());   // the compute stream, the weight-gradient stream and the bucket stream
  THIP(hipMemcpy(out, (grad ? g->g : g->p) + q.off, numel * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int ian_trainer_set_option(ian_trainer* t, const char* key, double value) {
  if (!t || !key) return -1;
  const std::string k = key;
  if (k == "learning_rate") t->cfg.learning_rate = value;  // train_IAN.py:523-527 learning-rate schedule
  else if (k == "head6") t->head6 = value != 0.0;
  else if (k == "overlap_wgrad") t->overlap_wgrad = value != 0.0;
  else if (k == "wgrad_priority") {      // 0: default-priority weight-gradient stream, 1: lowest priority (see make_wgrad_stream)
    (void)hipDeviceSynchronize();
    t->wgrad_priority = value != 0.0;
    if (t->finalized) (void)make_wgrad_stream(t);
  }
  else if (k == "update_running") t->update_running = value != 0.0;
  else if (k == "fused_stats") t->fused_stats = value != 0.0;                 // GEMM-epilogue batch statistics (single-process step)
  else if (k == "overlap") t->overlap = value != 0.0;                       // gradient buckets handed over during backward
  else if (k == "bucket_bytes") { t->bucket_bytes = (int64_t)value > 4 ? (int64_t)value : 4; t->plans.clear(); }
  else if (k == "measure_exposed") {
    (void)hipDeviceSynchronize();
    t->measure_exposed = value != 0.0; t->exposed_ms[0] = t->exposed_ms[1] = 0; t->exposed_n[0] = t->exposed_n[1] = 0; t->ex_pending = false;
    for (int w = 0; w < 2; ++w) { t->gev_used[w] = 0; t->gather_ms[w] = t->gather_calls[w] = 0; t->gather_n[w] = 0; }
  }
  else return tfail(t, -1, "unknown option '%s'", key);
  return 0;
}

int32_t ian_trainer_adam_steps(ian_trainer* t, int32_t group) {  /* 0 encoder_params, 1 Z_params, 2 decoder_params */
  if (!t) return -1;
  return group < 0 || group > 2 ? -1 : t->grp[group].t;
}

const char* ian_trainer_last_error(ian_trainer* t) { return t ? t->err.c_str() : "null trainer"; }

void ian_trainer_destroy(ian_trainer* t) {
  if (!t) return;
  IAN_GUARD_CHECK("ian_trainer_destroy");
  (void)hipDeviceSynchronize();
  for (hipEvent_t e : t->events) (void)hipEventDestroy(e);
  if (t->st2) (void)hipStreamDestroy(t->st2);
  if (t->st_comm) (void)hipStreamDestroy(t->st_comm);
  if (t->stB) (void)hipStreamDestroy(t->stB);
  if (t->ex0) (void)hipEventDestroy(t->ex0);
  if (t->ex1) (void)hipEventDestroy(t->ex1);
  for (auto& pool : t->gev)
    for (auto& e : pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (LayerRef& r : t->layers) ian_layer_destroy(r.l);
  for (float* p : t->allocs)
    if (p) (void)hipFree(p);
  delete t;
}

}  // extern "C"
