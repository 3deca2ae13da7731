// CPU call trace of the training sequencer csrc/ian_trainer.cpp (tests/test_trainer_trace_host.py).  The trainer is host-only code: its
// external symbols are the ian_k_* / ian_layer_* entry points of include/ian_train.h and a handful of HIP runtime calls, all plain C.  This
// program defines a recording stub for every one of them, is compiled together with the trainer (g++, ASan + UBSan, no GPU, no Python)
// and prints what the trainer would have launched, one line per call:
//   <function> <argument> ...      pointers into stub device memory  #k+byte_offset  (k = ordinal of the hipMalloc), host pointers `host`,
//                                  NULL `null`, streams s<k> (s0 = the caller's), events e<k>, layers L<k> in creation order, floats %.9g,
//                                  doubles %.17g, pointer arrays element by element inside [ ]
//   == <text>                      markers written by main: finalize, the parameter groups, parameters and named buffers,
//                                  step <i> which <w>, destroy
// Device memory is calloc, copies are memcpy (so ASan checks every size the trainer passes to them), ian_layer_stats_chunks answers 8
// after a launch that ian_layer_stats_next armed and 0 otherwise, the ian_comm_ops table records its three collectives; one process
// plays rank 0.  Usage:
//   trainer_trace PARAMS [--dump] [key=value ...] [@K:option=value ...]
// PARAMS: text file of `name numel` lines (every parameter gets the constant 0.5, the MADE masks are all ones).  Keys: mode=step|pieces
// (ian_train_step, or forward / metrics / backward / finish_allreduce / regularizers / apply_adam), which=0101 (the updates to run),
// world=1|2 (global batch 4 either way), exact=0|1; every other key is passed to ian_trainer_set_option after finalize, `@K:` ones
// right before step K.  Without --dump only the number of traced calls per step is printed.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../include/ian_train.h"

struct ian_layer {
  int id;
  bool armed;
  int chunks;
};

namespace {
struct Stream { void* s; };   // an argument that names a stream (the ABI passes it as void*)
inline Stream S(void* s) { return {s}; }

bool g_dump = false;
long g_calls = 0;
std::map<const char*, std::pair<size_t, int>> g_alloc;   // base -> (bytes, ordinal)
int g_mallocs = 0, g_layers = 0;
uintptr_t g_streams = 0, g_events = 0;   // handles are small integers in creation order

const std::pair<const char* const, std::pair<size_t, int>>* device_block(const void* p) {
  auto it = g_alloc.upper_bound((const char*)p);
  if (it == g_alloc.begin()) return nullptr;
  --it;
  return (const char*)p < it->first + it->second.first ? &*it : nullptr;
}
void put(const void* p) {
  if (!p) { printf(" null"); return; }
  if (auto* b = device_block(p)) printf(" #%d+%td", b->second.second, (const char*)p - b->first);
  else printf(" host");
}
void put(ian_layer* l) { printf(" L%d", l->id); }
void put(Stream s) { printf(" s%zu", (size_t)(uintptr_t)s.s); }
void put(hipStream_t s) { printf(" s%zu", (size_t)(uintptr_t)s); }
void put(hipEvent_t e) { printf(" e%zu", (size_t)(uintptr_t)e); }
void put(int v) { printf(" %d", v); }
void put(unsigned v) { printf(" %u", v); }
void put(long v) { printf(" %ld", v); }
void put(unsigned long v) { printf(" %lu", v); }
void put(float v) { printf(" %.9g", v); }
void put(double v) { printf(" %.17g", v); }
struct Arr { const float* const* p; int n; };
void put(Arr a) {
  if (!a.p) { printf(" null"); return; }
  printf(" [");
  for (int i = 0; i < a.n; ++i) put(a.p[i]);
  printf(" ]");
}
template <class... A>
int rec(const char* name, A... a) {
  ++g_calls;
  if (!g_dump) return 0;
  printf("%s", name);
  (put(a), ...);
  printf("\n");
  return 0;
}
void launch_consumes_arming(ian_layer* l) {
  l->chunks = l->armed ? 8 : 0;
  l->armed = false;
}

int comm_allreduce(void*, float* buf, int64_t count, void* stream) { return rec("allreduce_sum", buf, count, S(stream)); }
int comm_wait_all(void*, void* stream) { return rec("wait_all", S(stream)); }
int comm_allgather(void*, const float* src, float* dst, int64_t count, void* stream) {
  memcpy(dst, src, (size_t)count * sizeof(float));   // rank 0's slot
  return rec("allgather", src, dst, count, S(stream));
}
}  // namespace

extern "C" {
// ---- layers -----------------------------------------------------------------------------------------------------------------------
int ian_layer_create(const ian_op_desc* d, int32_t deconv_flip, ian_layer** out) {
  *out = new ian_layer{g_layers++, false, 0};
  ++g_calls;
  if (g_dump) {
    printf("ian_layer_create L%d kind %d cin %d cout %d in %dx%d flat %d %d %d unflat %d %d %d scales", (*out)->id, d->kind, d->cin,
           d->cout, d->in_h, d->in_w, d->flat_c, d->flat_h, d->flat_w, d->unflat_c, d->unflat_h, d->unflat_w);
    for (int i = 0; i < d->n_scales; ++i) printf(" %d", d->scales[i]);
    printf(" flip %d\n", deconv_flip);
  }
  return 0;
}
void ian_layer_destroy(ian_layer* l) {
  rec("ian_layer_destroy", l);
  delete l;
}
const char* ian_layer_last_error(ian_layer*) { return "stub"; }
const char* ian_k_last_error(void) { return "stub"; }
int ian_layer_stats_next(ian_layer* l, int32_t mode, const float* a, const float* yraw, const float* mean, const float* inv_std,
                         int32_t act, double* partial, int64_t cap_doubles) {
  l->armed = mode != 0;
  return rec("ian_layer_stats_next", l, mode, a, yraw, mean, inv_std, act, partial, cap_doubles);
}
int32_t ian_layer_stats_chunks(ian_layer* l) {
  rec("ian_layer_stats_chunks", l, l->chunks);
  return l->chunks;
}
int ian_layer_set_params(ian_layer* l, const float* const* params, int32_t nparams, void* stream) {
  return rec("ian_layer_set_params", l, Arr{params, nparams}, nparams, S(stream));
}
int ian_layer_forward(ian_layer* l, const float* x, int32_t n, float* y, int32_t y_stride, const float* bias, const float* res, int32_t act,
                      void* stream) {
  launch_consumes_arming(l);
  return rec("ian_layer_forward", l, x, n, y, y_stride, bias, res, act, S(stream));
}
int ian_layer_backward_data(ian_layer* l, const float* dy, int32_t n, float* dx, int32_t dx_stride, int32_t accumulate, void* stream) {
  launch_consumes_arming(l);
  return rec("ian_layer_backward_data", l, dy, n, dx, dx_stride, accumulate, S(stream));
}
int ian_layer_backward_weight(ian_layer* l, const float* x, const float* dy, int32_t n, float* const* dparams, int32_t nparams,
                              int32_t accumulate, void* stream) {
  return rec("ian_layer_backward_weight", l, x, dy, n, Arr{dparams, nparams}, nparams, accumulate, S(stream));
}
int ian_layer_head6_backward(ian_layer* l0, ian_layer* l1, ian_layer* l2, const float* x, const float* dy0, const float* dy1,
                             const float* dy2, int32_t n, int32_t dy_stride, float* dx, int32_t dx_stride, int32_t dx_accumulate,
                             float* const* dparams0, float* const* dparams1, float* const* dparams2, int32_t nparams,
                             int32_t accumulate, void* stream) {
  launch_consumes_arming(l0);
  return rec("ian_layer_head6_backward", l0, l1, l2, x, dy0, dy1, dy2, n, dy_stride, dx, dx_stride, dx_accumulate, Arr{dparams0, nparams},
             Arr{dparams1, nparams}, Arr{dparams2, nparams}, nparams, accumulate, S(stream));
}
// ---- the other entry points of include/ian_train.h that the trainer calls: record and return 0 ------------------------------------
int ian_layer_head6_forward(ian_layer* l0, ian_layer* l1, ian_layer* l2, const float* x, int32_t n, float* y0, float* y1, float* y2,
    int32_t y_stride, int32_t act0, int32_t act1, int32_t act2, void* stream) {
  return rec("ian_layer_head6_forward", l0, l1, l2, x, n, y0, y1, y2, y_stride, act0, act1, act2, S(stream));
}
int ian_layer_autotune(ian_layer* l, int32_t n, float* scratch_a, float* scratch_b, int64_t cap_floats, void* stream) {
  return rec("ian_layer_autotune", l, n, scratch_a, scratch_b, cap_floats, S(stream));
}
int ian_k_colstats(int32_t mode, const float* x, const float* a, const float* y, const float* mean, const float* inv_std, int64_t rows,
    int32_t C, int32_t stride, int32_t act, double* workspace, int32_t nchunks, double* sums, void* stream) {
  return rec("ian_k_colstats", mode, x, a, y, mean, inv_std, rows, C, stride, act, workspace, nchunks, sums, S(stream));
}
int ian_k_tree_sum(const double* partial, int32_t count, int32_t width, double* out, void* stream) {
  return rec("ian_k_tree_sum", partial, count, width, out, S(stream));
}
int ian_k_bn_make_affine(const double* sums, float count, float eps, const float* gamma, const float* beta, int32_t C, float* mean, float*
    inv_std, float* scale, float* shift, void* stream) {
  return rec("ian_k_bn_make_affine", sums, count, eps, gamma, beta, C, mean, inv_std, scale, shift, S(stream));
}
int ian_k_bn_running(float* run_mean, const float* mean, float* run_inv_std, const float* inv_std, int32_t C, float keep, float alpha,
    void* stream) {
  return rec("ian_k_bn_running", run_mean, mean, run_inv_std, inv_std, C, keep, alpha, S(stream));
}
int ian_k_bn_stats_affine(const float* y, int64_t rows, int32_t C, int32_t stride, double* workspace, int32_t nchunks, double* sums, float
    count, float eps, const float* gamma, const float* beta, float* mean, float* inv_std, float* scale, float* shift, float* run_mean,
    float* run_inv_std, float keep, float alpha, void* stream) {
  return rec("ian_k_bn_stats_affine", y, rows, C, stride, workspace, nchunks, sums, count, eps, gamma, beta, mean, inv_std, scale, shift,
             run_mean, run_inv_std, keep, alpha, S(stream));
}
int ian_k_bn_finish(const double* workspace, int32_t nchunks, int32_t C, double* sums, float count, float eps, const float* gamma, const
    float* beta, float* mean, float* inv_std, float* scale, float* shift, float* run_mean, float* run_inv_std, float keep, float alpha,
    void* stream) {
  return rec("ian_k_bn_finish", workspace, nchunks, C, sums, count, eps, gamma, beta, mean, inv_std, scale, shift, run_mean, run_inv_std,
             keep, alpha, S(stream));
}
int ian_k_bn_bwd_finish(const double* workspace, int32_t nchunks, int32_t C, double* sums, float* gbeta, int32_t acc_beta, float* ggamma,
    int32_t acc_gamma, void* stream) {
  return rec("ian_k_bn_bwd_finish", workspace, nchunks, C, sums, gbeta, acc_beta, ggamma, acc_gamma, S(stream));
}
int ian_k_bn_bwd_stats(const float* dA, const float* a, const float* y, const float* mean, const float* inv_std, int64_t rows, int32_t C,
    int32_t stride, int32_t act, double* workspace, int32_t nchunks, double* sums, float* gbeta, int32_t acc_beta, float* ggamma, int32_t
    acc_gamma, void* stream) {
  return rec("ian_k_bn_bwd_stats", dA, a, y, mean, inv_std, rows, C, stride, act, workspace, nchunks, sums, gbeta, acc_beta, ggamma,
             acc_gamma, S(stream));
}
int ian_k_affine(const float* x, float* y, const float* scale, const float* shift, int64_t rows, int32_t C, int32_t stride, int32_t act,
    void* stream) {
  return rec("ian_k_affine", x, y, scale, shift, rows, C, stride, act, S(stream));
}
int ian_k_bn_bwd(const float* dA, const float* a, const float* y, const float* mean, const float* inv_std, const float* scale, const
    double* sums, float count, float* dy, int64_t rows, int32_t C, int32_t stride, int32_t act, void* stream) {
  return rec("ian_k_bn_bwd", dA, a, y, mean, inv_std, scale, sums, count, dy, rows, C, stride, act, S(stream));
}
int ian_k_axpy(float alpha, const float* x, float* y, int64_t n, int32_t accumulate, void* stream) {
  return rec("ian_k_axpy", alpha, x, y, n, accumulate, S(stream));
}
int ian_k_axpy_f64(double alpha, const double* x, float* y, int64_t n, int32_t accumulate, void* stream) {
  return rec("ian_k_axpy_f64", alpha, x, y, n, accumulate, S(stream));
}
int ian_k_gather(const float* src, const int32_t* map, float* dst, int64_t count, void* stream) {
  return rec("ian_k_gather", src, map, dst, count, S(stream));
}
int ian_k_nchw_to_nhwc(const float* src, float* dst, int32_t n, int32_t hw, int32_t c, int32_t stride, void* stream) {
  return rec("ian_k_nchw_to_nhwc", src, dst, n, hw, c, stride, S(stream));
}
int ian_k_nhwc_to_nchw(const float* src, int32_t stride, float* dst, int32_t n, int32_t hw, int32_t c, void* stream) {
  return rec("ian_k_nhwc_to_nchw", src, stride, dst, n, hw, c, S(stream));
}
int ian_k_globalpool(const float* x, float* y, int32_t n, int32_t hw, int32_t C, int32_t xs, int32_t ys, void* stream) {
  return rec("ian_k_globalpool", x, y, n, hw, C, xs, ys, S(stream));
}
int ian_k_globalpool_bwd(const float* dy, float* dx, int32_t n, int32_t hw, int32_t C, int32_t xs, int32_t ys, int32_t accumulate, void*
    stream) {
  return rec("ian_k_globalpool_bwd", dy, dx, n, hw, C, xs, ys, accumulate, S(stream));
}
int ian_k_mb_weight(const float* theta, const float* lws, float* W, float* colscale, int32_t nin, int32_t ncol, void* stream) {
  return rec("ian_k_mb_weight", theta, lws, W, colscale, nin, ncol, S(stream));
}
int ian_k_mb_weight_bwd(const float* theta, const float* colscale, const float* dW, float* dtheta, float* dlws, int32_t nin, int32_t ncol,
    int32_t accumulate, void* stream) {
  return rec("ian_k_mb_weight_bwd", theta, colscale, dW, dtheta, dlws, nin, ncol, accumulate, S(stream));
}
int ian_k_mb_forward(const float* act_all, int32_t nall, int32_t as, int32_t row0, int32_t n, int32_t nk, int32_t nd, const float* bias,
    const float* feat, int32_t fs, int32_t fin, float* mb, int32_t ms, void* stream) {
  return rec("ian_k_mb_forward", act_all, nall, as, row0, n, nk, nd, bias, feat, fs, fin, mb, ms, S(stream));
}
int ian_k_mb_backward(const float* act_all, int32_t nall, int32_t as, int32_t row0, int32_t n, int32_t nk, int32_t nd, const float*
    df_all, int32_t dfs, float* dact, int32_t das, void* stream) {
  return rec("ian_k_mb_backward", act_all, nall, as, row0, n, nk, nd, df_all, dfs, dact, das, S(stream));
}
int ian_k_disc_head(const float* mb, int32_t ms, int32_t nfeat, const float* Wd, int32_t n, int32_t target0, int32_t target1, int32_t
    acc_target, float* p, float* loss, void* stream) {
  return rec("ian_k_disc_head", mb, ms, nfeat, Wd, n, target0, target1, acc_target, p, loss, S(stream));
}
int ian_k_disc_head_bwd(const float* p, const float* Wd, int32_t nfeat, int32_t n, int32_t t0, float w0, int32_t t1, float w1, float*
    dlogits, float* dmb, int32_t ms, void* stream) {
  return rec("ian_k_disc_head_bwd", p, Wd, nfeat, n, t0, w0, t1, w1, dlogits, dmb, ms, S(stream));
}
int ian_k_disc_head_wgrad(const float* mb, int32_t ms, int32_t nfeat, int32_t n, const float* dlogits, float* dWd, int32_t accumulate,
    void* stream) {
  return rec("ian_k_disc_head_wgrad", mb, ms, nfeat, n, dlogits, dWd, accumulate, S(stream));
}
int ian_k_sample(const float* mu, const float* ls, const float* eps, float* z0, float* klterm, int32_t n, int32_t d, int32_t stride,
    int32_t eps_stride, void* stream) {
  return rec("ian_k_sample", mu, ls, eps, z0, klterm, n, d, stride, eps_stride, S(stream));
}
int ian_k_sample_bwd(const float* mu, const float* ls, const float* eps, const float* dz0, float* dmu, float* dls, int32_t n, int32_t d,
    int32_t stride, int32_t eps_stride, float klw, void* stream) {
  return rec("ian_k_sample_bwd", mu, ls, eps, dz0, dmu, dls, n, d, stride, eps_stride, klw, S(stream));
}
int ian_k_made_iaf(const float* z0, float* z, const float* wts, const float* bias, int32_t n, int32_t d, int32_t zs, void* stream) {
  return rec("ian_k_made_iaf", z0, z, wts, bias, n, d, zs, S(stream));
}
int ian_k_made_iaf_bwd(const float* z0, const float* dz, float* dz0, const float* wts, const float* bias, int32_t n, int32_t d, int32_t
    zs, void* stream) {
  return rec("ian_k_made_iaf_bwd", z0, dz, dz0, wts, bias, n, d, zs, S(stream));
}
int ian_k_beta(const float* R, const float* G, const float* B, float* y_nchw, int32_t n, int32_t hw, int32_t rs, void* stream) {
  return rec("ian_k_beta", R, G, B, y_nchw, n, hw, rs, S(stream));
}
int ian_k_beta_bwd(const float* gout_nchw, const float* R, const float* G, const float* B, float* gR, float* gG, float* gB, int32_t n,
    int32_t hw, int32_t rs, int32_t act, void* stream) {
  return rec("ian_k_beta_bwd", gout_nchw, R, G, B, gR, gG, gB, n, hw, rs, act, S(stream));
}
int ian_k_concat2(const float* a, int32_t ca, int32_t sa, const float* b, int32_t cb, int32_t sb, float* y, int32_t sy, int64_t npix,
    void* stream) {
  return rec("ian_k_concat2", a, ca, sa, b, cb, sb, y, sy, npix, S(stream));
}
int ian_k_grad_pass(const float* gs, int32_t ss, int32_t coff, float* gd, const float* y, int32_t ds, int64_t npix, int32_t C, int32_t
    act, int32_t accumulate, void* stream) {
  return rec("ian_k_grad_pass", gs, ss, coff, gd, y, ds, npix, C, act, accumulate, S(stream));
}
int ian_k_pair_loss(const float* a, const float* b, float* da, int64_t rows, int32_t C, int32_t stride, int32_t mode, float w, int32_t
    accumulate, float* workspace, int32_t nblocks, float scale, float* out, void* stream) {
  return rec("ian_k_pair_loss", a, b, da, rows, C, stride, mode, w, accumulate, workspace, nblocks, scale, out, S(stream));
}
int ian_k_sum_rows(const float* x, int32_t n, int32_t width, float scale, float* out, void* stream) {
  return rec("ian_k_sum_rows", x, n, width, scale, out, S(stream));
}
int ian_k_ortho(const float* W, float* dW, int32_t A, int32_t B, int32_t K, float c, float* vals, void* stream) {
  return rec("ian_k_ortho", W, dW, A, B, K, c, vals, S(stream));
}
int ian_k_adam(float* p, const float* g, float* m, float* v, int64_t n, float a_t, float b1, float b2, float eps, void* stream) {
  return rec("ian_k_adam", p, g, m, v, n, a_t, b1, b2, eps, S(stream));
}
// ---- HIP runtime ------------------------------------------------------------------------------------------------------------------
hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  *p = calloc(1, bytes);
  g_alloc[(const char*)*p] = {bytes, g_mallocs};
  rec("hipMalloc", g_mallocs++, bytes);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  rec("hipFree", (const void*)p);
  g_alloc.erase((const char*)p);
  free(p);
  return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t bytes) {
  memset(p, v, bytes);
  return (hipError_t)rec("hipMemset", (const void*)p, v, bytes);
}
hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t s) {
  memset(p, v, bytes);
  return (hipError_t)rec("hipMemsetAsync", (const void*)p, v, bytes, s);
}
hipError_t hipMemcpy(void* d, const void* s, size_t bytes, hipMemcpyKind kind) {
  memcpy(d, s, bytes);
  return (hipError_t)rec("hipMemcpy", (const void*)d, s, bytes, (int)kind);
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  memcpy(d, s, bytes);
  return (hipError_t)rec("hipMemcpyAsync", (const void*)d, s, bytes, (int)kind, st);
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipDeviceSynchronize(void) { return (hipError_t)rec("hipDeviceSynchronize"); }
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) {
  *least = 0;
  *greatest = -1;
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
  *s = (hipStream_t)++g_streams;
  return (hipError_t)rec("hipStreamCreateWithFlags", *s, flags);
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority) {
  *s = (hipStream_t)++g_streams;
  return (hipError_t)rec("hipStreamCreateWithPriority", *s, flags, priority);
}
hipError_t hipStreamDestroy(hipStream_t s) { return (hipError_t)rec("hipStreamDestroy", s); }
hipError_t hipStreamSynchronize(hipStream_t s) { return (hipError_t)rec("hipStreamSynchronize", s); }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags) { return (hipError_t)rec("hipStreamWaitEvent", s, e, flags); }
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = (hipEvent_t)++g_events;
  return (hipError_t)rec("hipEventCreate", *e);
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  *e = (hipEvent_t)++g_events;
  return (hipError_t)rec("hipEventCreateWithFlags", *e, flags);
}
hipError_t hipEventDestroy(hipEvent_t e) { return (hipError_t)rec("hipEventDestroy", e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return (hipError_t)rec("hipEventRecord", e, s); }
hipError_t hipEventSynchronize(hipEvent_t e) { return (hipError_t)rec("hipEventSynchronize", e); }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = 0.f;
  return (hipError_t)rec("hipEventElapsedTime", a, b);
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p) {
  if (!device_block(p)) return hipErrorInvalidValue;
  memset(a, 0, sizeof *a);
  a->type = hipMemoryTypeDevice;
  return hipSuccess;
}
}  // extern "C"

namespace {
// every name ian_trainer_buffer serves: "<pass>.<buffer>", "<pass>.<bn>.<field>", "scalars", "ws_loss"
std::vector<std::string> buffer_names() {
  std::vector<std::string> v = {"scalars", "ws_loss"}, bn;
  auto add = [&](const char* pass, const std::vector<std::string>& names, bool is_bn) {
    for (auto& n : names) (is_bn ? bn : v).push_back(std::string(pass) + "." + n);
  };
  for (const char* e : {"EX", "EH", "EG"}) {
    add(e, {"x", "dx", "a1", "a2", "a3", "a4", "da1", "da2", "da3", "da4", "y2", "y3", "y4", "feat", "dfeat", "act", "dact", "mb", "dmb",
            "act_all", "dmb_all", "p", "loss", "dlogits"}, false);
    add(e, {"bn2", "bn3", "bn4"}, true);
  }
  add("ZS", {"y_fc1", "f", "df", "y_mu", "mu", "dmu", "y_ls", "ls", "dls", "z0", "z", "dz0", "kl"}, false);
  add("ZS", {"bn_fc1", "bn_mu", "bn_ls"}, true);
  for (const char* d : {"DZ", "DG"}) {
    add(d, {"h0", "dh0", "y4", "h4", "dh4", "R", "G", "B", "Ga", "Ba", "RG", "gR", "gG", "gB", "dRG", "dRt", "xhat", "dxhat", "tmp_img",
            "dz"}, false);
    add(d, {"bn4"}, true);
    for (const char* blk : {"dec_conv2a", "dec_conv3a", "dec_conv4a"}) {
      for (const char* n : {"x", "a", "b", "c", "e", "h", "dx", "da", "dc", "dh"}) add(d, {std::string(blk) + "_" + n}, false);
      for (const char* n : {"_bn0", "_bn1", "_bn2"}) add(d, {std::string(blk) + n}, true);
    }
  }
  for (auto& b : bn)
    for (const char* f : {"mean", "inv_std", "scale", "shift", "sums", "bsums"}) v.push_back(b + "." + f);
  return v;
}
int fail(ian_trainer* t, const char* what, int rc) {
  fprintf(stderr, "%s failed (%d): %s\n", what, rc, t ? ian_trainer_last_error(t) : "");
  return 1;
}
}  // namespace

#define CHECK(call)                           \
  do {                                        \
    const int rc_ = (call);                   \
    if (rc_) return fail(t, #call, rc_);      \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return fail(nullptr, "usage: trainer_trace PARAMS [--dump] [key=value ...] [@K:option=value ...]", 0);
  std::string mode = "step", which = "0101";
  int world = 1, exact = 0;
  std::vector<std::pair<std::string, double>> options;             // after finalize
  std::vector<std::pair<int, std::pair<std::string, double>>> at;  // before step K
  for (int i = 2; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--dump") { g_dump = true; continue; }
    int k = -1;
    if (a[0] == '@') {
      const size_t c = a.find(':');
      if (c == std::string::npos) return fail(nullptr, argv[i], 0);
      k = atoi(a.c_str() + 1);
      a = a.substr(c + 1);
    }
    const size_t eq = a.find('=');
    if (eq == std::string::npos) return fail(nullptr, argv[i], 0);
    const std::string key = a.substr(0, eq), val = a.substr(eq + 1);
    if (k >= 0) at.push_back({k, {key, atof(val.c_str())}});
    else if (key == "mode") mode = val;
    else if (key == "which") which = val;
    else if (key == "world") world = atoi(val.c_str());
    else if (key == "exact") exact = atoi(val.c_str());
    else options.push_back({key, atof(val.c_str())});
  }
  if ((mode != "step" && mode != "pieces") || (world != 1 && world != 2)) return fail(nullptr, "bad mode / world", 0);
  const int B = 4 / world;

  ian_train_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.batch = B; cfg.num_latents = 100; cfg.deconv_flip = 1;
  cfg.learning_rate = 2e-4; cfg.beta1 = 0.5; cfg.reg = 1e-5f; cfg.ortho = 1e-3f;
  cfg.recon_weight = 3.f; cfg.feature_weight = 1.f; cfg.dg_weight = 1.f; cfg.dd_weight = 1.f; cfg.agr_weight = 1.f; cfg.ags_weight = 1.f;
  ian_trainer* t = nullptr;
  CHECK(ian_trainer_create(&cfg, &t));
  std::vector<std::string> names;
  {
    FILE* f = fopen(argv[1], "r");
    if (!f) return fail(nullptr, argv[1], 0);
    char name[256];
    long numel;
    while (fscanf(f, "%255s %ld", name, &numel) == 2) {
      const std::vector<float> v((size_t)numel, 0.5f);
      CHECK(ian_trainer_load_param(t, name, v.data(), numel));
      names.push_back(name);
    }
    fclose(f);
  }
  const std::vector<float> ones(100 * 100, 1.f);
  CHECK(ian_trainer_set_made_masks(t, ones.data(), ones.data(), ones.data(), 100));
  ian_comm_ops ops;
  memset(&ops, 0, sizeof ops);
  ops.world = world; ops.rank = 0;
  ops.allreduce_sum = comm_allreduce; ops.wait_all = comm_wait_all; ops.allgather = comm_allgather;
  if (world > 1) CHECK(ian_trainer_set_comm(t, &ops, exact));
  if (g_dump) printf("== finalize\n");
  CHECK(ian_trainer_finalize(t));
  if (g_dump) {
    for (int g = 0; g < 4; ++g) {
      float *p, *gr, *m, *v;
      int64_t numel;
      CHECK(ian_trainer_group(t, g, &p, &gr, &m, &v, &numel));
      printf("== group %d", g);
      put(p); put(gr); put(m); put(v);
      printf(" %ld\n", (long)numel);
    }
    for (const std::string& nm : names) {
      int32_t g;
      int64_t off, numel;
      if (ian_trainer_param_info(t, nm.c_str(), &g, &off, &numel) == 0)
        printf("== param %s %d %ld %ld\n", nm.c_str(), g, (long)off, (long)numel);
    }
    for (const std::string& nm : buffer_names()) {   // the name registry of ian_trainer_buffer (a name this configuration lacks is skipped)
      void* ptr;
      int64_t numel;
      if (ian_trainer_buffer(t, nm.c_str(), &ptr, &numel)) continue;
      printf("== buffer %s", nm.c_str());
      put(ptr);
      printf(" %ld\n", (long)numel);
    }
  }
  for (auto& o : options) CHECK(ian_trainer_set_option(t, o.first.c_str(), o.second));

  const std::vector<float> X((size_t)B * 3 * 4096, 0.25f), Z((size_t)B * 100, 0.125f), E((size_t)B * 100, -0.125f);
  float met[9];
  for (int i = 0; i < (int)which.size(); ++i) {
    const int w = which[i] - '0';
    for (auto& o : at)
      if (o.first == i) CHECK(ian_trainer_set_option(t, o.second.first.c_str(), o.second.second));
    const long c0 = g_calls;
    if (g_dump) printf("== step %d which %d\n", i, w);
    if (mode == "step") {
      CHECK(ian_train_step(t, w, X.data(), Z.data(), E.data(), B, met, nullptr));
    } else {
      CHECK(ian_trainer_forward(t, X.data(), Z.data(), E.data(), B, nullptr, nullptr, nullptr));
      CHECK(ian_trainer_metrics(t, met));
      CHECK(ian_trainer_backward(t, w));
      CHECK(ian_trainer_finish_allreduce(t, w));
      CHECK(ian_trainer_regularizers(t, w));
      CHECK(ian_trainer_apply_adam(t, w));
    }
    if (!g_dump) printf("step %d which %d: %ld calls\n", i, w, g_calls - c0);
  }
  if (g_dump) printf("== destroy\n");
  ian_trainer_destroy(t);
  return 0;
}
