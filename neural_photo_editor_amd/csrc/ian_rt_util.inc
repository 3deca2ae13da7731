// ian_rt_util.inc -- options, error text, parameter lookup, uploads.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
namespace {

// key=value tuning knobs (ian_set_option; also read once from the environment variable IAN_OPTS="k=v,k=v" when a handle
// or a training layer is created, so that tests and profiling runs can pin a schedule policy for every object)
bool apply_option(Options& o, const std::string& k, int value) {
  if (k == "tg_cfg") o.tg_cfg = value;
  else if (k == "tg_target_items") o.tg_target_items = std::max(1, value);
  else if (k == "tg_min_steps") o.tg_min_steps = std::max(1, value);
  else if (k == "tg_no_split_items") o.tg_no_split_items = value;
  else if (k == "tg_split") o.tg_split = value;
  else if (k == "tg_pos_major") { if (value < 0 || value > 2) return false; o.tg_pos_major = value; }
  else if (k == "tg_xcd_group") o.tg_xcd_group = std::max(1, value);
  else if (k == "tg_xcd_spatial") o.tg_xcd_spatial = value;
  else if (k == "tg_prefer_nosplit") o.tg_prefer_nosplit = value;
  else if (k == "tg_nosplit_min_out") o.tg_nosplit_min_out = value;
  else if (k == "tg_variant") {
    if (!tg_schedule_valid(value)) return false;   // ian_internal.h: the negative results and the timing-only variants exist in libian_ablation.so only
    o.tg_variant = value;
  }
  else if (k == "tg_variant_force") {
    if (value != -1 && !tg_schedule_valid(value)) return false;
    o.tg_variant_force = value;
  }
  else if (k == "tg_noepi") {
#ifndef IAN_ABLATION
    if (value != 0) return false;
#endif
    o.tg_noepi = value;
  }
  else if (k == "tg_fast_epilogue") o.tg_fast_epilogue = value;
  else if (k == "tg_tune_pin") o.tg_tune_pin = value;
  else if (k == "tg_tune_deep") o.tg_tune_deep = value;
  else if (k == "tg_tune_model") o.tg_tune_model = value;
  else if (k == "tg_tune_final") o.tg_tune_final = std::max(0, value);
  else if (k == "tg_reduce_kp") o.tg_reduce_kp = value;
  else if (k == "tg_bf16x3") { if (value < 0 || value > 1) return false; o.tg_bf16x3 = value; }
  else if (k == "tg_bf16x3_min_m") o.tg_bf16x3_min_m = std::max(1, value);
  else if (k == "tg_bf16x3_min_images") o.tg_bf16x3_min_images = std::max(1, value);
  else if (k == "tg_bf16x3_wsplit") o.tg_bf16x3_wsplit = value;
  else if (k == "tg_bf16x3_sched") { if (value < 0 || value > 2) return false; o.tg_bf16x3_sched = value; }
  else if (k == "tg_bf16x3_fwd") o.tg_bf16x3_fwd = value;
  else if (k == "tg_bf16x3_bwd") o.tg_bf16x3_bwd = value;
  else if (k == "tg_fuse") { if (value < 0 || value > 2) return false; o.tg_fuse = value; }
  else if (k == "tg_fuse_max_m") o.tg_fuse_max_m = value;
  else if (k == "tg_fuse_tune") { if (value < 0 || value > 2) return false; o.tg_fuse_tune = value; }
  else if (k == "mdc_head") o.mdc_head = value;
  else if (k == "head_fused") o.head_fused = value;
  else if (k == "head_fused_min_n") o.head_fused_min_n = std::max(1, value);
  else if (k == "fuse_latent_update") o.fuse_latent_update = value;
  else if (k == "edit_graph") o.edit_graph = value;
  else if (k == "edit_zero_copy") o.edit_zero_copy = value;
  else if (k == "edit_spin") o.edit_spin = value;
  else if (k == "edit_keep_warm_us") { if (value < 0 || value > 20000) return false; o.edit_keep_warm_us = value; }
  else if (k == "dec_out_mfma") o.dec_out_mfma = value;
  else if (k == "dec_out_px") o.dec_out_px = value;
  else if (k == "dense_gemv") o.dense_gemv = value;
  else if (k == "brush_pass") o.brush_pass = value < 1 ? 1 : (value > 256 ? 256 : value);
  else if (k == "session_stage_bytes") o.session_stage_bytes = std::max(1, value);
  else if (k == "b1_conv") {
#ifndef IAN_ABLATION
    if (value != 0) return false;             // batch-1 streaming deconv (kernels_b1.hip): measured slower, libian_ablation.so only
#endif
    o.b1_conv = value;
  }
  else if (k == "alias_io") o.alias_io = value;
  else if (k == "dec_out_wgs") o.dec_out_wgs = std::max(1, value);
  else if (k == "head_wgs") o.head_wgs = std::max(1, value);
  else if (k == "dec_out_bal") o.dec_out_bal = value;
  else if (k == "mdc_thin_tile") o.mdc_thin_tile = value;
  else if (k == "wg_target_items") o.wg_target_items = value;
  else if (k == "wg_xcd_split") o.wg_xcd_split = value;
  else if (k == "wg_pipe") o.wg_pipe = value;
  else if (k == "wg_reduce_tci") { if (value != 16 && value != 32) return false; o.wg_reduce_tci = value; }
  else if (k == "wg_reduce_tiled") o.wg_reduce_tiled = value;
  else if (k == "pack_tiled") o.pack_tiled = value;
  else if (k == "zbuild_rows") o.zbuild_rows = value;
  else if (k == "wg_w8") {
#ifndef IAN_ABLATION
    if (value != 1) return false;             // the 4-wave 128x128 tapwgrad tile: superseded, libian_ablation.so only
#endif
    o.wg_w8 = value;
  }
  else return false;
  return true;
}
void apply_env_options(Options& o) {
  const char* env = getenv("IAN_OPTS");
  if (!env) return;
  std::string sv(env);
  size_t pos = 0;
  while (pos < sv.size()) {
    size_t end = sv.find(',', pos);
    if (end == std::string::npos) end = sv.size();
    const std::string kv = sv.substr(pos, end - pos);
    const size_t eq = kv.find('=');
    if (eq != std::string::npos && !apply_option(o, kv.substr(0, eq), atoi(kv.c_str() + eq + 1)))
      fprintf(stderr, "libian: IAN_OPTS entry '%s' refused (unknown key, or a value that exists in libian_ablation.so only)\n", kv.c_str());
    pos = end + 1;
  }
}

int fail(ian_handle* h, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  return code;
}

// the rectangle (c1,r1)-(c2,r2) of a brush, a loss or a fit lies inside the model's image; fn != nullptr: item `item` of a batched
// call fn.  `what` is the caller's word for it ("patch", "rectangle").
int check_rect(ian_handle* h, const char* fn, int item, int c1, int r1, int c2, int r2, const char* what) {
  const Slot& out = h->slots[h->desc.out_slot];
  if (c1 >= 0 && r1 >= 0 && c2 <= out.w && r2 <= out.h) return 0;
  char where[96] = "";
  if (fn) snprintf(where, sizeof where, "%s: item %d: ", fn, item);
  return fail(h, -7, "%s%s (%d,%d,%d,%d) outside the %dx%d image", where, what, c1, r1, c2, r2, out.w, out.h);
}

#define HIPCHK(h, expr)                                                                            \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return fail(h, -2, "HIP error %s at %s:%d (%s)", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
  } while (0)

const HostTensor* find_param(ian_handle* h, const std::string& n) {
  auto it = h->params.find(n);
  return it == h->params.end() ? nullptr : &it->second;
}

int need_param(ian_handle* h, const std::string& n, std::initializer_list<int64_t> shape, const HostTensor** out) {
  const HostTensor* t = find_param(h, n);
  if (!t) return fail(h, -3, "missing parameter '%s'", n.c_str());
  std::vector<int64_t> want(shape);
  if (t->shape != want) {
    std::string a, b;
    for (auto s : t->shape) a += std::to_string(s) + ",";
    for (auto s : want) b += std::to_string(s) + ",";
    return fail(h, -3, "parameter '%s' has shape (%s) expected (%s)", n.c_str(), a.c_str(), b.c_str());
  }
  *out = t;
  return 0;
}

template <typename T>
int upload(ian_handle* h, const std::vector<T>& v, T** dptr) {
  if (v.empty()) {
    *dptr = nullptr;
    return 0;
  }
  HIPCHK(h, hipMalloc((void**)dptr, v.size() * sizeof(T)));
  HIPCHK(h, hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  ++h->alloc_epoch;
  return 0;
}

}  // namespace
