// ian_rt_types.h -- types of the runtime: packed layers, slots, op plans, options, the handle.
// Part of the libian runtime: one translation unit, included by ian_runtime.cpp in this order (see the list there).
#pragma once
namespace {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
static inline int ilog2_exact(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return ((1 << s) == v) ? s : -1;
}

struct Schedule {
  int variant = -1;
  int cfg = 0;
  int nitems = 0;
  TgItem* d_items = nullptr;
  int ntiles = 0;  // >0 => split-K: slabs + reduce pass
  TgTile* d_tiles = nullptr;
  int* d_counters = nullptr;   // split-K combine fused into the tapgemm launch: one arrival counter per tile (zero at rest)
  float* d_raw = nullptr;      // fused == 2: one accumulation tile per output tile (zero at rest)
  int fused = 0;               // how this schedule's split-K partials are combined (TgParams::fused)
  bool bf16x3 = false;         // launches go to tapgemm_bf16x3_kernel (option tg_bf16x3 and a tile it is instantiated for)
  size_t slab_tiles = 0;
  int max_nsplit = 1;
  std::vector<TgItem> h_items;  // kept for tests / debugging
  std::vector<TgTile> h_tiles;
  // row order and tap lists (ian_tg_types.h, ian_tg_plan.h): M rows; position-major schedules carry b_shift >= 0 and per-tile tap lists
  bool pos_major = false;
  int M = 0, b_shift = -1;
  long long steps = 0, steps_full = 0;   // K-steps the launch executes / would with every tile listing every tap
  TgTapE* d_ttaps = nullptr;             // the schedule's tap table (TgItem::tap0 indexes it)
  std::vector<TgTapE> h_ttaps;
};

struct TgChoice {  // autotuned (or forced) schedule shape for one (layer, batch)
  int cfg = -1;        // enum TgConfig, -1 = heuristic
  int max_steps = -1;  // -1 = heuristic, 0 = never split K, >0 = split so that no item exceeds this many K-steps
  int variant = -1;    // K-loop schedule of tapgemm_kernel, -1 = the handle's option
  int fused = -1;      // split-K combine: -1 = the handle's option (tg_fuse for small M), 0 reduce launch, 1 in-launch slabs, 2 atomics
  int pos_major = -1;  // row order: -1 = the launch model decides where option tg_pos_major admits it, 0 image-major, 1 position-major
};

// one linear map executed by the tapgemm kernel (forward or backward-data form of an op)
struct TgLayer {
  bool valid = false;
  int IH = 1, IW = 1, Cin = 32, QH = 1, QW = 1, si = 1, by = 0, bx = 0, so = 1, OH = 1, OW = 1, Cout = 0, CoutPad = 0;
  int cin_real = 0;  // for FLOP accounting
  std::vector<TgClass> classes;
  std::vector<TgTap> taps;
  std::vector<float> h_w;  // packed weights (freed after upload)
  size_t w_floats = 0;
  float* d_w = nullptr;
  unsigned short* d_wsplit = nullptr;   // d_w split into a bf16 hi plane + lo plane (2 x w_floats values) for tapgemm_bf16x3_kernel; made lazily
  bool wsplit_valid = false;            // ... and re-made after d_w changed (training layers repack their slabs after every update)
  TgClass* d_classes = nullptr;
  TgTap* d_taps = nullptr;
  std::map<int, Schedule> sched;  // per batch size
  std::map<int, TgChoice> choice;  // per batch size, set by ian_autotune
  double macs_per_image() const {
    double m = 0;
    for (auto& c : classes) m += (double)QH * QW * c.ntaps * cin_real * Cout;
    return m;
  }
};

struct Slot {
  int h = 1, w = 1, c = 1, cs = 32;
  bool nchw = false;  // external-layout tensors (image in / image out)
  float* d = nullptr;
  float* g = nullptr;  // gradient wrt the producer's pre-epilogue value (latent-brush backward)
  size_t cap = 0, gcap = 0;
  size_t per_image() const { return nchw ? (size_t)c * h * w : (size_t)h * w * cs; }
};

struct OpPlan {
  ian_op_desc d;
  std::string name, bn_name;
  TgLayer fwd, bwd;
  bool edge = false;  // 3-channel edge kernel instead of tapgemm
  float* d_edge_w = nullptr;
  std::vector<float> h_edge_w;
  float* d_scale = nullptr;
  float* d_shift = nullptr;
  std::vector<float> h_scale, h_shift;
  float* d_made_w = nullptr;
  float* d_made_b = nullptr;
  // batch-1 streaming form of a transposed conv and of its backward-data (kernels_b1.hip)
  std::vector<float> h_b1_fwd, h_b1_bwd;
  float* d_b1_fwd = nullptr;
  float* d_b1_bwd = nullptr;
  long long b1_cls_off[4] = {0, 0, 0, 0};
  long long head_done_serial = -1;  // run_serial of the call in which a sibling's fused head launch produced this op
};

struct Options {
  int tg_cfg = -1;            // force a tile config (enum TgConfig) or -1 = auto
  int tg_target_items = 768;  // split-K aims at about this many workgroups
  int tg_min_steps = 16;      // never make a K-range shorter than this many 32-channel steps
  int tg_no_split_items = 384;  // do not split when tiles alone give at least this many workgroups
  int tg_split = 1;
  int tg_pos_major = 1;       // position-major tile rows with the out-of-image taps of a tile skipped (ian_tg_plan.h): 0 off, 1 auto (batches
                              // that are a power of two >= 64, per layer where the tuner / the launch model finds it faster), 2 forced for
                              // any batch (tests).  Training layer contexts default to 0.
  int tg_xcd_group = 8;       // supergroup edge (tiles) dealt to one XCD
  int tg_xcd_spatial = 0;            // experiment (round 4, OFF): equal-weight runs of tile groups dealt to the XCDs in contiguous pieces instead of
                                     // round-robin.  Measured: same step time, HBM fetch per tapgemm launch 85 -> 122 MB at batch 64
  int tg_prefer_nosplit = 1;  // try smaller tiles before resorting to split-K
  int tg_nosplit_min_out = 1 << 30;  // outputs (M*Cout) above which 64x64 is forced even if it under-fills
  int mdc_head = 2;                  // few-filter MDCL layers: 0 = tapgemm, 1 = VALU head kernel, 2 = + sibling layers fused
  int tg_variant = 2;                // K-loop schedule of tapgemm_kernel (kernels_tapgemm.hip); autotune picks per layer
  int tg_fuse = 0;                   // split-K combine of launches with images*QH*QW <= tg_fuse_max_m (the batch-1 chains, where a reduce launch
                                     // costs as much as the K loop): 0 = separate tapgemm_reduce launch; 1 = write-through (sc1) slabs summed by
                                     // the tile's last-arriving workgroup in slice order (deterministic); 2 = float atomics into a zero-at-rest
                                     // tile + epilogue by the last arriver (run-to-run last-bit differences).  The autotuner may pick per layer.
  int tg_fuse_max_m = 1024;
  int tg_fuse_tune = 0;              // fused modes ian_autotune may try for such launches: 0 none, 1 = mode 1, 2 = modes 1 and 2.  OFF: measured on
                                     // MI355X (profiles/r05_b1_inlaunch_combine_ab.json) the autotuner kept the reduce launch for every 5x5 layer, and
                                     // the fused modes forced on untuned layers cost +13 us (mode 1) / +9 us (mode 2) per layer
  int tg_bf16x3 = 0;                 // OPT-IN, never the default: tap-GEMMs with at least tg_bf16x3_min_m rows on the bf16 matrix cores, every fp32
                                     // product as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi of split-bf16 operands with fp32 accumulation (kernels_tapgemm.hip
                                     // tapgemm_bf16x3_kernel): ~1e-5 relative error instead of exact fp32 -- inside the 1e-4 parity bar, but a different
                                     // arithmetic type, so bench.py reports it as a labelled secondary only
  int tg_bf16x3_min_m = 256;
  int tg_bf16x3_min_images = 2;      // ... and never to batch-1 launches: the interactive chains are latency-bound (no use for matrix rate), and the
                                     // brush GRADIENT is discontinuous in the forward activations (ReLU / leaky-ReLU kinks): measured, a 1e-5 forward
                                     // error flips a unit under the patch and moves dL/dz by 1e-3 on 2 of the 6 fixture patches, while split-bf16
                                     // backward-data alone stays within 1.1e-5 (scripts/exp/bf16x3_brush_debug.py)
  int tg_bf16x3_wsplit = 1;          // weights pre-split once per layer (0: split at staging like the activations)
  int tg_bf16x3_sched = 1;           // K-loop schedule of tapgemm_bf16x3_kernel (0..2, kernels_tapgemm.hip)
  int tg_bf16x3_fwd = 1, tg_bf16x3_bwd = 1;   // which epilogue modes (forward / backward-data launches) the option applies to
  int tg_tune_deep = 1;              // 1: autotune also times K-loop schedule 7 (the rotated schedule with two K-steps of loads in flight)
  int tg_tune_model = 1;             // 1: autotune also times the split limits a longest-first model of the launch ranks best (ian_rt_autotune.inc)
  int tg_tune_final = 6;             // autotune: the N fastest candidates of the first pass (5 launches each) are timed again in 3 interleaved rounds of 12 launches; 0 = first pass decides
  int tg_variant_force = -1;         // >= 0: every tapgemm launch takes this K-loop schedule, also over an autotuned choice (A/B and ablation timing: scripts/exp/tg_ablate7.py)
  int tg_noepi = 0;                  // libian_ablation.so only: tapgemm returns right after its K loop (timing-only ablation, wrong results)
  int tg_fast_epilogue = 1;          // tapgemm: the per-row / per-column epilogue (tg_store_fast) where it applies; 0 = the general form everywhere (A/B, bitwise the same)
  int tg_tune_pin = 0;               // 1: autotune also times K-loop schedule 6 (schedule 2 with its fragment reads pinned; kernels_tapgemm.hip).  OFF: measured,
                                     // 44.28 / 44.03 k reconstructions/s without vs 44.13 / 44.01 k with the candidate: no gain, 25 % more tuning time
  int tg_reduce_kp = 4;              // split-K reduce: lanes sharing one output element's slabs when a tile has >= 8 slabs
  int wg_w8 = 1;                     // tapwgrad: 8-wave 128x128 workgroups (16 waves per CU instead of 8)
  int wg_reduce_tci = 16;            // tiled split reduce / repack: channels per tile row (16: 64-byte runs; 32: 128-byte runs, half the filters per tile)
  int wg_pipe = 3;                   // tapwgrad: the software-pipelined K loop of the 8-wave tile (tapwgrad_p_kernel; 0 = the compiler-scheduled loop, bitwise the same)
  int zbuild_rows = 1;               // head6 backward: Z built a pixel row at a time through LDS (head6_zbuild_rows_kernel; 0 = per (pixel, tap), same bytes)
  int pack_tiled = 1;                // training layers repack their slabs after an update through LDS tiles (pack_tiled_kernel; 0 = the gather, same bytes)
  int wg_reduce_tiled = 1;           // tapwgrad's split reduce scatters to the reference layout through LDS (wgrad_reduce_tiled_kernel; 0 = the gather, bitwise the same)
  int wg_xcd_split = 1;              // tapwgrad: all items of one pixel range go to one XCD (its rows are fetched into that L2 once), split count a
                                     // multiple of 8 (round 5); 0 = round 4's (split, tap) order
  int wg_target_items = 1024;        // tapwgrad: split the pixel range until taps x channel tiles x splits reaches this many workgroups
  int dec_out_bal = 1;               // dec_out (Cout = 3) on 16 x 16 MFMA blocks, five per SIMD (deconv_small_kernel<3, true>); 0 = the 32 x 32 tiling (six of eight waves)
  int mdc_thin_tile = 1;             // thin MDCL (G_b / B_b and their backward-data) with the input rows staged through LDS
  int b1_conv = 0;                   // batch-1 transposed convs and their backward-data as whole-contraction streaming launches
                                     // (kernels_b1.hip).  OFF: measured slower than tapgemm + reduce (brush event 0.178 vs 0.160 ms):
                                     // 16-pixel tiles re-read weights and input rows from L2 at 4 FLOP/B
  int dec_out_wgs = 256;             // image-producing deconv: split images into row bands until this many workgroups exist (ian_row_bands.h)
  int head_wgs = 256;                // RGB-Beta head (head6_kernel, inference and ian_layer_head6_forward): the same, 1 / 2 / 4 / 8 bands per image
  int alias_io = 1;                  // ian_reconstruct: device-pointer images are read / written in place (no boundary copies)
  int dense_gemv = 1;                // batch-1 backward of the dense layer fed by the latent as one GEMV launch
  int dec_out_px = 1;                // ... and, below that batch, 8 lanes per output pixel instead of 16 tile workgroups
  int dec_out_mfma = 1;              // image-producing deconv (IAN_simple dec_out) on the matrix cores for batches >= 4
  int brush_pass = 256;              // ian_grad_batch / ian_brush_step_batch: items per forward / backward / forward pass (A/B)
  int session_stage_bytes = 64 << 20; // ian_session_save / _load with a host body: bytes of records per gather-then-copy pass (never less than one record)
  int fuse_latent_update = 1;        // ian_brush_step: the latent update rides in the epilogue of the latent's backward GEMV (round 5)
  int edit_graph = 1;                // batch-1 host-pointer calls (the NPE edit loop) replay captured hipGraphs
  int edit_spin = 1;                 // ... and their final wait polls the stream (hipStreamQuery) before it falls back to hipStreamSynchronize
  int edit_keep_warm_us = 0;         // EXPERIMENT (off): after a brush event a one-wave kernel keeps the interactive stream's queue busy for up to
                                     // this many microseconds, released by the next call (kernels_npe.hip keep_warm_kernel)
  int edit_zero_copy = 1;            // their kernels read the brush rectangle from / write z, dz, the image to the pinned block directly
  int head_fused = 1;                // RGB-Beta head as head6 + head_tail (kernels_head.hip) when the graph matches IAN.py:183-207
  int head_fused_min_n = 8;          // ... for batches of at least this many images (the latent brush's batch-1 backward
                                     // needs the per-layer activations of the unfused ops)
};

// IAN.py:183-207 recognised in the lowered decoder: op indices of R, G_a, G_b, B_a, B_b, the [R,G] concat and the beta op
struct HeadPlan {
  bool searched = false, valid = false;
  int opR = -1, opGa = -1, opGb = -1, opBa = -1, opBb = -1, opCat = -1, opBeta = -1, first = -1;
  int* d_itab = nullptr;
  float* d_ftab = nullptr;
  float* d_comp = nullptr;
  size_t comp_cap = 0;
  int halo = 0;
};

}  // namespace

struct ian_handle {
  ian_model_desc desc;
  std::vector<OpPlan> ops;
  std::vector<Slot> slots;
  std::vector<std::string> strings;
  std::map<std::string, HostTensor> params;
  std::vector<float> made_masks[3];
  int made_n = 0;
  bool finalized = false;
  Options opt;
  std::string err;
  // workspaces
  float* d_slab = nullptr;
  size_t slab_cap = 0;
  float* d_stage_in = nullptr;
  size_t stage_in_cap = 0;
  float* d_stage_out = nullptr;
  size_t stage_out_cap = 0;
  float* d_gseed = nullptr;  // 3*H*W gradient seed (n*3*H*W after a batched brush call)
  size_t gseed_cap = 0;
  float* d_rgb = nullptr;
  // decoder-forward cache for the interactive loop (NPE.py:205,218: imgradRGB(z) right after sample_at(z)):
  // the batch-1 decoder activations of the last HOST latent are kept; a gradient call on the same latent skips
  // its forward pass.  Any other use of the decoder slots invalidates it.
  long long run_serial = 0;  // incremented per executed segment (fused head bookkeeping)
  std::map<int, char> slot_stale;  // external-layout slots whose own buffer was bypassed by a device-pointer call (SlotAlias)
  std::map<int, char> slot_aliased;  // ... and which of them are bound to a caller's buffer right now
  std::vector<float> dec_cache_z;
  std::vector<float> rgb_cache;  // host copy of the brush image last uploaded to d_rgb
  // NPE.paint photo blend (ian_photo_blend): device copies of RECON / ERROR with their host shadows, outputs
  unsigned char* d_recon = nullptr;
  float* d_error = nullptr;
  unsigned char* d_im = nullptr;
  double* d_mask = nullptr;
  std::vector<unsigned char> recon_cache;
  std::vector<float> error_cache;
  unsigned char* d_u8 = nullptr;
  size_t u8_cap = 0;
  bool dec_cache_valid = false;
  HeadPlan head;
  // Interactive loop (NPE.py:192-235): batch-1 calls with HOST pointers on the default stream run on an internal stream
  // and, from the third call on, replay a captured hipGraph (decoder forward; backward chain per loss kind), removing
  // the ~15 launches x 3-4 us of host launch time per call.  alloc_epoch counts (re)allocations of anything a captured
  // kernel argument may point to; a graph captured under an older epoch is dropped and re-captured.
  struct EditGraph {
    hipGraphExec_t exec = nullptr;
    long long epoch = -1;
    int warm = 0;
    long long warm_epoch = -1;   // the eager pass counts only for the options / schedules / buffers it ran with
    bool mirrors = false;        // its image kernel writes the pinned image as well (zero-copy): no device -> host copy needed
  };
  long long alloc_epoch = 0;
  hipStream_t edit_stream = nullptr;
  float* pin = nullptr;      // pinned host block: z [0,128) | dz [128,256) | image [256, 256+12288) | patch (4 ints) after that
  // Round 4: the block is allocated mapped + coherent and the kernels of the interactive graphs read the brush rectangle from it
  // and write the new latent, the gradient and the image into it directly (pin_dev = its device address; nullptr: not
  // available, the graphs keep their copy nodes).  Every hipMemcpyAsync of a graph is a 4.6 us copy kernel plus a kernel
  // boundary on this runtime: four of them per brush event.
  float* pin_dev = nullptr;
  // training step (ian_layer_stats_next): the NEXT tap-GEMM launch through this context also produces the batch statistics of
  // the tensor it stores (TgStats); one-shot.  stats_chunks_last = partial rows the last launch wrote (0: it could not -- split-K
  // schedule, VALU path, workspace too small -- and the caller runs colstats instead)
  TgStats stats_next;
  long long stats_cap = 0;       // doubles available at stats_next.partial
  int stats_chunks_last = 0;
  float* out_mirror = nullptr;   // set around run_segment(DEC): the batch-1 image kernel also writes the image there
  // several editors (ian_grad_batch / ian_brush_step_batch): the device copy of the ian_brush_item table, the brush colour images,
  // RECON / ERROR (each with the host shadow of its last upload), staging for host outputs, and the resident-activation cache:
  // bcache_z = the n latents the decoder activations belong to; enter_stream (every other call) clears bcache_valid
  struct BatchState {
    int* d_items = nullptr;
    std::vector<int32_t> items_shadow;
    float* d_rgb = nullptr;
    size_t rgb_cap = 0;
    std::vector<float> rgb_cache;
    unsigned char* d_recon = nullptr;
    size_t recon_cap = 0;
    std::vector<unsigned char> recon_cache;
    float* d_error = nullptr;
    size_t error_cap = 0;
    std::vector<float> error_cache;
    float* d_out = nullptr;           // z_new rows | dz rows, packed (n * zl each)
    size_t out_cap = 0;
    unsigned char* d_im = nullptr;
    size_t im_cap = 0;
    double* d_mask = nullptr;
    size_t mask_cap = 0;
    std::vector<float> cache_z;
    int cache_n = 0;
    bool cache_valid = false;
  } batch;
  // device-resident edit sessions (ian_session_*, ian_rt_session.inc): the pool (one row per session id in each array), what the
  // host keeps per session (opened, latent version), the small per-call uploads, and the residency key of ian_session_brush: the
  // decoder activations belong to sessions res_ids, in that order, at latent versions res_ver; enter_stream clears res_valid.
  // The device buffers beside the pool, as plain data: SESS_SCRATCH (ian_rt_session.inc) names each once, with the reservation that
  // owns it and its size; nothing else allocates or frees them.
  struct SessionScratch {
    int* d_tab = nullptr;              // per call: open / set_latent = n ids, ian_canvas_place = [n ids | 5n placement words], ian_place_oriented = [n ids | 6n]
    float* d_tanh = nullptr;           // to_tanh of the 256 uint8 levels, float32
    unsigned char* d_photo = nullptr;  // staging of host photos [256][3*64*64], allocated by the first open that needs it
    unsigned char* d_shown = nullptr;  // staging of the canvas images [256][3*64*64]
    int* d_views = nullptr;            // full-resolution: per call n ian_session_view records
    unsigned char* d_out = nullptr;    // full-resolution: staging of rendered windows for a host `out`, grown on demand (out_cap)
    float* d_guide = nullptr;          // full-resolution: f32[766], the range weights of ian_sessions_reserve_guide; nullptr = no guide, the plain bilinear render
    double* d_falloff = nullptr;       // local edits: f64[64], the table of ian_sessions_set_local
    int* d_ltab = nullptr;             // local edits: per ian_session_local call [n ids | n flags]
    int* d_htab = nullptr;             // undo history: per ian_session_mark / _undo call [n ids | n save slots | n load slots]
    int* d_rtab = nullptr;             // saved sessions: per ian_session_save / _load call n x (id, has_source, ring base, history length); by the first such call
    unsigned char* d_stage = nullptr;  // saved sessions: staging of records for a host `body`, grown on demand (stage_cap) up to opt.session_stage_bytes
    float* d_fit = nullptr;            // ian_session_fit: Adam's moments of one pass, m [256][zl] then v [256][zl]; by the first such call
    double* d_fit_loss = nullptr;      // ian_session_fit: staging of the loss trace for a host `loss`, [256][513]; by the first call that asks for one
    int* d_stab = nullptr;             // brush, clone, stroke and fit calls: the call's table, laid out by EditTable (ian_edit_plan.h), grown on demand (stab_cap words)
    float* d_tips = nullptr;           // brush tips: f32[tip_count][64 * 64], row stride 64 (ian_sessions_reserve_tips / _set_tip); nullptr = no tips
    double* d_tip_shape = nullptr;     // brush tips: f64[tip_count][64 * 64], the tips' shapes wn / max wn (tip_shape_slot) for the tip-shaped footprint; with d_tips
  };
  struct SessionState : SessionScratch {
    int capacity = 0;
    struct SessionArrays {             // every device array SESS_COLUMNS describes: the pool the kernels take, and the history's rings
      SessionPool pool;
      SessionRings rings;
    };
    SessionArrays arr = {};
    std::vector<char> opened;
    std::vector<uint64_t> version;
    std::vector<int32_t> tab_shadow;   // upload source of d_tab (outlives the caller's array)
    double w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int radius = -1;                   // -1: ian_sessions_set_blend has not been called
    int pixels = 0;                    // the pixel format of every window call's out (ian_sessions_set_pixels; PIXELS_*); ian_sessions_reserve(0): planar again
    std::vector<int32_t> res_ids;
    std::vector<uint64_t> res_ver;
    bool res_valid = false;
    // full-resolution sessions (ian_sessions_reserve_hires): per session whether SRC holds a photo
    std::vector<char> has_src;
    std::vector<int32_t> views_shadow;   // upload source of d_views
    size_t out_cap = 0;
    // local edits (ian_sessions_reserve_local): the host's copy of every session's LOCAL flags (what the device array holds: only
    // ian_session_local writes either), whether the falloff table is set, and the dampen threshold of ian_sessions_set_local
    std::vector<char> local_flags;
    bool falloff_set = false;
    double dampen_thresh = 0.75;
    std::vector<int32_t> ltab_shadow;    // upload source of d_ltab
    // undo history (ian_sessions_reserve_history): per session the list of saved states and the cursor (ian_session_history.h); the
    // depth is arr.rings.depth.  The host is the only owner of these counters.
    std::vector<SessionHistory> hist;
    std::vector<int32_t> htab_shadow;    // upload source of d_htab
    // saved sessions (ian_session_save / ian_session_load)
    std::vector<int32_t> rtab_shadow;    // upload source of d_rtab
    size_t stage_cap = 0;
    // the table of a brush, clone, stroke or fit call
    std::vector<int32_t> stab_shadow;    // upload source of d_stab
    size_t stab_cap = 0;
    // brush tips (ian_sessions_reserve_tips): how many d_tips holds and per tip its (tw, th), (0, 0) until ian_sessions_set_tip gave it
    // weights.  Per handle, not per session: no record, history or canvas knows of them.
    int tip_count = 0;
    std::vector<int32_t> tip_wh;
    bool tip_footprint = false;          // ian_sessions_set_soft_mask: a tipped paint event leaves its tip's shape in UMASK, not its rectangle's
    // canvases (ian_sessions_reserve_canvas, ian_rt_canvas.inc): the device arrays, per canvas the size of its picture (0 x 0: never
    // put), per session where it is placed (canvas -1: nowhere; sized with the pool while canvases exist, empty otherwise), and the
    // host's copy of the device table (canv.table), from which a canvas's 8 entries are uploaded whenever they change
    SessionCanvases canv = {};
    std::vector<int32_t> canvas_wh;
    std::vector<ian_canvas_placement> placed;
    std::vector<int32_t> ctab_shadow;
    std::vector<char> cdirty;            // per canvas: the device table lags behind ctab_shadow
    int* d_cwin = nullptr;               // per ian_canvas_compose / _brush / _commit call n ian_canvas_window records
    std::vector<int32_t> cwin_shadow;    // upload source of d_cwin
    float* d_edges = nullptr;            // f32[766], the range weights of ian_sessions_reserve_edges; nullptr = the plain compose.  Goes with the canvases
    // oriented placements (ian_place_oriented): per session where it is placed in that form (canvas -1: nowhere;
    // sized with `placed`, a session is in at most one of the two), the canvases' second device table int[count][8][8], allocated
    // by the first oriented place of a reservation and freed with the canvases, its host copy and per canvas whether it lags
    std::vector<ian_canvas_oriented> oplaced;
    int* d_otab = nullptr;
    std::vector<int32_t> otab_shadow;
    std::vector<char> odirty;
  } sess;
  bool warm_armed = false;       // a keep_warm_kernel is (or may still be) spinning on edit_stream: enter_stream releases it
  bool pin_img_valid = false;    // pin[PIN_IMG..] holds the image that is resident in the output slot
  int* d_patch = nullptr;
  bool keep_layer_acts = false;   // set around the forward passes of ian_grad_batch / ian_brush_step_batch: no fused RGB-Beta head
  EditGraph g_fwd, g_bwd[2], g_step[2][2];   // g_step[mode][image wanted]: backward + latent update + forward (ian_brush_step)
  bool graph_failed = false;
  hipStream_t last_stream = nullptr;   // stream of the last call that left work un-synchronised (or nullptr)
  bool last_pending = false;
  // profiling
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_total;
  size_t ev_total_used = 0;
  double prof_flops = 0;
  int64_t prof_launches = 0;
};

