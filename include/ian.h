/* ian.h -- C ABI of libian.so: the MI355X-native IAN compute path.
 *
 * The reference (ajbrock/Neural-Photo-Editor) has no FFI: its hot path is the
 * plat-style Python class API.py:11-110, whose methods call Theano functions
 * compiled from Lasagne graphs (IAN_simple.py:56-241, IAN.py:67-228) built out
 * of layers.py's custom ops.  This header is what a binding for that path binds
 * (ctypes stub: INTEGRATION.md; the shipped host class is
 * neural_photo_editor_amd/api.py).  Every entry point names the reference
 * interface it replaces.
 *
 * Conventions
 *   - plain C types only; no torch / numpy types cross this boundary;
 *   - every buffer is caller-owned; a pointer may be host or device memory
 *     (detected with hipPointerGetAttributes); the library owns weights,
 *     activations and workspaces;
 *   - external tensor layout is the reference's: float32, C-contiguous, NCHW
 *     images in [-1,1] (API.py:80-88); NHWC is internal only;
 *   - return 0 on success, negative on error; ian_last_error() gives the text;
 *   - one handle per device, not thread-safe, all work ordered on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).  Calls with
 *     host output pointers synchronise the stream before returning.
 */
#ifndef IAN_H_
#define IAN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ian_handle ian_handle;

/* Fused op kinds the host lowers a Lasagne-style graph to. */
enum ian_op_kind {
  IAN_OP_CONV5S2 = 1,   /* Conv2D(DNN)Layer 5x5 stride 2 pad 2, flip_filters=False: IAN_simple.py:73-116, IAN.py:71-110 */
  IAN_OP_DECONV5S2 = 2, /* layers.py:436-483 DeconvLayer (== TransposedConv2DLayer branch IAN_simple.py:182-223) */
  IAN_OP_MDC3 = 3,      /* layers.py:207-258 MDCL: shared-W multiscale dilated 3x3 */
  IAN_OP_DENSE = 4,     /* lasagne DenseLayer: IAN_simple.py:117-135, IAN.py:114-134 */
  IAN_OP_AFFINE = 5,    /* stand-alone BatchNorm(+nonlinearity) on a tensor: layers.py:412 (bnorm0) */
  IAN_OP_MADE_IAF = 6,  /* MADE x2 + IAFLayer: IAN.py:127-128, layers.py:641-650,735-853 */
  IAN_OP_BETA = 7,      /* layers.py:397-408 beta_layer x3 + concat: IAN.py:207 */
  IAN_OP_CONCAT = 8     /* ConcatLayer on channels: IAN.py:201 */
};

/* lasagne.nonlinearities used by the configs */
enum ian_act {
  IAN_ACT_NONE = 0,
  IAN_ACT_RELU = 1,
  IAN_ACT_LRELU = 2, /* LeakyRectify(0.2) */
  IAN_ACT_ELU = 3,
  IAN_ACT_TANH = 4,
  IAN_ACT_SIGMOID = 5
};

/* Which compiled function of API.py / sample_IAN.py an op belongs to. */
enum ian_segment {
  IAN_SEG_ENC = 0, /* l_in -> l_Z_IAF (== l_Z for IAN_simple): Zfn, sample_IAN.py:90 */
  IAN_SEG_IAF = 1, /* l_Z_IAF -> l_Z: Z_IAF_fn, sample_IAN.py:93 */
  IAN_SEG_DEC = 2  /* l_Z -> l_out: X_hat_fn, API.py:46-47 */
};

#define IAN_MAX_SCALES 4

typedef struct ian_op_desc {
  int32_t kind;    /* enum ian_op_kind */
  int32_t segment; /* enum ian_segment */
  int32_t src;     /* input tensor slot */
  int32_t src2;    /* second input: residual added BEFORE the affine (ElemwiseSumLayer, layers.py:412),
                      second/third tensor for BETA / CONCAT; -1 if none */
  int32_t src3;    /* third input (BETA); -1 if none */
  int32_t dst;     /* output tensor slot */
  int32_t cin, cout;  /* channels (DENSE: in / out features) */
  int32_t in_h, in_w; /* input spatial extent (DENSE: 1,1) */
  int32_t act;        /* enum ian_act applied after bias / batch-norm */
  int32_t has_bias;   /* parameter "<name>.b" exists */
  /* DENSE only: the reference flattens (C,H,W) row-major (App. B.6) while the
     internal layout is (H,W,C); non-zero triplets make finalize permute the
     weight rows / columns so no data movement happens at run time. */
  int32_t flat_c, flat_h, flat_w;       /* input was a (C,H,W) map   */
  int32_t unflat_c, unflat_h, unflat_w; /* output is reshaped to (C,H,W): ReshapeLayer IAN_simple.py:136 */
  int32_t n_scales;                     /* MDC3: len(scales) */
  int32_t scales[IAN_MAX_SCALES];       /* MDC3: scales (0 = the 1x1 mean branch) */
  const char* name;    /* Lasagne layer name. Parameters are looked up as "<name>.W"/"<name>.b"
                          (MDC3: "<name>W", "<name>_coeff_base", "<name>_coeff_1x1", "<name>_coeff_<s>";
                          MADE_IAF: "<name>_{mu,ls}_{input,output_W,output_D}.{W,b}") -- SURVEY App. B.5 */
  const char* bn_name; /* BatchNormLayer name ("<bn>.gamma|beta|mean|inv_std") or NULL */
} ian_op_desc;

typedef struct ian_slot_desc {
  int32_t h, w, c; /* logical NHWC extent per image */
} ian_slot_desc;

typedef struct ian_model_desc {
  int32_t n_ops;
  const ian_op_desc* ops; /* topologically ordered */
  int32_t n_slots;
  const ian_slot_desc* slots;
  int32_t x_slot;      /* l_in  (n,3,64,64)                       */
  int32_t zpre_slot;   /* l_Z_IAF: encoder mean, before the IAF   */
  int32_t z_slot;      /* l_Z: what the decoder consumes (== zpre_slot when there is no IAF) */
  int32_t out_slot;    /* l_out (n,3,64,64)                       */
  int32_t num_latents; /* cfg['num_latents'] (API.py:92-96)       */
  int32_t deconv_flip; /* 1: DeconvLayer is the gradient of a true convolution */
} ian_model_desc;

/* API.py:12-21: build the model for a config (the graph arrives already lowered). */
int ian_create(const ian_model_desc* desc, ian_handle** out);
/* GANcheckpoints.py:33-57 load_weights: one call per npz entry, Theano parameter names. Host pointer. */
int ian_load_param(ian_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* layers.py:831-853 MADE.reset("Once") result (API.py:33-36): 0/1 masks, (in,out) row-major, shared by both MADEs. */
int ian_set_made_masks(ian_handle* h, const float* m0, const float* m1, const float* md, int32_t n);
/* Ends API.py:23-36: fold batch-norm statistics, repack weights for the kernels, upload. */
int ian_finalize(ian_handle* h);

/* API.py:78-90 encode_images -> Z_hat_fn (API.py:50-51).  x f32[n,3,64,64] -> z f32[n,num_latents] */
int ian_encode(ian_handle* h, const float* x, int32_t n, float* z, void* stream);
/* API.py:98-110 sample_at -> X_hat_fn (API.py:46-47).     z f32[n,num_latents] -> x f32[n,3,64,64] */
int ian_decode(ian_handle* h, const float* z, int32_t n, float* x, void* stream);
/* sample_IAN.py:90-91 Zfn: x -> l_Z_IAF (deterministic mean) */
int ian_encode_pre_iaf(ian_handle* h, const float* x, int32_t n, float* z, void* stream);
/* sample_IAN.py:93-94 Z_IAF_fn: l_Z_IAF -> l_Z */
int ian_iaf(ian_handle* h, const float* zpre, int32_t n, float* z, void* stream);
/* encode followed by decode with the latent kept on the device (bench config 2: reconstruction). */
int ian_reconstruct(ian_handle* h, const float* x, int32_t n, float* xhat, void* stream);

/* API.py:72-76,64 imgradRGB: d mean((X_hat[0,:,r1:r2,c1:c2]-RGB[0,:,r1:r2,c1:c2])^2) / dZ.
   rgb f32[1,3,64,64], z f32[1,num_latents] -> dz f32[1,num_latents] */
int ian_grad_rgb(ian_handle* h, int32_t c1, int32_t r1, int32_t c2, int32_t r2, const float* rgb, const float* z,
                 float* dz, void* stream);
/* API.py:66-70,59 imgrad: d mean(X_hat[0,:,r1:r2,c1:c2]) / dZ */
int ian_grad_light(ian_handle* h, int32_t c1, int32_t r1, int32_t c2, int32_t r2, const float* z, float* dz,
                   void* stream);

/* ---- the steps NPE.py runs right after the hot path on every edit, chained after the decoder ---- */
/* NPE.py:110,261 (update_photo, RECON): np.uint8(from_tanh(sample_at(z))) -> out u8[n,3,64,64]; the float image stays
   on the device, 12 KB per image cross the bus.  Bare cast as in the reference: truncation toward zero, modulo 256. */
int ian_decode_u8(ian_handle* h, const float* z, int32_t n, uint8_t* out, void* stream);
/* NPE.py:218-231 (NPE.paint, photo mode), for the latent z (f32[1,num_latents]):
     DELTA = sample_at(z)[0] - to_tanh(float32(RECON))
     MASK  = scipy.ndimage.gaussian_filter(min(mean_c |DELTA|, 1), sigma)          float64, 'reflect', truncate 4
     IM    = uint8(from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR))
   recon u8[3,64,64], error f32[3,64,64] (host or device; host copies are re-uploaded only when their bytes change),
   gauss_half f64[radius+1] = scipy's normalised 1-D Gaussian from the centre outwards (the host computes it exactly as
   scipy does: npe_ops.gaussian_half_kernel), radius <= 7.  im u8[3,64,64]; mask f64[64,64] or NULL.  Bit-exact with the
   numpy/scipy expression (tests/test_gpu_npe.py).  Reuses the decoder activations of the last ian_decode /
   ian_grad_* call on the same host latent. */
int ian_photo_blend(ian_handle* h, const float* z, const uint8_t* recon, const float* error, const double* gauss_half,
                    int32_t radius, uint8_t* im, double* mask, void* stream);

/* One whole brush event of NPE.paint / NPE.scroll (NPE.py:199-218, 305-316) in ONE call, one graph replay, one
   synchronisation -- instead of imgradRGB + host update + sample_at (two round trips):
     dZ    = rgb ? imgradRGB(c1,r1,c2,r2, rgb, z) : imgrad(c1,r1,c2,r2, z)        (API.py:66-76)
     z_new = z + coef * (dZ * gscale)        float32, each product rounded on its own, in this order -- NPE.py:205-209
             "grad = temp*(1+(x2-x1)); Z -= weight*grad" is coef = -weight, gscale = 1+(x2-x1); NPE.py:313-314 is
             coef = sign*weight -- bit-identical to the numpy expression on a float32 Z
     x     = sample_at(z_new)                                                       (API.py:98-110)
   z, z_new f32[num_latents] (host; may alias), dz f32[num_latents] or NULL, x f32[3,64,64] or NULL (the decoder runs either
   way: its activations stay resident for the next event), photo = NULL or the arguments of ian_photo_blend, applied to
   sample_at(z_new) in the same submission (photo mode, NPE.py:218-231).  rgb f32[1,3,64,64] host or device.
   Falls back to the composition of the public calls when the captured-graph path is not available. */
typedef struct ian_photo_args {
  const uint8_t* recon;       /* u8[3,64,64] */
  const float* error;         /* f32[3,64,64] */
  const double* gauss_half;   /* f64[radius+1] */
  int32_t radius;
  uint8_t* im;                /* out u8[3,64,64] */
  double* mask;               /* out f64[64,64] or NULL */
} ian_photo_args;
int ian_brush_step(ian_handle* h, int32_t c1, int32_t r1, int32_t c2, int32_t r2, const float* rgb, const float* z, float coef,
                   float gscale, float* z_new, float* dz, float* x, const ian_photo_args* photo, void* stream);

/* ---- several editors on one device: n independent brush events in one submission (1 <= n <= 256) ----
   Item i is exactly one single-image call on (z[i], items[i], rgb[i]): the decoder runs per sample, rows do not couple.
   An empty rectangle (c2 <= c1 or r2 <= r1) gives a zero gradient; a rectangle outside the image fails the whole call
   with -7 (the message names the item) before anything is written.  items is a host array. */
typedef struct ian_brush_item {
  int32_t c1, r1, c2, r2;   /* API.py:66-76 rectangle, columns first as in imgrad */
  int32_t mode;             /* 1: imgradRGB against rgb[i]; 0: imgrad (lighten / darken) */
  float coef, gscale;       /* z_new = z + coef * (dz * gscale); ignored by ian_grad_batch */
} ian_brush_item;

/* n latents' brush gradients in one submission. rgb f32[n,3,64,64] (rows of mode-0 items are not read) or NULL when
   no item has mode 1; z f32[n,zl]; dz f32[n,zl].  Host or device pointers, like the single-image calls. */
int ian_grad_batch(ian_handle* h, int32_t n, const ian_brush_item* items, const float* rgb, const float* z, float* dz,
                   void* stream);

typedef struct ian_photo_batch_args {
  const uint8_t* recon;       /* u8[n,3,64,64] */
  const float* error;         /* f32[n,3,64,64] */
  const double* gauss_half;   /* f64[radius+1], shared; host memory */
  int32_t radius;             /* 0..7 */
  uint8_t* im;                /* out u8[n,3,64,64] */
  double* mask;               /* out f64[n,64,64] or NULL */
} ian_photo_batch_args;

/* n brush events (gradient + update + decoder [+ blend]) in one submission, one synchronisation.
   z_new f32[n,zl] (may alias z), dz f32[n,zl] or NULL, x f32[n,3,64,64] or NULL, photo NULL or as above.
   When z is byte for byte the z_new the previous call of this function left resident (same n, no other call in
   between), the forward at z is skipped (IAN_NO_DEC_CACHE switches that off). */
int ian_brush_step_batch(ian_handle* h, int32_t n, const ian_brush_item* items, const float* rgb, const float* z,
                         float* z_new, float* dz, float* x, const ian_photo_batch_args* photo, void* stream);

/* ---- device-resident edit sessions: the state of NPE.py's globals (GIM, IM, RECON, ERROR, Z, SAMPLE_FLAG) per editor, in
   device memory, addressed by session id ----
   A handle owns a pool of `capacity` sessions; a session is GIM, IM, RECON u8[3,64,64], ERROR f32[3,64,64], Z f32[num_latents] and
   a mode flag (0 = photo, 1 = sample), about 85 KB.  The caller chooses ids in 0..capacity-1 (no allocator); opening an id again
   overwrites it.  Every call takes 1 <= n <= 256 sessions in ONE submission on the caller's stream, on the batched path at any
   n; ids / events are host arrays.  Everything is checked before anything is enqueued or written: an id outside the pool, a
   session that was not opened (brush, set_latent, re-open from stored state), the same session twice in one call, a rectangle
   outside the image, a mode outside {0,1} or n outside 1..256 return -7 with a message that names the item, and no session
   changes.  Models whose image is not 3x64x64 return -7.  The captured-graph ian_brush_step stays the lowest-latency path for
   ONE editor; session calls invalidate its decoder cache and the resident activations of ian_brush_step_batch. */

/* Allocate the pool (0 frees it; growing or shrinking keeps the sessions whose ids remain).  Synchronises the device. */
int ian_sessions_reserve(ian_handle* h, int32_t capacity);
/* The photo blend's Gaussian for every later session call, as in ian_photo_batch_args: gauss_half f64[radius+1] (host; the
   host computes it exactly as scipy does: npe_ops.gaussian_half_kernel), radius 0..7.  NPE.py:224 is sigma 0.7, radius 3.
   ian_session_brush and ian_session_set_latent with as_sample = 0 return -6 until it was called. */
int ian_sessions_set_blend(ian_handle* h, const double* gauss_half, int32_t radius);

/* NPE.py:239-274 infer (photos given), :330-340 Reset (photos NULL, source 0: from the stored GIM), :342-345 UpdateGIM (photos
   NULL, source 1: GIM := IM first) for n sessions.  photos u8[n,3,64,64], host or device (4-byte aligned).  Per session
     Z     = encode_images(np.asarray([to_tanh(GIM)], dtype=np.float32))     float64 to_tanh, one rounding: NPE.py:257
     RECON = np.uint8(from_tanh(sample_at(Z)))                               NPE.py:261
     ERROR = to_tanh(np.float32(GIM)) - to_tanh(np.float32(RECON))           float32: NPE.py:264
     IM = GIM, mode = photo (SAMPLE_FLAG = 0)
   with the encoder and decoder run exactly as ian_encode / ian_decode_u8 run them at batch n (bitwise their Z and RECON);
   the uint8 photo is what crosses the bus, not a 48 KB float image.  shown u8[n,3,64,64] (host or device) or NULL receives IM. */
int ian_session_open(ian_handle* h, int32_t n, const int32_t* ids, const uint8_t* photos, int32_t source, uint8_t* shown,
                     void* stream);
/* z f32[n,num_latents], host or device.
   as_sample = 1: NPE.py:317-327 sample with the caller's z (the reference draws it with numpy; that stays on the host):
     Z := z; RECON := np.uint8(from_tanh(sample_at(z))); ERROR := to_tanh(np.float32(IM)) - to_tanh(np.float32(RECON));
     mode := sample; shown = RECON.
   as_sample = 0: NPE.py:286-302 paint_latents: Z := z; shown = the photo blend of sample_at(z) against RECON / ERROR in photo
     mode, np.uint8(from_tanh(sample_at(z))) in sample mode; the stored IM is not changed (IM is local to that callback). */
int ian_session_set_latent(ian_handle* h, int32_t n, const int32_t* ids, const float* z, int32_t as_sample, uint8_t* shown,
                           void* stream);

typedef struct ian_session_event {
  int32_t session;          /* id in the pool */
  int32_t c1, r1, c2, r2;   /* API.py:66-76 rectangle; an empty one gives a zero gradient */
  int32_t mode;             /* 1: imgradRGB toward the constant colour rgb (NPE.py:205 myRGB); 0: imgrad (NPE.py:311) */
  float coef, gscale;       /* Z := Z + coef * (dZ * gscale), the expression of ian_brush_step_batch */
  float rgb[3];             /* the brush colour in tanh space: np.float32(to_tanh(np.float32(level))) per channel */
} ian_session_event;

/* NPE.py:192-235 paint / :305-316 scroll for n sessions: per event, on the session's state, the brush gradient (against the
   constant colour for mode 1), Z := Z + coef * (dZ * gscale), x = sample_at(Z); then what the callback displays:
     mode 1 on a session in photo mode: the NPE.py:218-231 blend against the session's RECON / ERROR, written to its IM and to
       shown[i];
     a session in sample mode, and mode 0 in either mode (NPE.scroll ends in update_photo(None)): shown[i] =
       np.uint8(from_tanh(x)), IM untouched.
   Bitwise what ian_brush_step_batch gives for the same latents, boxes and constant-colour rgb images in the same order.
   Host -> device: the event table (11 words per event); device -> host: shown (u8[n,3,64,64], host or device, or NULL).
   The forward at Z is skipped when the decoder's activations were left by the previous ian_session_brush for the same
   ids in the same order at the same latent versions, with no other call in between (IAN_NO_DEC_CACHE switches that off). */
int ian_session_brush(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, void* stream);

enum ian_session_field {
  IAN_SESSION_Z = 0,     /* f32[num_latents] */
  IAN_SESSION_RECON = 1, /* u8[3,64,64] */
  IAN_SESSION_ERROR = 2, /* f32[3,64,64] */
  IAN_SESSION_IM = 3,    /* u8[3,64,64] */
  IAN_SESSION_GIM = 4,   /* u8[3,64,64] */
  IAN_SESSION_MODE = 5,  /* int32: 0 photo, 1 sample */
  /* full-resolution pools only (-6 without ian_sessions_reserve_hires) */
  IAN_SESSION_FIELD = 6,      /* f32[3,64,64]: what the last call displayed, see ian_session_render */
  IAN_SESSION_FIELD_KIND = 7, /* int32: 0 = FIELD is an edit field on top of the source, 1 = FIELD is the sample x itself */
  IAN_SESSION_SOURCE = 8,     /* u8[3,S,S]: the raw full-resolution source (-7 for a session without one) */
  /* pools with the local reservation only (-6 without ian_sessions_reserve_local) */
  IAN_SESSION_UMASK = 9, /* f64[64,64] */
  IAN_SESSION_LOCAL = 10 /* int32 flags */
};
/* One field of an opened session -> out (host or device): tests, saving a picture (NPE.py has no counterpart: its state is
   host globals).  Leaves the resident activations alone. */
int ian_session_read(ian_handle* h, int32_t id, int32_t what, void* out, void* stream);
/* ---- full-resolution edit sessions: photos of S x S pixels, S = 64 * scale, edited through the 64x64 model ----
   What NPE.paint shows, from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR) with ERROR = to_tanh(GIM) - to_tanh(RECON), is the
   photo plus the smooth field MASK*(DELTA - ERROR).  A full-resolution pool keeps the photo at its own size (SRC u8[3,S,S]) and that
   field (FIELD f32[3,64,64], FIELD_KIND) per session, and renders windows of SRC + 127.5 * bilinear(FIELD) on the device: the
   unedited part of the photo stays pixel-exact.  FIELD always describes what the last call on the session displayed:
     open / Reset / commit: zeros, kind 0;  set_latent(as_sample = 1): x, kind 1;
     a paint event or set_latent(as_sample = 0) on a photo-mode session: float32(MASK * (float64(DELTA) - float64(ERROR))), kind 0;
     the same on a sample-mode session, and every lighten event (mode 0): x, kind 1 (what these display is the plain sample).
   The arithmetic, operation by operation, is npe_ops.hires_downsample / edit_field / hires_axis_taps / hires_render (numpy); the
   device matches them bit for bit.  Without the reservation below nothing of this exists and no other call changes. */

/* scale 1..16 allocates SRC / FIELD / FIELD_KIND for every session of the pool (0 frees them).  Needs ian_sessions_reserve first
   (-6 otherwise).  Synchronises the device.  Changing the scale drops every session's source (its 64x64 state stays);
   ian_sessions_reserve(capacity) afterwards resizes the three arrays too, keeping the rows that remain.  An allocation failure
   (-2) leaves the old pool intact.  3 * S * S + 49 156 bytes per session: 4096 sessions at scale 16 are 12 GB. */
int ian_sessions_reserve_hires(ian_handle* h, int32_t scale);

/* photos u8[n,3,S,S], host or device (4-byte aligned).  SRC := photos; GIM := the exact integer box mean of SRC over scale x scale
   blocks, (sum + scale*scale/2) / (scale*scale), computed on the device; then exactly ian_session_open(photos = GIM), in the same
   submission.  shown u8[n,3,64,64] or NULL receives IM (= GIM).  A plain ian_session_open with 64x64 photos on a session of such
   a pool clears its source; ian_session_open(source = 1) (commit) on a session with a source first sets SRC := the whole rendered
   picture, then updates the 64x64 state as always (GIM := IM): SRC's box mean and GIM then differ by rounding. */
int ian_session_open_hires(ian_handle* h, int32_t n, const int32_t* ids, const uint8_t* photos, uint8_t* shown, void* stream);

typedef struct ian_session_view {
  int32_t session; /* id in the pool */
  int32_t x, y;    /* top-left corner of the window in the S x S picture */
} ian_session_view;

/* Window (x, y, vw, vh) of each view's session at full resolution -> out u8[n,3,vh,vw] (host or device, 4-byte aligned):
     v = bilinear sample of FIELD at half-pixel centres, edges clamped, float32, every operation rounded on its own
     kind 0: out = uint8(clip(rint(float32(SRC) + 127.5f * v), 0, 255));   kind 1: out = uint8(clip(rint(127.5f * (v + 1.0f)), 0, 255))
   (rint rounds ties to even; a zero field returns the source bytes).  x and vw must be multiples of 4 (every lane stores 4 aligned
   bytes), vw >= 4, vh >= 1, the window inside S x S.  Like ian_session_read it touches neither the decoder's activations nor the
   residency of ian_session_brush.  The same session may appear several times, as tiles of one picture.
   -6: no full-resolution reservation.  -7, naming the item, before anything is enqueued: n outside 1..256, an id outside the
   pool, a session not opened or without a source, a window outside the picture, x or vw not a multiple of 4. */
int ian_session_render(ian_handle* h, int32_t n, const ian_session_view* views, int32_t vw, int32_t vh, uint8_t* out, void* stream);

/* ian_session_brush followed by ian_session_render of the same sessions, in ONE submission with one synchronisation: the event's
   64x64 canvas (shown, or NULL) and its full-resolution window (out) come back together.  views[i].session must equal
   events[i].session (-7). */
int ian_session_brush_view(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, const ian_session_view* views,
                           int32_t vw, int32_t vh, uint8_t* out, void* stream);

/* ---- edge-aware render: the edit field guided by the photo (joint bilateral upsampling) ----
   The plain bilinear tap above lets an edit bleed over every edge of the photo by up to `scale` pixels.  With a guide reserved, each
   of the four taps is also weighted by how close the photo's pixel is to the tap's pixel of GIM (the photo's own 64x64 box mean),
   through a table of 766 range weights indexed by the summed absolute byte difference of the three channels.  The table is made
   on the host (npe_ops.guide_table(sigma): max(float32(exp(-d*d / (2 * (3*sigma)^2))), 2^-24), exponent in float64, sigma in levels
   per channel); no exp runs on the device.  Kind 1 (FIELD is a sample, there is no photo to guide by) renders as without a guide.
   Kind 0, per output pixel (Y, X), float32, every operation rounded on its own:
     (r0, r1, ty), (c0, c1, tx) = the taps of ian_session_render;  tap k = 0..3 is (r0,c0), (r0,c1), (r1,c0), (r1,c1);
     s_k = wy * wx, wy in {1.0f - ty, ty}, wx in {1.0f - tx, tx};
     d_k = sum over c of |int(SRC[c,Y,X]) - int(GIM[c,r_k,c_k])|;   w_k = s_k * table[d_k]   (the same four weights for all channels);
     den = ((w0 + w1) + w2) + w3;   num_c = ((w0*f0 + w1*f1) + w2*f2) + w3*f3, f_k = FIELD[c,r_k,c_k];   v = num_c / den (one division);
     out = uint8(clip(rint(float32(SRC[c,Y,X]) + 127.5f * v), 0, 255)).
   A zero field gives num = 0: the source bytes.  The arithmetic is npe_ops.hires_render_guided; the device matches it bit for bit.

   count == 766: table (host, f32[766], every entry finite and > 0) goes to a device buffer the pool owns and the guide is on; again:
   the table is replaced.  count == 0 (table ignored): the buffer is freed and the guide is off.  While it is on, ian_session_render,
   ian_session_brush_view and the whole-picture render of ian_session_open(source = 1) launch the guided kernel in place of the
   bilinear one, with the same checks, copies and synchronisation; without it every call enqueues what it always did.  The table is a
   setting of the pool, not session state: ian_session_save / _load, records and history do not know it.  Synchronises the device.
   ian_sessions_reserve_hires(0) frees the guide with its group; a new scale keeps it.
   -6: no full-resolution reservation, or canvases are reserved (ian_canvas_compose shares the bilinear tap and promises
   ian_session_render's bytes; ian_sessions_reserve_canvas returns -6 while a guide is reserved).  -7: any other count, a null
   table, an entry that is not finite or is <= 0. */
int ian_sessions_reserve_guide(ian_handle* h, const float* table, int32_t count);
/* 1 with a guide (its table -> table_out, host f32[766], or NULL), 0 without one; -6 without a full-resolution reservation. */
int ian_sessions_guide(ian_handle* h, float* table_out);

/* ---- local edits: the edit stays where the user painted ----
   NPE.paint's MASK comes from |DELTA| anywhere in the picture, so a stroke on the hair can change the mouth.  The reference left three
   tools for that: USER_MASK ("currently not implemented", NPE.py:58-59, :221), the brush falloff gk (NPE.py:167-175) and dampen
   (NPE.py:184-189, commented out at :227 and :298).  A pool with the reservation below keeps per session UMASK f64[64,64] (where the
   user has brushed) and LOCAL (int32 flags: bit 0 = local, bit 1 = dampen).  For an opened session with flags != 0:
     a mode-1 event of ian_session_brush / ian_session_brush_view on a photo-mode session, bit 0 set: first
       UMASK := max(UMASK, F), F[y][x] = falloff[dy] * falloff[dx] with gk's distances to the rectangle (0 inside it; an empty
       rectangle adds nothing); then the blend with MASK_L = MASK * UMASK in place of MASK:
       D = MASK_L*DELTA + (1-MASK_L)*ERROR; IM = uint8(from_tanh(to_tanh(RECON) + D)); FIELD = float32(MASK_L * (DELTA - ERROR));
     bit 1: with t = to_tanh(float32(RECON)), D := thresh - t where t + D > thresh, and FIELD = float32(D - ERROR); bit 1 alone
       uses the plain MASK and leaves UMASK untouched;
     ian_session_set_latent(as_sample = 0) on a photo-mode session: the same blend with the current UMASK, no footprint added (an
       edit on the latent canvas shows only where the user has brushed);
     lighten events, sample-mode sessions and as_sample = 1: as without the flags.
   ian_session_open (all three sources) and ian_session_open_hires clear the session's UMASK in the same submission (USER_MASK *= 0,
   NPE.py:267, :337) and keep LOCAL; a commit on a session with a full-resolution source renders first.  A session with flags 0 gives
   byte for byte the results of a pool without the reservation, and such a pool runs the kernels it always ran.  The arithmetic,
   operation by operation in float64, is npe_ops.local_falloff_table / local_footprint / umask_paint / photo_blend_local (numpy); the
   device matches them bit for bit. */

/* on = 1 allocates UMASK and LOCAL for every session of the pool, both zero; on = 0 frees them and forgets the falloff table.  Needs
   ian_sessions_reserve first (-6 otherwise).  Synchronises the device.  ian_sessions_reserve(capacity) afterwards resizes both
   arrays too, keeping the rows that remain (new rows are zero).  An allocation failure (-2) leaves the old pool intact.
   32 772 bytes per session. */
int ian_sessions_reserve_local(ian_handle* h, int32_t on);
/* The footprint's falloff and the dampen threshold for every later call: falloff64 f64[64] (host; npe_ops.local_falloff_table:
   exp(-(d*d/64.0)/(2*sigma*sigma)), sigma 0.3 in NPE.py:170), falloff64[d] at d pixels from the rectangle along one axis.  -7 for a
   table whose entry 0 is not 1.0 or that has an entry outside [0,1] or a NaN; -6 without the reservation.  NPE.py:187's threshold is
   0.75.  Events and set_latent(as_sample = 0) that name a session with flags != 0 return -6 until this was called.  Synchronises
   the device. */
int ian_sessions_set_local(ian_handle* h, const double* falloff64, double dampen_thresh);
/* LOCAL[ids[i]] := flags[i] (0..3; bit 0 local, bit 1 dampen) and UMASK[ids[i]] := 0, whichever flags are given, for n opened
   sessions in one submission.  ids and flags are host arrays.  Like ian_session_read it leaves the decoder's resident activations
   and the residency of ian_session_brush alone.  -6 without the reservation; -7, naming the item, before anything is enqueued: n
   outside 1..256, an id outside the pool, a session not opened, an id given twice, flags outside 0..3. */
int ian_session_local(ian_handle* h, int32_t n, const int32_t* ids, const int32_t* flags, void* stream);

/* ---- undo and redo: one history per session, on the device ----
   Every brush event overwrites the session's Z, UMASK, IM and FIELD in place.  A pool with the reservation below keeps, per session, a
   ring of saved states in device memory; the host keeps only a list length and a cursor per session.  A saved state is the session's
   Z row and, in a pool that had the local reservation when the history was reserved, its UMASK row.  IM, FIELD, FIELD_KIND and the
   canvas are not saved: they are a function of (Z, UMASK, RECON, ERROR, mode, LOCAL) and are recomputed on restore.
   Per session: entries E[0..len-1], a cursor c (0 <= c <= len; c == len: the live state is not in the list).
     mark     (ian_session_mark, "a stroke begins"): the entries after the cursor go; with `depth` entries the oldest goes; the live
              state becomes the last entry, c = len.
     undo k   1 <= k <= c: from the tip (c == len) the live state is first saved behind the list, so that redo can come back to it;
              c -= k, live := E[c].
     redo k   1 <= k <= len - 1 - c: c += k, live := E[c].
     edited   any other call that writes Z without clearing (ian_session_brush, _brush_view, ian_session_set_latent with as_sample = 0)
              with c < len: the entries after E[c] go and c = len; the state the user came back to stays an undo target (the oldest
              entry goes when that makes depth + 1 of them).
     clear    len = c = 0: every call that rewrites RECON / ERROR / GIM or zeroes UMASK (ian_session_open with all three sources,
              ian_session_open_hires, ian_session_set_latent with as_sample = 1, ian_session_local, ian_session_fit), and a change of the depth.
   So `depth` is the largest number of steps that can be undone.  Restoring a state means, in one submission: UMASK and Z := the saved
   rows; x = the decoder at Z at batch n exactly as ian_session_set_latent runs it; on a photo-mode session the blend of
   ian_session_set_latent(as_sample = 0) -- the session's LOCAL flags, the restored UMASK, no footprint -- but stored:
   IM := shown := blend, FIELD := the edit field, kind 0; on a sample-mode session shown = uint8(from_tanh(x)), IM untouched,
   FIELD := x, kind 1.  After an undo IM is therefore the blend at the restored latent, even if the last thing displayed in that
   state was a lighten event's plain sample.  Without the reservation no call launches, moves or computes anything it did not before. */

/* depth 1..64 allocates the rings for every session of the pool (0 frees them); every history starts empty.  Needs
   ian_sessions_reserve first (-6 otherwise).  Synchronises the device.  The same depth again changes nothing; another depth builds new
   rings and clears every history.  ian_sessions_reserve(capacity) afterwards resizes the rings with the rest: the sessions whose ids
   remain keep their histories.  An allocation failure (-2) leaves the old pool intact.  While a history is reserved,
   ian_sessions_reserve_local with another `on` than the pool has returns -6: free the history first.
   (depth + 1) * (4 * num_latents + 32 768) bytes per session with the local reservation, (depth + 1) * 4 * num_latents without: depth
   16 and 100 latents are 563 856 or 6 800 bytes. */
int ian_sessions_reserve_history(ian_handle* h, int32_t depth);
/* Saves the live state of n opened sessions as a new last entry ("mark" above): one launch.  ids is a host array.  Like
   ian_session_read it leaves the decoder's resident activations and the residency of ian_session_brush alone.  -6 without the
   reservation; -7, naming the item, before anything is enqueued: n outside 1..256, an id outside the pool, a session not opened, an
   id given twice. */
int ian_session_mark(ian_handle* h, int32_t n, const int32_t* ids, void* stream);
/* steps[i] > 0 undoes that many marks on session ids[i], < 0 redoes as many (steps NULL: one undo each); one submission on the
   caller's stream.  shown u8[n,3,64,64] (host or device) or NULL receives what the canvases show.  ids and steps are host arrays.
   -6: no history reservation, ian_sessions_set_blend not called, a session with LOCAL flags but no falloff table.  -7, naming the item,
   before anything is enqueued or any counter moves: n outside 1..256, an id outside the pool, a session not opened, an id given
   twice, steps[i] == 0, more undo or redo steps than the session has (the message gives the count it has). */
int ian_session_undo(ian_handle* h, int32_t n, const int32_t* ids, const int32_t* steps, uint8_t* shown, void* stream);
/* out[0] = the pool's depth, out[1] = how many steps ian_session_undo can undo on this opened session now, out[2] = how many it can
   redo.  Host only: no device state is touched.  -6 without the reservation, -7 for an id outside the pool or not opened. */
int ian_session_history(ian_handle* h, int32_t id, int32_t out[3]);

/* ---- fitting the latent to the photo: Adam steps on the reconstruction loss, on the device ----
   An open keeps the encoder's latent, so RECON is as far from the photo as the encoder leaves it and ERROR carries the rest.  This
   call refines the latent of n opened sessions by gradient descent on the API.py:64 loss against each session's own photo, `steps`
   Adam steps in ONE submission on the caller's stream, and then ends like Reset at the fitted latent.  Per item:
     T    = tanh_table[GIM byte]: np.asarray([to_tanh(GIM)], dtype=np.float32), the floats an open feeds the encoder; nothing is uploaded.
     Z_0  = the session's current Z (after an open the encoder's latent, after edits the edited one).
     g    = imgradRGB(c1, r1, c2, r2, T, Z_{t-1}) for t = 1..steps: bit for bit what ian_grad_batch returns for that rectangle, that
            target image and that latent at the same batch size; an empty rectangle gives g = 0.
     Adam step t in float32, every operation rounded on its own, no contraction, in exactly this order (csrc/ian_fit_step.h,
     npe_ops.fit_adam_step):
            m  = (0.9f * m) + (0.1f * g);   v = (0.999f * v) + ((0.001f * g) * g);   mh = m * c1[t];   vh = v * c2[t]
            Z_t = Z_{t-1} - ((lr * mh) / (sqrtf(vh) + 1e-8f))
            c1[t] = float32(1.0 / (1.0 - 0.9**t)), c2[t] = float32(1.0 / (1.0 - 0.999**t)), computed in double on the host
            (npe_ops.fit_adam_consts).  m and v start at zero on every call: they live in a per-handle workspace, not in the pool, so
            a second call starts a fresh optimiser.  g = 0 leaves Z unchanged (0 / 1e-8f = 0).
     Then IM := GIM, Z := Z_steps, RECON := uint8(from_tanh(sample_at(Z_steps))) exactly as ian_decode_u8 computes it at that batch,
     ERROR := to_tanh(float32(GIM)) - to_tanh(float32(RECON)), mode := photo, UMASK := 0 (LOCAL kept), FIELD := 0 at kind 0 (the "SRC
     holds a photo" flag kept), the history cleared, a new latent version.  The residency of ian_session_brush ends and is not
     re-armed.  A placement on a canvas stays: GIM does not change.  Any opened session may be fitted, a sample-mode one included
     (its GIM is still there); it ends in photo mode.
   shown u8[n,3,64,64] (host or device, or NULL) receives RECON, the one picture the caller does not already have.
   loss f64[n, steps+1] (host or device, or NULL) receives loss[i][t], t = 0..steps: the API.py:64 loss at Z_t, the float64 mean of
   (float64(x) - float64(T))**2 over the rectangle, summed in a fixed order (deterministic), 0 for an empty rectangle; with NULL the
   loss kernel is not launched.  One synchronisation at the end, and only when loss or shown is host memory.
   steps is 1..512, lr finite and > 0, n 1..256; more than `brush_pass` items (ian_set_option) run as passes, each pass through all
   its steps before the next starts.  A pool that never calls this launches, moves and computes nothing it did not before.
   -6: no pool.  -7, naming the item, before anything is enqueued or any host state moves: n outside 1..256, an id outside the pool,
   a session not opened, an id given twice, a rectangle outside the image, steps outside 1..512, lr not finite or not positive. */
typedef struct ian_session_fit_item {
  int32_t session;          /* id in the pool */
  int32_t c1, r1, c2, r2;   /* API.py:72-76 rectangle the loss is taken over, columns first; (0,0,64,64) = the whole picture */
} ian_session_fit_item;
int ian_session_fit(ian_handle* h, int32_t n, const ian_session_fit_item* items, int32_t steps, float lr, double* loss, uint8_t* shown,
                    void* stream);

/* ---- strokes: a session's whole brush path in ONE submission ----
   ian_session_brush takes one event per session per call, as NPE.paint takes one <B1-Motion>.  An editor behind a server receives the
   path of a drag -- K rectangles along the mouse track -- and wants the picture at its end.  A stroke is that path: per session
   `count` rectangles boxes[first .. first + count), applied in that order, with one mode, coef and colour for all of them.
   Meaning: let Kmax = strokes[0].count.  For k = 0 .. Kmax-1 take the strokes with count > k, in the order given, and call
   ian_session_brush on them with the events
       rectangle = boxes[first + k], gscale = boxes[first + k].gscale, mode / coef / rgb = the stroke's.
   The result is what that sequence of calls gives: afterwards every session equals the session after it, byte for byte -- Z, IM, RECON,
   ERROR, GIM, the mode and, where the pool has them, FIELD, FIELD_KIND, UMASK and LOCAL -- and shown[i] (u8[n,3,64,64], host or device,
   or NULL) is what session i's last event displayed.  What is saved is everything between the steps that nobody looks at: one table
   upload instead of Kmax, no blend, no copy of shown and no synchronisation before the last point of a stroke, and no decoder forward
   at the start of a step whose sessions are those of the step before (brush_step's forward at z_new is the next step's forward at Z).
   In a pool with the local reservation the footprints of ALL of a stroke's rectangles go into UMASK before its first step (max is
   exact, so the order does not matter); the blend of the last point then sees the UMASK the K calls would have built.
   Order: the strokes must come with non-increasing count, so that the strokes of every step are a prefix of the array and the ones
   that end at a step the tail of that prefix.
   flags: bit 0 = mark first: what ian_session_mark does on the n sessions, in the same submission, so that one stroke is one undo step
   (-6 without the history reservation).  ian_session_history afterwards reports what the separate calls would.
   More than `brush_pass` strokes (ian_set_option) run as passes, each pass through all its steps before the next starts.  The
   residency of ian_session_brush is used at the start (same ids, same order, same latent versions) and re-armed at the end when the
   call was one pass and every stroke was active at the last step.  One synchronisation at the end, and only when shown is host memory.
   -6: no pool, ian_sessions_set_blend not called, a session with LOCAL flags but no falloff table, bit 0 without a history.  -7, naming
   the item (and the point, where one is concerned), before anything is enqueued or any host state moves: everything ian_session_brush
   refuses, count outside 1..IAN_STROKE_MAX_POINTS, first < 0 or first + count > nboxes, a rectangle outside the image (an empty one is
   allowed and gives a zero gradient), counts that increase, a flag bit other than bit 0, strokes or boxes in device memory. */
#define IAN_STROKE_MAX_POINTS 64
typedef struct ian_stroke_box {
  int32_t c1, r1, c2, r2;   /* API.py:66-76 rectangle, columns first */
  float gscale;             /* as ian_session_event.gscale: NPE.py:206 has 1 + (c2 - c1) */
} ian_stroke_box;
typedef struct ian_session_stroke_item {
  int32_t session;          /* id in the pool */
  int32_t first, count;     /* its rectangles: boxes[first .. first + count), applied in that order */
  int32_t mode;             /* as ian_session_event.mode, for every point of the stroke */
  float coef;               /* as ian_session_event.coef, for every point */
  float rgb[3];             /* as ian_session_event.rgb */
} ian_session_stroke_item;
int ian_session_stroke(ian_handle* h, int32_t n, const ian_session_stroke_item* strokes, int32_t nboxes, const ian_stroke_box* boxes,
                       int32_t flags, uint8_t* shown, void* stream);

/* ---- the clone brush: paint from another picture of the pool ----
   ian_session_brush pulls a rectangle towards one flat colour.  A photo editor's second brush pulls it towards a picture: "give A the
   mouth of B" (another session as the source), the clone stamp (the session itself, at an offset), the restore brush (the session's own
   GIM at offset 0).  Every byte of such a target already lies in the pool, so nothing but the event table is uploaded.
   Meaning, steps == 1: item i is a mode-1 event of ian_session_brush on events[i].session whose target image T_i replaces the constant
   colour,
       T_i[co, r, c] = tanh_table[F[source][co, r + dr, c + dc]]   for (r, c) inside the rectangle,
   F the source's GIM, IM or RECON row and tanh_table the table of ian_session_open / ian_session_fit
   (np.asarray([to_tanh(level)], dtype=np.float32), ian_session_tanh_table); elements outside the rectangle are not read.  Z, IM (photo-mode
   destination: the NPE.py:218-231 blend), shown and, where the pool has them, FIELD / FIELD_KIND and UMASK (the rectangle's footprint
   under LOCAL bit 0, exactly as a paint event) are bit for bit what ian_brush_step_batch gives for the same latents, rectangles, coef,
   gscale and rgb = T at the same batch size with photo = (RECON, ERROR) of the destinations.  A sample-mode destination shows
   np.uint8(from_tanh(x)) and keeps its IM, as in ian_session_brush.
   steps == K (1..IAN_CLONE_MAX_STEPS; a target picture needs several gradient steps where a flat colour gets them from the drag): every
   session ends byte for byte where K calls with steps == 1 and the same events leave it, and shown is what the last of them displays.
   Only the last step blends: IM and FIELD are rewritten from RECON by every event and the UMASK footprint of a repeated rectangle is
   idempotent; the forward at z_new of step k is the forward at Z of step k + 1.  The sources do not change during the call: GIM and
   RECON are not written by a brush, and an IM source that is also a destination is refused.  The same source may serve several items.
   Residency, latent versions and the history behave as in ian_session_brush: a hit on the same ids, order and versions skips the
   gather and the forward, the residency is re-armed at the end when the call was one pass, every destination gets one new latent version
   and one `edited` note.  For one undo step per call, call ian_session_mark first.  More than `brush_pass` items (ian_set_option) run
   as passes, each pass through all its steps before the next starts.  Host -> device: the event table (11 words per event); device ->
   host: shown (u8[n,3,64,64], host or device, or NULL).  One synchronisation at the end, and only when shown is host memory.  A pool
   that never calls this launches, moves and computes nothing it did not before.
   -6 where ian_session_brush returns it.  -7, naming the item, before anything is enqueued or any host state moves: everything
   ian_session_brush refuses for the destination, a source outside the pool or not opened, a field other than the three, a non-empty
   rectangle whose shifted copy leaves the image (c1 + dc < 0, c2 + dc > 64, likewise rows), a source with field == IAN_SESSION_IM that
   is also a destination of this call, steps outside 1..IAN_CLONE_MAX_STEPS, events in device memory. */
#define IAN_CLONE_MAX_STEPS 64
typedef struct ian_session_clone_event {
  int32_t session;          /* destination: id in the pool */
  int32_t c1, r1, c2, r2;   /* rectangle on the destination, columns first; an empty one gives a zero gradient */
  int32_t source;           /* id of the session the target is read from; may equal `session` */
  int32_t field;            /* IAN_SESSION_GIM, IAN_SESSION_IM or IAN_SESSION_RECON of the source */
  int32_t dc, dr;           /* the target of destination pixel (r, c) is source pixel (r + dr, c + dc) */
  float coef, gscale;       /* Z := Z + coef * (dZ * gscale), as ian_session_event */
} ian_session_clone_event;
int ian_session_clone(ian_handle* h, int32_t n, const ian_session_clone_event* events, int32_t steps, uint8_t* shown, void* stream);

/* ---- brush tips: a weighted brush loss, for round brushes with a soft edge ----
   Every brush above weights the pixels of its rectangle alike (1/N).  A tip is a small weight image wn, f32[th][tw] with
   1 <= tw, th <= 64, and a paint or light event that names a tip takes the tip's weights in the place of the flat 1/N:
       mode 1:  loss = sum_{co,r,c} wn[r - r1][c - c1] * (x_hat[co,r,c] - rgb[co])^2      seed g = 2.f * (x_hat - rgb[co]) * wn[r - r1][c - c1]
       mode 0:  loss = sum wn * x_hat                                                       seed g = wn[r - r1][c - c1]
   and zero outside the rectangle; the three channels share the one weight.  The library takes wn as given (a general weighted loss);
   how a brush shape becomes weights is the host's policy: npe_ops.tip_weights(w) = float32(w) * (float32(1) / float32(3 * sum w)), for
   which an all-ones tip IS the rectangle brush, bit for bit, in both modes (wn == 1.f / (float)(3 * th * tw), the rectangle's own 1/N).
   The event's rectangle lies inside the image as always, and its size is exactly the tip's: c2 - c1 == tw and r2 - r1 == th.
   Tips belong to the handle, not to a session: they are no part of a saved session, of the undo history, of the guide or of a canvas.
   Tips weight every call that paints on a session: the colour brushes (ian_session_brush_tip, ian_session_path_tip, and on a whole
   photo ian_compose_brush_soft) and the clone and restore brushes (ian_session_stamp_soft).  ian_session_fit and the stateless
   ian_grad_batch / ian_brush_step_batch keep the unweighted loss.  Under the local reservation the footprint that goes into UMASK is
   that of the rectangle unless ian_sessions_set_soft_mask switched on the footprint shaped by the tip (below).  A pool that
   never reserves tips launches, moves and computes nothing it did not before. */

/* Room for `count` tips (0..64; 0 frees them; another count frees them and every tip starts unset; the same count changes nothing).
   Needs the pool (-6 otherwise), synchronises the device.  ian_sessions_reserve(0) and ian_destroy free the tips too. */
int ian_sessions_reserve_tips(ian_handle* h, int32_t count);
/* Tip `tip` := wn, host f32[th][tw].  Synchronises the device first, so that no event in flight sees the tip change.  -6 without the
   tip reservation.  -7, with nothing changed: tip outside the reservation, tw or th outside 1..64, a weight that is negative,
   infinite or NaN (all zero is allowed and gives a zero gradient), wn in device memory. */
int ian_sessions_set_tip(ian_handle* h, int32_t tip, int32_t tw, int32_t th, const float* wn);
/* wh := (tw, th) of tip `tip` and, where wn_out (host f32[th][tw]) is given, its weights.  -7 for a tip never set. */
int ian_sessions_tip(ian_handle* h, int32_t tip, int32_t wh[2], float* wn_out);
/* ian_session_brush (views == NULL; vw, vh, out unused) or ian_session_brush_view (views given) with one tip index per event: tips
   int32[n], host; -1 = no tip, and such an item is today's rectangle event, byte for byte.  Everything else is the plain call's:
   residency, latent versions, history notes, passes of brush_pass, the blend, shown and the windows.  Host -> device: the event table,
   12 words per event.  -6 where the plain call returns it, and without the tip reservation.  -7, naming the item, before anything
   is enqueued: everything the plain call refuses, a tip outside -1..count-1, a tip never set, a rectangle whose size is not the
   tip's, tips NULL or in device memory. */
int ian_session_brush_tip(ian_handle* h, int32_t n, const ian_session_event* events, const int32_t* tips, uint8_t* shown,
                          const ian_session_view* views, int32_t vw, int32_t vh, uint8_t* out, void* stream);
/* ian_session_stroke with one tip per stroke (tips int32[n], host; -1 = none): every rectangle of stroke i must have the size of tip
   tips[i].  Its meaning is the loop given for ian_session_stroke with ian_session_brush_tip in the place of ian_session_brush, byte
   for byte.  Refusals: those of ian_session_stroke and of ian_session_brush_tip, naming the item and the point. */
int ian_session_path_tip(ian_handle* h, int32_t n, const ian_session_stroke_item* strokes, const int32_t* tips, int32_t nboxes,
                         const ian_stroke_box* boxes, int32_t flags, uint8_t* shown, void* stream);

/* ian_session_clone with one tip index per event (tips int32[n], host; -1 = no tip, and such an item is today's clone event, byte
   for byte).  Item i with tip t >= 0 is a clone event whose seed, inside the rectangle, is
       g = 2.f * (x_hat[co,r,c] - tanh_table[F[source][co, r + dr, c + dc]]) * wn_t[r - r1][c - c1]
   (float32, in that order) and zero outside: the clone's target with the tip's weight in the place of 1/N.  Everything else is
   ian_session_clone's: steps 1..IAN_CLONE_MAX_STEPS of which only the last blends, residency, latent versions, history notes, passes
   of brush_pass, the refusals.  Host -> device: the event table, 12 words per event.  -6 also without the tip reservation; -7, naming
   the item, before anything is enqueued: what ian_session_brush_tip refuses about tips. */
int ian_session_stamp_soft(ian_handle* h, int32_t n, const ian_session_clone_event* events, const int32_t* tips, int32_t steps,
                          uint8_t* shown, void* stream);
/* A user mask shaped by the tip.  on = 1: an item that names a tip >= 0, is a paint event (mode 1, or a clone), targets a session in
   photo mode with LOCAL bit 0 set, in a pool with the local reservation -- exactly where the rectangle's footprint goes into UMASK
   -- max-es the footprint of its tip into UMASK in the place of the rectangle's, every point of a stroke included:
       s[qy,qx] = (double)wn[qy][qx] / (double)max wn          (all zero for an all-zero tip)
       R[qy,x]  = max_qx s[qy,qx] * falloff[|x - (c1 + qx)|]
       F[y,x]   = max_qy falloff[|y - (r1 + qy)|] * R[qy,x]    UMASK := max(UMASK, F)        (npe_ops.tip_footprint)
   in float64, one product each; for an all-ones tip that is the rectangle's footprint bit for bit.  Items with tip -1, light events,
   sample-mode sessions and sessions with bit 0 clear behave as ever.  on = 0 (the default): every call is byte for byte what it is
   without this setting.  A setting of the handle like the pixel format: not a LOCAL flag, no part of a saved session (the UMASK it
   leaves is).  Needs the tip reservation (-6 otherwise), synchronises the device; ian_sessions_reserve_tips with another count and
   ian_sessions_reserve(0) clear it; without the local reservation it is kept and changes nothing.  -7 for on outside 0..1. */
int ian_sessions_set_soft_mask(ian_handle* h, int32_t on);
int ian_sessions_soft_mask(ian_handle* h, int32_t* on);

/* ---- saving and loading whole sessions: the editor state as bytes that can leave the pool ----
   Everything a session is -- the 64x64 state, the full-resolution source and edit field, the user mask and flags, the ring of undo
   states with its cursor -- lives in one handle's pool.  A record is that state as plain bytes: keep a project beyond the process,
   move an editor to another handle or GPU, park an idle editor and give its id to someone else.  One session is one meta block (64
   bytes, host data) and one body:
     body = every array of the pool, in the order GIM IM RECON ERROR Z MODE | SRC FIELD FIELD_KIND | UMASK LOCAL | the ring's Z rows,
            the ring's UMASK rows -- the groups the pool has reserved -- each padded with zeros to a multiple of 16 bytes.
   Records are canonical: two saves of the same logical state give the same bytes, and no byte of a record comes from memory the
   session never wrote.  Entry k of the history goes to slot k of the record whatever its place in the ring; slots >= hist_len are
   zero; SRC of a session without a source is zero.  A load puts entry k into ring slot k, leaves the slots >= hist_len and the SRC
   row of a record without a source unwritten, and restarts the ring at slot 0.
   A record belongs to the pool layout it was saved from (num_latents, scale, local, depth): a load into any other layout is
   refused, never converted.  It is only meaningful with the weights it was edited under; the record carries no fingerprint of them,
   so keeping the two together is the caller's business. */
#define IAN_SESSION_RECORD_MAGIC 0x534e4149u /* "IANS" */
#define IAN_SESSION_RECORD_FORMAT 1
#define IAN_SESSION_RECORD_MAX_COLUMNS 13
typedef struct ian_session_meta {
  uint32_t magic;           /* IAN_SESSION_RECORD_MAGIC */
  int32_t format;           /* IAN_SESSION_RECORD_FORMAT */
  int32_t num_latents;      /* the layout of the pool the record came from: the model's latent size, */
  int32_t scale;            /*   the full-resolution scale (0: no such reservation), */
  int32_t local;            /*   1 with the local reservation, */
  int32_t depth;            /*   the history's depth (0: none) */
  int32_t has_source;       /* what the library keeps per session on the host: 1 when SRC holds a photo, */
  int32_t local_flags;      /*   the LOCAL flags 0..3, */
  int32_t hist_len;         /*   the history's entries and cursor (0 <= hist_cur <= hist_len; see ian_session_undo) */
  int32_t hist_cur;
  int64_t body_bytes;       /* bytes of one body in this layout: a multiple of 16 */
  int32_t reserved[4];      /* zero */
} ian_session_meta;

/* The record layout of this handle's pool.  layout (or NULL) receives magic, format, the four layout fields and body_bytes, the
   per-session fields zero; offsets (or NULL; room for IAN_SESSION_RECORD_MAX_COLUMNS) the byte offset in the body of every array the
   pool has, in the order above; ncols (or NULL) how many those are.  Host only: no device state is touched.  -6 without a pool. */
int ian_session_record_info(ian_handle* h, ian_session_meta* layout, int64_t* offsets, int32_t* ncols);
/* n opened sessions -> n records in one submission: meta is a host array of n entries, body n * body_bytes bytes, host or device,
   16-byte aligned.  One upload (4 words per session), one gather kernel straight into a device body; a host body goes through a
   staging buffer of at most `session_stage_bytes` (ian_set_option; default 64 MiB, never less than one record), as many
   gather-then-copy passes in stream order as that takes, and one synchronisation.  Like ian_session_read it leaves the decoder's
   resident activations and the residency of ian_session_brush alone, and it changes no session.
   -6: no pool.  -7, naming the item, before anything is enqueued: n outside 1..256, an id outside the pool, a session not opened, an
   id given twice, ids or meta not host arrays, body not 16-byte aligned. */
int ian_session_save(ian_handle* h, int32_t n, const int32_t* ids, ian_session_meta* meta, void* body, void* stream);
/* n records -> sessions ids[0..n-1] of this pool, opened or not, in one submission (one upload, one scatter kernel; a host body in
   copy-then-scatter passes as above).  Afterwards each target is opened, holds the record's state -- source bit, LOCAL flags, history
   entries and cursor included -- and counts as a new latent version, so that a forward left resident for its old latent is not
   reused.  No other session and none of the decoder's activations are touched; nothing is displayed: read IM or redisplay.
   -6: no pool.  -7, naming the item and the field, before anything is enqueued or any host state moves: the cases of
   ian_session_save (the targets need not be opened); a bad magic or format; num_latents, scale, local, depth or body_bytes other
   than this pool's (the message gives both values); local_flags outside 0..3, or not 0 in a layout without the local reservation;
   has_source outside 0..1, or 1 at scale 0; a cursor outside 0 <= hist_cur <= hist_len, hist_len > depth with hist_cur == hist_len,
   hist_len > depth + 1 otherwise, any entry at depth 0; a reserved word that is not zero. */
int ian_session_load(ian_handle* h, int32_t n, const int32_t* ids, const ian_session_meta* meta, const void* body, void* stream);

/* ---- canvases: sessions placed on whole photos, and the composed result ----
   A full-resolution session is a square of 64 * scale pixels and the pool has one scale.  A real photo is some W x H; the face the
   model can edit is a square somewhere inside it, and a group photo has several.  With the reservation below photos of any size
   (canvases) live in device memory, sessions are placed on a canvas as squares -- each with its own integer scale, at any pixel
   offset -- and one kernel composes windows of the whole photo from the canvas and every placed session's edit field (FIELD /
   FIELD_KIND of the full-resolution reservation), feathered towards each square's edge.  Per output pixel and channel, float32,
   every operation rounded on its own:
     acc = float32(canvas byte); then for every placement whose square covers the pixel, in ascending session id:
       v = the bilinear sample of its FIELD at the pixel's place in the square, exactly as ian_session_render samples it;
       w = ry * rx, each r = min(1.0f, float32(2d + 1) / float32(2 * feather * scale)) with d the distance to the nearer edge of
           the square along that axis (feather 0: w = 1.0f);
       kind 0: acc = acc + (127.5f * v) * w;   kind 1: t = 127.5f * (v + 1.0f); acc = t where w == 1.0f, else acc + (t - acc) * w;
     out = uint8(clip(rint(acc), 0, 255)), ties to even.
   Zero fields return the canvas bytes, no byte outside every square changes, and in the core of a lone placement (w == 1) the
   result is byte for byte what ian_session_render gives for the crop.  The arithmetic is npe_ops.canvas_crop_mean / canvas_ramp /
   canvas_compose (numpy); the device matches them bit for bit.  Without the reservation nothing of this exists and no other call
   launches, moves or computes anything it did not before.  A placement is not part of a saved session (ian_session_save). */
typedef struct ian_canvas_placement {
  int32_t session; /* id in the pool */
  int32_t canvas;  /* id of the canvas, 0..count-1 */
  int32_t x, y;    /* top-left corner of the square on the canvas, any alignment */
  int32_t scale;   /* 1..16: the square is 64 * scale pixels a side */
} ian_canvas_placement;
typedef struct ian_canvas_window {
  int32_t canvas; /* id of the canvas */
  int32_t x, y;   /* top-left corner of the window on the canvas */
} ian_canvas_window;
#define IAN_CANVAS_MAX_PLACED 8

/* count 1..64 canvases of up to max_w x max_h pixels (64..8192 each, max_w a multiple of 4): `count` arrays u8[3,max_h,max_w] and
   a device table of IAN_CANVAS_MAX_PLACED placements per canvas; feather 0..16 is the width of every square's feathered rim in
   field pixels.  count 0 frees the arrays and every placement.  Needs ian_sessions_reserve and ian_sessions_reserve_hires at any
   scale first (-6 otherwise): a placement uses FIELD and FIELD_KIND, SRC is not touched.  Synchronises the device.  A second
   reservation starts from nothing: no canvas holds a picture, no session is placed.  An allocation failure (-2) leaves the old
   state intact.  While canvases are reserved ian_sessions_reserve_hires(0) returns -6 (the only new refusal of an existing call);
   ian_sessions_reserve(capacity) drops the placements of the ids that leave the pool, ian_sessions_reserve(0) frees the canvases
   with everything else. */
int ian_sessions_reserve_canvas(ian_handle* h, int32_t count, int32_t max_w, int32_t max_h, int32_t feather);
/* The picture of one canvas: pixels u8[3,hgt,w], host or device; 64 <= w <= max_w, w a multiple of 4, 64 <= hgt <= max_h.  A strided
   copy into the canvas's array.  Every placement on that canvas is dropped; the sessions keep their 64x64 state. */
int ian_canvas_put(ian_handle* h, int32_t canvas, int32_t w, int32_t hgt, const uint8_t* pixels, void* stream);
/* Per item: GIM := the exact integer box mean of the canvas's square (x, y) + 64 * scale over scale x scale blocks, computed on the
   device straight from the canvas; then exactly ian_session_open(photos = GIM) in the same submission (the UMASK clear, the history
   clear and a zero FIELD at kind 0 included); the session is placed at (canvas, x, y, scale).  A session already placed moves.
   shown u8[n,3,64,64] (host or device) or NULL receives IM.  The session counts as opened without a full-resolution source.
   -6: no canvas reservation.  -7, naming the item, before anything is enqueued: n outside 1..256, an id or a canvas outside its
   range, a canvas never put, a square outside the canvas, scale outside 1..16, an id given twice, a ninth session on one canvas. */
int ian_canvas_place(ian_handle* h, int32_t n, const ian_canvas_placement* items, uint8_t* shown, void* stream);
/* Window (x, y, vw, vh) of each named canvas -> out u8[n,3,vh,vw] (host or device, 4-byte aligned), composed as above over that
   canvas's placements.  x and vw must be multiples of 4, vw >= 4, vh >= 1, the window inside the canvas's w x hgt.  Like
   ian_session_render it touches neither the decoder's activations nor the residency of ian_session_brush.  The same canvas may
   appear several times, as tiles.  -6: no canvas reservation.  -7, naming the item: n outside 1..256, a canvas outside its range or
   never put, a window outside the picture, x or vw not a multiple of 4. */
int ian_canvas_compose(ian_handle* h, int32_t n, const ian_canvas_window* windows, int32_t vw, int32_t vh, uint8_t* out, void* stream);
/* ian_session_brush on n events followed by ian_canvas_compose of m windows, in ONE submission with one synchronisation: what
   ian_session_brush_view is to ian_session_render.  The events' sessions need not be placed and the windows need not belong to
   them.  Every check of both calls is made before anything is enqueued. */
int ian_canvas_brush(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, int32_t m,
                     const ian_canvas_window* windows, int32_t vw, int32_t vh, uint8_t* out, void* stream);
/* ian_canvas_brush with one tip index per event (tips int32[n], host; -1 = none): a soft brush on a whole photo, ian_session_brush_tip
   whose windows are a canvas's.  Refusals: those of both; ian_sessions_set_soft_mask applies. */
int ian_compose_brush_soft(ian_handle* h, int32_t n, const ian_session_event* events, const int32_t* tips, uint8_t* shown, int32_t m,
                         const ian_canvas_window* windows, int32_t vw, int32_t vh, uint8_t* out, void* stream);
/* The canvas becomes the compose of its whole picture, in place; then every session placed on it is placed again where it is: the
   box mean of the new canvas and the open above, at batch k = the number of sessions placed there.  shown u8[k,3,64,64] (host or
   device; ascending session id) or NULL.  ian_session_open(source = 1) on a placed session returns -7 and names this call: GIM := IM
   would bake the unfeathered 64x64 blend into the session.  Reset (source = 0) works as always.  ian_session_open with photos,
   ian_session_open_hires and ian_session_load on a placed session un-place it; every other session call works on a placed
   session as on any other, and a compose reads whatever FIELD it left. */
int ian_canvas_commit(ian_handle* h, int32_t canvas, uint8_t* shown, void* stream);
/* The picture of one canvas as it is stored (the placed sessions' edits are NOT on it before a commit) -> out u8[3,hgt,w], host or
   device; wh (host, or NULL) receives w and hgt.  out NULL: only wh. */
int ian_canvas_read(ian_handle* h, int32_t canvas, uint8_t* out, int32_t wh[2], void* stream);
/* The sessions placed on one canvas, in ascending session id -> out8 (host; room for IAN_CANVAS_MAX_PLACED) and their count.  Host
   only: no device state is touched. */
int ian_canvas_placements(ian_handle* h, int32_t canvas, ian_canvas_placement* out8, int32_t* count);

/* ---- edge-aware compose: the placed sessions' edit fields guided by the canvas ----
   The compose above samples a field with the plain bilinear tap, so at scale 16 an edit bleeds over up to 16 pixels of the photo
   along every edge.  With the table below set, the sample v of every KIND 0 placement is ian_sessions_reserve_guide's: the four
   taps weighted by table[d_k], d_k the summed absolute byte difference between the canvas's pixel and the tap's pixel of the
   session's GIM (the box mean of its square), one IEEE division.  The photo's pixel is the STORED canvas byte, not the running
   acc: overlapping placements do not see each other's edits in their weights.  acc = acc + (127.5f * v) * w follows as above;
   kind 1 placements, the feather, the order of the placements and the rounding are unchanged.  In the core of a lone placement the
   result is byte for byte what ian_session_render gives for the crop under a guide with the same table.  The arithmetic is
   npe_ops.canvas_compose_guided; the device matches it bit for bit.

   count == 766: table (host, f32[766], every entry finite and > 0; npe_ops.guide_table(sigma)) goes to a device buffer that belongs
   to the canvas reservation and ian_canvas_compose, ian_canvas_brush and ian_canvas_commit launch the guided kernel in place of the
   plain one; again: the table is replaced.  count == 0 (table ignored): the buffer is freed and the compose is the plain one.
   Synchronises the device.  The table is no session state: records, the history and ian_session_read do not know it.  Any
   ian_sessions_reserve_canvas that succeeds frees it (a new reservation starts with the plain compose), as do
   ian_sessions_reserve(0) and ian_destroy.  -6: no canvas reservation.  -7: any other count, a null table, a device pointer, an
   entry that is not finite and positive (the message names it); a refused call leaves the previous table in force.  A pool that
   never calls this launches, uploads and computes exactly what it did before. */
int ian_sessions_reserve_edges(ian_handle* h, const float* table, int32_t count);
/* 1 with the edge-aware compose on (its table -> table_out, host f32[766], or NULL), 0 with the plain one; -6 without canvases. */
int ian_sessions_edges(ian_handle* h, float* table_out);

/* ---- zoomed views: a picture or a canvas at 1/zoom, produced on the device ----
   What an editor shows while the user paints is a fit-to-window view, not the photo pixel for pixel.  For zoom in 1..16, output
   pixel (Y, X) of a window whose source origin is (x, y) is the exact integer box mean of the full-resolution result,
     (sum of the zoom x zoom block of result bytes at (y + zoom*Y .., x + zoom*X ..) + zoom*zoom/2) / (zoom*zoom),
   the result bytes being exactly those ian_session_render (ian_canvas_compose) gives for the source window
   (x, y, zoom*vw, zoom*vh): rounded to uint8 per pixel first, then averaged, the rounding of ian_session_open_hires's box mean.
   The arithmetic is npe_ops.zoom_box_mean over hires_render / hires_render_guided / canvas_compose / canvas_compose_guided; no
   full-resolution result is written on the way, the device stores and sends 3*vw*vh bytes a window.  x and y of the views and
   windows stay in full-resolution pixels; vw, vh are the OUTPUT size; out u8[n,3,vh,vw], host or device, 4-byte aligned.  Only
   whole blocks count: the source window must lie inside the picture.  A reserved guide (edges table) applies as it does at 1:1.
   zoom == 1 is the plain call.  The four entries are, in this order, ian_session_render, ian_session_brush_view (tips == NULL) or
   ian_session_brush_tip with views (tips given), ian_canvas_compose and ian_canvas_brush with a zoom; everything those calls say
   about submissions, synchronisation, the decoder's activations and the residency holds.  The commit has no zoomed form.
   -6: the reservation the plain call needs is missing.  -7, naming the item, before anything is enqueued: zoom outside 1..16, the
   source window outside the picture or canvas, x or vw not a multiple of 4, vw < 4, vh < 1, and whatever the plain call refuses. */
int ian_session_zoom(ian_handle* h, int32_t n, const ian_session_view* views, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out,
                     void* stream);
int ian_session_brush_zoom(ian_handle* h, int32_t n, const ian_session_event* events, const int32_t* tips, uint8_t* shown,
                           const ian_session_view* views, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out, void* stream);
int ian_compose_zoom(ian_handle* h, int32_t n, const ian_canvas_window* windows, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out,
                     void* stream);
int ian_compose_brush_zoom(ian_handle* h, int32_t n, const ian_session_event* events, uint8_t* shown, int32_t m,
                           const ian_canvas_window* windows, int32_t vw, int32_t vh, int32_t zoom, uint8_t* out, void* stream);

/* ---- oriented placements: a session on a canvas at any size and tilt ----
   A face in a group photo is 150 or 230 pixels across and leans; ian_canvas_place only knows upright squares of 64 * scale pixels.
   An oriented placement is a similarity transform in integers: the centre (cx2, cy2) of the square in HALF pixels of the canvas
   (pixel X covers [X, X+1), its centre is 2X+1) and A = (ax, ay), the canvas displacement per field pixel along the field's x axis
   in Q16; the field's y axis is B = (-ay, ax).  L2 = ax*ax + ay*ay must lie in [2^32, 2^40]: a step of 1..16 canvas pixels, a side
   of 64..1024 at any angle.  The library derives m (the smallest of 0..4 with 2^(32+2m) >= L2) and (bx, by) = round(A * 2^36 / L2),
   field pixels per canvas pixel in Q20.
     gather   n = 2^m nearest-pixel samples per field pixel per axis: sub-sample k of 64n has U = 2k + 1 - 64n (rows: V),
              X = ((cx2 << (16+m)) + U*ax - V*ay) >> (17+m), Y = ((cy2 << (16+m)) + U*ay + V*ax) >> (17+m);
              GIM = (sum of the n*n bytes + n*n/2) / (n*n).
     compose  per pixel dx = 2X+1-cx2, dy = 2Y+1-cy2, Uq = dx*bx + dy*by (u - 32 in Q21), Vq = dy*bx - dx*by; inside the square when
              -2^26 <= Uq, Vq < 2^26; bilinear taps at a = Q + 2^26 - 2^20, i0 = a >> 21, t = (a & (2^21-1)) / 2^21, clamped to 0..63;
              the feather min(1, (min(Q + 2^26, 2^26 - Q) >> 5) / (feather << 16)) per axis; kinds, order and rounding as above.
   At angle 0 with an integer origin and an integer step both are ian_canvas_place's and ian_canvas_compose's bytes.  The arithmetic
   is npe_ops.canvas_crop_mean_oriented / canvas_compose_oriented (numpy); the device matches them bit for bit.
   A canvas holds placements of ONE form: placing the other form while any placement of the first remains returns -7 and names the
   canvas (a caller with mixed faces places the upright ones at angle 0).  Eight per canvas and every un-place rule hold unchanged:
   ian_canvas_put, ian_session_open with photos, ian_session_open_hires, ian_session_load and a smaller pool un-place an oriented
   session, ian_session_open(source = 1) on it returns -7.  ian_canvas_compose, ian_canvas_brush, ian_compose_zoom,
   ian_compose_brush_zoom and ian_canvas_commit work on such a canvas as they are, and one call may name canvases of both forms.
   The edge-aware compose is not extended: ian_place_oriented returns -6 while ian_sessions_reserve_edges holds a table, and
   ian_sessions_reserve_edges returns -6 while any oriented placement exists. */
typedef struct ian_canvas_oriented {
  int32_t session; /* id of the session, 0..capacity-1 */
  int32_t canvas;  /* id of the canvas, 0..count-1 */
  int32_t cx2, cy2; /* centre of the square on the canvas, in half pixels */
  int32_t ax, ay;  /* canvas displacement per field pixel along the field's x axis, Q16 */
} ian_canvas_oriented;
/* ian_canvas_place with the oriented gather in place of the box mean: GIM, then exactly ian_session_open(photos = GIM), and the
   session is placed.  A session already placed (in either form) moves.  shown as for ian_canvas_place.
   -6: no canvas reservation, or an edges table is reserved.  -7, naming the item, before anything is enqueued: n outside 1..256, an
   id or a canvas outside its range, a canvas never put, L2 outside 2^32..2^40, a gather sample off the canvas, an id given twice, a
   ninth session on one canvas, a canvas that holds placements of the other form. */
int ian_place_oriented(ian_handle* h, int32_t n, const ian_canvas_oriented* items, uint8_t* shown, void* stream);
/* The oriented sessions placed on one canvas, in ascending session id -> out8 (host; room for IAN_CANVAS_MAX_PLACED) and their
   count.  Host only. */
int ian_placements_oriented(ian_handle* h, int32_t canvas, ian_canvas_oriented* out8, int32_t* count);

/* ---- display-ready pixels: interleaved RGB, RGBA and BGRA out ----
   Whatever shows or saves a picture (a toolkit's image, a browser's ImageData, a texture upload, PIL) takes interleaved pixels; the
   calls above write planes.  The pool has one pixel format for `out` of ian_session_render, ian_canvas_compose, ian_session_zoom,
   ian_session_brush_zoom, ian_compose_zoom, ian_compose_brush_zoom, ian_session_brush_view, ian_session_brush_tip with views and
   ian_canvas_brush, at every zoom, with or without a guide or an edges table, for upright and oriented canvases:
     0  planar (the default)  u8[n,3,vh,vw], exactly as documented with each call
     1  rgb                   u8[n,vh,vw,3]
     2  rgba                  u8[n,vh,vw,4], A = 255
     3  bgra                  u8[n,vh,vw,4], A = 255
   Window i starts at out + i * vh * vw * bytes-per-pixel.  Every byte is the byte format 0 gives for that pixel and channel
   (npe_ops.pack_window of the planar result); the device stores a lane's four pixels at once, 12 or 16 consecutive bytes, and no
   planar copy is written on the way.  What the calls check stays: x and vw multiples of 4, out 4-byte aligned.
   Not governed: shown (64x64, planar), ian_session_read, ian_canvas_read, and what is written in place (ian_canvas_commit,
   ian_session_open(source = 1)): the stored pictures stay planar, and ian_canvas_put / ian_session_open_hires keep taking planes.
   The format is a setting of the pool, not session state: records, history and ian_session_read know nothing of it.  Host only: no
   device state is touched, nothing is synchronised, and the next call is the first under the new format.  ian_sessions_reserve(0)
   puts it back to 0, a resize keeps it.
   -6 without ian_sessions_reserve.  -7: a format outside 0..3; the previous format stays in force. */
int ian_sessions_set_pixels(ian_handle* h, int32_t format);
/* The format in force, 0..3; -6 without ian_sessions_reserve. */
int ian_sessions_pixels(ian_handle* h);

/* The 256 float32 values the open kernel maps uint8 levels to: np.float32(2.0 * (level / 255.0) - 1.0), i.e. NPE.py:257's
   np.asarray([to_tanh(IM)], dtype=np.float32) per level.  Needs no handle and no device. */
void ian_session_tanh_table(float* out256);

/* Introspection used by tests, bench.py and profiling (not part of the reference surface). */
/* Copy the activation of tensor slot `slot` from the last call, converted to NCHW, into out (host or device). */
int ian_read_slot(ian_handle* h, int32_t slot, int32_t n, float* out, void* stream);
/* Same for the gradient buffer the last ian_grad_* call left in `slot`: d loss / d (pre-epilogue value of the
   slot's producer), i.e. before batch-norm scale and activation (NCHW). */
int ian_read_slot_grad(ian_handle* h, int32_t slot, int32_t n, float* out, void* stream);
/* Name and accumulated device time (ms, HIP events on `stream`) of the dominant kernel family since the last reset. */
int ian_profile_enable(ian_handle* h, int32_t on);
int ian_profile_read(ian_handle* h, double* tapgemm_ms, int64_t* tapgemm_launches, double* tapgemm_flops,
                     double* total_ms);
/* Time candidate (tile shape, split-K) decompositions of every tapgemm layer for batch n on this device and keep
   the fastest.  what: bit 0 = forward ops (needs one prior forward call with batch >= n), bit 1 = latent-brush
   backward chain (n must be 1, needs one prior ian_grad_* call).  Results are identical for every choice up to
   float32 summation order; without this call a static heuristic is used. */
int ian_autotune(ian_handle* h, int32_t n, int32_t what, void* stream);
/* Tuning knobs (tile shape / split-K policy); key=value, returns <0 on unknown key. */
int ian_set_option(ian_handle* h, const char* key, int32_t value);

/* Box fingerprint for the bench line (no reference counterpart: the reference has no measurement code; it makes driver numbers
   from different boxes comparable).  Runs `launches` back-to-back launches of a register-only v_mfma_f32_32x32x2_f32 loop of
   `iters` x 4 MFMAs per wave (2 workgroups of 4 waves on each of the 256 CUs, non-zero operands, no memory traffic) on the
   current device's `stream` and returns the sustained fp32 matrix rate in TFLOP/s and the mean launch duration in microseconds.
   iters = 900 gives launches of ~200 us (one IAN_simple batch-64 layer), 3200 ~700 us.  Needs no handle.  0 = ok, <0 = HIP error. */
int ian_box_probe(int32_t iters, int32_t launches, double* tflops, double* us_per_launch, void* stream);

const char* ian_last_error(ian_handle* h);
const char* ian_version(void);
void ian_destroy(ian_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* IAN_H_ */
