// Device-resident edit sessions (ian_session_*, include/ian.h): the state NPE.py's callbacks keep in host globals -- GIM, IM, RECON,
// ERROR, Z, SAMPLE_FLAG (NPE.py:239-279, 317-345) -- lives in a per-handle pool in HBM, indexed by session id.  These kernels are
// the pool's side of every call: bandwidth and latency work (a few 12 KB / 48 KB rows per session), never MFMA.
//   session_open_in_kernel     infer / Reset / UpdateGIM, input side: uint8 photo -> GIM, IM and the encoder's float32 input
//   session_store_kernel       infer / Reset / sample, output side: RECON, ERROR, Z, mode flag, the canvas image
//   session_gather_z_kernel    brush: the sessions' latents -> the decoder's latent slot
//   session_blend_kernel       brush / paint_latents: photo blend (photo mode) or uint8 image (sample mode) per session, z_new -> pool
//   session_blend_local_kernel the same in a pool with the local reservation: per-session user mask, brush footprint, dampen
//   session_local_set_kernel   local edits: a session's UMASK := 0 (every open) and its LOCAL flags (ian_session_local)
//   session_stroke_umask_kernel  strokes: the footprints of all of a stroke's rectangles max-ed into the session's UMASK
//   session_tip_umask_kernel   the same for the items that name a brush tip: the tip's own shape in the place of the rectangle
//   session_fit_begin_kernel / _adam_kernel / _loss_kernel  ian_session_fit: IM := GIM, one Adam step on the latent rows, the loss read-out
//   session_hires_open_kernel  full-resolution open: the photo at its own size -> SRC, its exact box mean -> GIM, IM, encoder input
//   canvas_place_kernel        canvases: the exact box mean of a square of a whole photo -> GIM, IM, encoder input (any byte alignment)
//   canvas_place_oriented_kernel   the same for a square of any size and tilt: n x n nearest-pixel samples per field pixel, in integers
//   session_history_save_kernel / _move_kernel  undo history: a session's Z and UMASK rows to and from its ring of saved states
//   session_pack_kernel / session_unpack_kernel  saved sessions: every row of a session, its ring included, to and from one record
// The kernels that show a window of a full-resolution picture or of a canvas (render, compose, their zoomed views) are in
// kernels_window.hip.
// Every image row is addressed as pool + id * 12288: consecutive lanes touch consecutive bytes (uchar4 / float4 per lane).
#include <cstring>
#include <type_traits>

#include "ian_internal.h"

namespace ian {

// ---- undo history: copies between a session's live rows and its ring of saved states, one workgroup per session -------
// A saved state is the session's Z row and, in a pool that had the local reservation when the history was reserved, its UMASK row.
// Slot k of session id is row id * (depth + 1) + k of SessionRings' hist_z / hist_umask (size_t throughout).  Nothing is computed, so contraction does
// not matter here.  A lane moves 16 bytes at consecutive addresses: double2 for UMASK (2048 per row), float4 for Z when vec != 0 (the
// launcher sets it when zl and every row stride are multiples of 4 floats: both shipped configs, zl = 100), otherwise float by
// float; vec is uniform over the launch.
constexpr int HIST_T = 256;
__device__ __forceinline__ void hist_copy_z(float* dst, const float* src, int zl, int vec) {
  if (vec) {
    for (int j = threadIdx.x; j < (zl >> 2); j += HIST_T) reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[j];
  } else {
    for (int j = threadIdx.x; j < zl; j += HIST_T) dst[j] = src[j];
  }
}
__device__ __forceinline__ void hist_copy_umask(double* dst, const double* src) {
  for (int j = threadIdx.x; j < 64 * 64 / 2; j += HIST_T) reinterpret_cast<double2*>(dst)[j] = reinterpret_cast<const double2*>(src)[j];
}

// mark: slot save[i] of session ids[i] := its live state
__global__ __launch_bounds__(HIST_T) void session_history_save_kernel(SessionPool P, SessionRings R, const int* __restrict__ ids,
                                                                      const int* __restrict__ save, int vec) {
  const int i = blockIdx.x;
  const int id = ids[i], sv = save[i];
  if ((unsigned)sv > (unsigned)R.depth) return;   // never sent by the host; a slot outside the ring is not written
  const size_t row = (size_t)id * (R.depth + 1) + sv;
  hist_copy_z(R.hist_z + row * P.zl, P.z + (size_t)id * P.zl, P.zl, vec);
  if (R.hist_umask) hist_copy_umask(R.hist_umask + row * (64 * 64), P.umask + (size_t)id * (64 * 64));
}
hipError_t launch_session_history_save(const SessionPool& P, const SessionRings& R, const int* ids, const int* save, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || !R.hist_z || !P.z || R.depth < 1 || (R.hist_umask && !P.umask)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_history_save_kernel, dim3(n), dim3(HIST_T), 0, s, P, R, ids, save, (P.zl & 3) == 0 ? 1 : 0);
  return hipGetLastError();
}

// undo / redo: where save[i] >= 0 the live state goes to that slot first (the tip, so that redo can come back to it); then slot
// load[i] goes to row i of the decoder's latent slot (stride zs, as session_gather_z_kernel writes it; the blend that follows writes
// the row back to the session's Z) and to the session's UMASK row.
// No barrier between the two copies: the load overwrites the UMASK row the save has just read, but lane t saves exactly the 16-byte
// pieces t, t + 256, ... that it later overwrites (hist_copy_umask walks the row the same way both times), so every piece is read
// and written by one lane, in program order.  Z is saved from the session's row and loaded into the latent slot: no overlap at all.
__global__ __launch_bounds__(HIST_T) void session_history_move_kernel(SessionPool P, SessionRings R, const int* __restrict__ ids,
                                                                      const int* __restrict__ save, const int* __restrict__ load,
                                                                      float* zslot, int zs, int vec) {
  const int i = blockIdx.x;
  const int id = ids[i], sv = save[i], ld = load[i];
  if ((unsigned)ld > (unsigned)R.depth || sv > R.depth) return;   // never sent by the host
  const size_t ring = (size_t)id * (R.depth + 1);
  double* um = R.hist_umask ? P.umask + (size_t)id * (64 * 64) : nullptr;
  if (sv >= 0) {
    hist_copy_z(R.hist_z + (ring + sv) * P.zl, P.z + (size_t)id * P.zl, P.zl, vec);
    if (um) hist_copy_umask(R.hist_umask + (ring + sv) * (64 * 64), um);
  }
  hist_copy_z(zslot + (size_t)i * zs, R.hist_z + (ring + ld) * P.zl, P.zl, vec);
  if (um) hist_copy_umask(um, R.hist_umask + (ring + ld) * (64 * 64));
}
hipError_t launch_session_history_move(const SessionPool& P, const SessionRings& R, const int* ids, const int* save, const int* load,
                                       float* zslot, int zs, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || !R.hist_z || !P.z || R.depth < 1 || (R.hist_umask && !P.umask) || !zslot || zs < P.zl) return hipErrorInvalidValue;
  const int vec = (P.zl & 3) == 0 && (zs & 3) == 0 && (reinterpret_cast<uintptr_t>(zslot) & 15) == 0;
  hipLaunchKernelGGL(session_history_move_kernel, dim3(n), dim3(HIST_T), 0, s, P, R, ids, save, load, zslot, zs, vec);
  return hipGetLastError();
}

// ---- saved sessions: the pool's rows of n sessions <-> n records, grid (chunks of the record, n) ---------------------
// A record's body is every array of the pool, each padded to 16 bytes (SessionRecordCols, built by the runtime from SESS_COLUMNS).  A
// lane owns REC_PIECES pieces of 16 body bytes, REC_T * 16 bytes apart: consecutive lanes, consecutive addresses on the body's side
// always, and on the pool's side wherever a row (a ring slot) is a multiple of 16 bytes -- the images, ERROR, FIELD, UMASK, SRC, the
// rings, Z at 100 latents.  The 4-byte arrays (MODE, FIELD_KIND, LOCAL) and a Z row whose size is no multiple of 16 move word by word
// on the pool's side.  Which array a piece belongs to is found by walking the table (at most 13 entries, uniform loads); a chunk
// may span several arrays.  The kernels take the table and the arrays' pointers (SessionRecordBases: the launchers read them out of
// SessionPool / SessionRings through the table's member offsets) by value.  Nothing is computed.
// Canonical form: history entry k sits in ring slot (base + k) % slots and goes to record slot k; record slots >= the history's
// length, the SRC row of a session without a source and the padding are zero in the record and are not written back.
constexpr int REC_T = 256, REC_PIECES = 4, REC_CHUNK = REC_T * 16 * REC_PIECES;
struct RecSel {
  char* base;
  unsigned off, unit, slots, rule;
};
__device__ __forceinline__ RecSel rec_select(const SessionRecordCols& T, const SessionRecordBases& B, unsigned o) {
  RecSel s = {nullptr, 0u, 16u, 0u, 0u};   // slots 0: nothing to move (never selected: the first array starts at 0)
#pragma unroll
  for (int k = 0; k < SESS_REC_MAX_COLS; ++k) {
    if (k >= T.ncols) break;
    const SessionRecordCol c = T.col[k];
    if (o >= c.off) {
      s.base = B.p[k]; s.off = c.off; s.unit = c.unit; s.slots = c.slots; s.rule = c.rule;
    }
  }
  return s;
}
// where the `w`-th byte of an array's part of the record lives in the pool; nullptr: zero in the record, not written back
__device__ __forceinline__ char* rec_addr(const RecSel& s, const int4 it, unsigned w, bool rotate) {
  if (w >= s.unit * s.slots) return nullptr;                       // padding
  if (s.rule == SESS_REC_SOURCE && !it.y) return nullptr;          // no source
  size_t row = (size_t)it.x;
  if (s.rule == SESS_REC_RING) {
    const unsigned k = w / s.unit;
    if (k >= (unsigned)it.w) return nullptr;                       // not an entry of the history
    row = row * s.slots + (rotate ? ((unsigned)it.z + k) % s.slots : k);
    w -= k * s.unit;
  }
  return s.base + row * s.unit + w;
}

// One walk for both directions.  PACK: the pool's side is loaded (ring slots rotated into canonical order) and the record stored;
// otherwise the record is loaded and the pool's side stored (the ring restarts at slot 0: no rotation).  Either way all loads of a
// lane's REC_PIECES pieces are issued before its stores.
template <bool PACK>
using RecBody = std::conditional_t<PACK, unsigned char, const unsigned char>;
template <bool PACK>
__device__ __forceinline__ void session_record_walk(const SessionRecordCols& T, const SessionRecordBases& B, const int* __restrict__ items,
                                                    RecBody<PACK>* __restrict__ body) {
  const int i = blockIdx.y;
  const int4 it = reinterpret_cast<const int4*>(items)[i];
  RecBody<PACK>* rec = body + (size_t)i * T.body_bytes;
  uint4 v[REC_PIECES];
  // the pool's side of piece p (already loaded into / still to be stored from v[p]); the 16-byte path or word by word
  auto pool_side = [&](int p, unsigned o) {
    const RecSel s = rec_select(T, B, o);
    const unsigned w = o - s.off;
    if ((s.unit & 15u) == 0) {
      if (char* a = rec_addr(s, it, w, PACK)) {
        if constexpr (PACK) v[p] = *reinterpret_cast<const uint4*>(a);
        else *reinterpret_cast<uint4*>(a) = v[p];
      }
    } else {
      unsigned t[4] = {v[p].x, v[p].y, v[p].z, v[p].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (char* a = rec_addr(s, it, w + 4u * j, PACK)) {
          if constexpr (PACK) t[j] = *reinterpret_cast<const unsigned*>(a);
          else *reinterpret_cast<unsigned*>(a) = t[j];
        }
      if constexpr (PACK) v[p] = make_uint4(t[0], t[1], t[2], t[3]);
    }
  };
#pragma unroll
  for (int p = 0; p < REC_PIECES; ++p) {
    const unsigned o = blockIdx.x * (unsigned)REC_CHUNK + (unsigned)(p * REC_T + threadIdx.x) * 16u;
    v[p] = make_uint4(0u, 0u, 0u, 0u);
    if (o >= T.body_bytes) continue;
    if constexpr (PACK) pool_side(p, o);
    else v[p] = *reinterpret_cast<const uint4*>(rec + o);
  }
#pragma unroll
  for (int p = 0; p < REC_PIECES; ++p) {
    const unsigned o = blockIdx.x * (unsigned)REC_CHUNK + (unsigned)(p * REC_T + threadIdx.x) * 16u;
    if (o >= T.body_bytes) continue;
    if constexpr (PACK) *reinterpret_cast<uint4*>(rec + o) = v[p];
    else pool_side(p, o);
  }
}
__global__ __launch_bounds__(REC_T) void session_pack_kernel(SessionRecordCols T, SessionRecordBases B, const int* __restrict__ items,
                                                             unsigned char* __restrict__ body) {
  session_record_walk<true>(T, B, items, body);
}
__global__ __launch_bounds__(REC_T) void session_unpack_kernel(SessionRecordCols T, SessionRecordBases B, const int* __restrict__ items,
                                                               const unsigned char* __restrict__ body) {
  session_record_walk<false>(T, B, items, body);
}
// What both launchers refuse: a table that does not describe these arrays (every offset and size is checked here, so that no lane
// can be sent outside a row), a body that is not 16-byte aligned.  -> B: the arrays' pointers, taken out of P and R here: a kernel
// that picked a member of a by-value struct by a run-time offset would keep the struct in scratch memory.
static bool session_record_args_ok(const SessionPool& P, const SessionRings& R, const SessionRecordCols& T, const int* items,
                                   const void* body, int n, SessionRecordBases& B) {
  if (n < 1 || n > 65535 || !items || !body || (reinterpret_cast<uintptr_t>(body) & 15) || (reinterpret_cast<uintptr_t>(items) & 15)) return false;
  if (T.ncols < 1 || T.ncols > SESS_REC_MAX_COLS || T.body_bytes == 0 || (T.body_bytes & 15u) || T.col[0].off != 0) return false;
  memset(&B, 0, sizeof B);
  unsigned long long end = 0;
  for (int k = 0; k < T.ncols; ++k) {
    const SessionRecordCol& c = T.col[k];
    const size_t holder = c.in_rings ? sizeof(SessionRings) : sizeof(SessionPool);
    if (c.off != end || c.unit == 0 || (c.unit & 3u) || c.slots < 1 || c.member + sizeof(void*) > holder || c.rule > SESS_REC_RING) return false;
    if (c.rule == SESS_REC_RING && (!c.in_rings || c.slots != (unsigned)R.depth + 1)) return false;
    if (c.rule != SESS_REC_RING && c.slots != 1) return false;
    memcpy(&B.p[k], (c.in_rings ? reinterpret_cast<const char*>(&R) : reinterpret_cast<const char*>(&P)) + c.member, sizeof B.p[k]);
    if (!B.p[k]) return false;
    end += ((unsigned long long)c.unit * c.slots + 15ull) & ~15ull;
    if (end > 0x7fffffffull) return false;
  }
  return end == T.body_bytes;
}
template <typename Body>
static hipError_t launch_session_record(void (*kernel)(SessionRecordCols, SessionRecordBases, const int*, Body*), const SessionPool& P,
                                        const SessionRings& R, const SessionRecordCols& T, const int* items, Body* body, int n, hipStream_t s) {
  SessionRecordBases B;
  if (!session_record_args_ok(P, R, T, items, body, n, B)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((T.body_bytes + REC_CHUNK - 1) / REC_CHUNK, n), dim3(REC_T), 0, s, T, B, items, body);
  return hipGetLastError();
}
hipError_t launch_session_pack(const SessionPool& P, const SessionRings& R, const SessionRecordCols& T, const int* items,
                               unsigned char* body, int n, hipStream_t s) {
  return launch_session_record(session_pack_kernel, P, R, T, items, body, n, s);
}
hipError_t launch_session_unpack(const SessionPool& P, const SessionRings& R, const SessionRecordCols& T, const int* items,
                                 const unsigned char* body, int n, hipStream_t s) {
  return launch_session_record(session_unpack_kernel, P, R, T, items, body, n, s);
}

}  // namespace ian

#include "npe_blend.h"   // floating-point contraction off from here on; np_uint8f, photo_blend_image
#include "ian_fit_step.h"   // ian_fit_adam_step

namespace ian {

constexpr int S_IMG = 3 * 64 * 64;

// the host's to_tanh table of the 256 uint8 levels (ian_session_tanh_table) -> LDS.  The barrier also publishes whatever the caller
// wrote to LDS before the call.  T: the workgroup's size where the kernel fixes it (256: one load and one store per lane, no loop
// left), 0: whatever the launch chose.
template <int T = 0>
__device__ __forceinline__ void stage_tanh_table(float* tab, const float* __restrict__ table) {
  for (int j = threadIdx.x; j < 256; j += T ? T : blockDim.x) tab[j] = table[j];
  __syncthreads();
}
// what every open writes per uchar4 at offset o of a 3x64x64 row: GIM and IM of session id, and the encoder's input row i,
// x = np.asarray([to_tanh(IM)], dtype=np.float32) through the table
__device__ __forceinline__ void store_opened_px(const SessionPool& P, int id, int i, size_t o, const uchar4 v, const float* tab,
                                                float* __restrict__ x) {
  *reinterpret_cast<uchar4*>(P.gim + (size_t)id * S_IMG + o) = v;
  *reinterpret_cast<uchar4*>(P.im + (size_t)id * S_IMG + o) = v;
  *reinterpret_cast<float4*>(x + (size_t)i * S_IMG + o) = make_float4(tab[v.x], tab[v.y], tab[v.z], tab[v.w]);
}

// ---- open, input side (NPE.py:244-257 infer, :332-333 Reset, :344 UpdateGIM) --------------------------------------------------
// grid (S_IMG / 1024, n), a lane owns 4 consecutive bytes.  The source row is photos[i] (a new photo), the session's GIM (Reset) or
// its IM (UpdateGIM); it becomes GIM and IM, and x[i] = np.asarray([to_tanh(IM)], dtype=np.float32): the host builds `table` with
// exactly that expression for the 256 levels (float64, one rounding), so the encoder sees the bits the host path uploads.
__global__ __launch_bounds__(256) void session_open_in_kernel(const unsigned char* __restrict__ photos, SessionPool P,
                                                              const int* __restrict__ ids, int source, const float* __restrict__ table,
                                                              float* __restrict__ x) {
  __shared__ float tab[256];
  stage_tanh_table<256>(tab, table);
  const int i = blockIdx.y;
  const int id = ids[i];
  const size_t row = (size_t)id * S_IMG;
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
  const unsigned char* src = photos ? photos + (size_t)i * S_IMG : (source == 1 ? P.im + row : P.gim + row);
  store_opened_px(P, id, i, e, *reinterpret_cast<const uchar4*>(src + e), tab, x);
}
hipError_t launch_session_open_in(const unsigned char* photos, const SessionPool& P, const int* ids, int source, const float* table,
                                  float* x, int n, hipStream_t s) {
  if (n < 1 || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_open_in_kernel, dim3(S_IMG / 1024, n), dim3(256), 0, s, photos, P, ids, source, table, x);
  return hipGetLastError();
}

__device__ __forceinline__ float to_tanh_f32(float v) { return (2.0f * (v / 255.0f)) - 1.0f; }   // to_tanh(np.float32(.)): three roundings
// uint8(from_tanh(x)) of four values (NPE.py:110, :261): to_uint8_kernel's expression (kernels_npe.hip), contraction off
__device__ __forceinline__ uchar4 from_tanh_u8(const float4 v) {
  uchar4 r;
  r.x = np_uint8f(255.0f * (v.x + 1.0f) / 2.0f);
  r.y = np_uint8f(255.0f * (v.y + 1.0f) / 2.0f);
  r.z = np_uint8f(255.0f * (v.z + 1.0f) / 2.0f);
  r.w = np_uint8f(255.0f * (v.w + 1.0f) / 2.0f);
  return r;
}

// ---- open / sample, output side (NPE.py:261-270, 323-326, 335-338) ---------------------------------------------------------
//   RECON = uint8(from_tanh(x))            from_tanh_u8
//   ERROR = to_tanh(float32(IM)) - to_tanh(float32(RECON))       float32, numpy's order, no contraction
// both scattered to the session's rows; the latent row of the z slot goes to the session's Z, the mode flag is set, and the canvas
// image (IM after an open, RECON after a sample) is written to shown[i] when asked for.
__global__ __launch_bounds__(256) void session_store_kernel(const float* __restrict__ xhat, const float* __restrict__ zslot, int zs,
                                                            SessionPool P, const int* __restrict__ ids, int new_mode, int shown_recon,
                                                            unsigned char* __restrict__ shown) {
  const int i = blockIdx.y;
  const int id = ids[i];
  const size_t row = (size_t)id * S_IMG;
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
  const float4 v = *reinterpret_cast<const float4*>(xhat + (size_t)i * S_IMG + e);
  const uchar4 r = from_tanh_u8(v);
  const uchar4 a = *reinterpret_cast<const uchar4*>(P.im + row + e);
  float4 err;
  err.x = to_tanh_f32((float)a.x) - to_tanh_f32((float)r.x);
  err.y = to_tanh_f32((float)a.y) - to_tanh_f32((float)r.y);
  err.z = to_tanh_f32((float)a.z) - to_tanh_f32((float)r.z);
  err.w = to_tanh_f32((float)a.w) - to_tanh_f32((float)r.w);
  *reinterpret_cast<uchar4*>(P.recon + row + e) = r;
  *reinterpret_cast<float4*>(P.error + row + e) = err;
  if (shown) *reinterpret_cast<uchar4*>(shown + (size_t)i * S_IMG + e) = shown_recon ? r : a;
  // full-resolution pools: a sample displays x itself (kind 1), an open / Reset / commit the unedited photo (a zero field, kind 0)
  if (P.field) *reinterpret_cast<float4*>(P.field + row + e) = new_mode ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  if (blockIdx.x == 0) {
    for (int j = threadIdx.x; j < P.zl; j += 256) P.z[(size_t)id * P.zl + j] = zslot[(size_t)i * zs + j];
    if (threadIdx.x == 0) {
      P.mode[id] = new_mode;
      if (P.kind) P.kind[id] = new_mode;
    }
  }
}
hipError_t launch_session_store(const float* xhat, const float* zslot, int zs, const SessionPool& P, const int* ids, int new_mode,
                                int shown_recon, unsigned char* shown, int n, hipStream_t s) {
  if (n < 1 || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_store_kernel, dim3(S_IMG / 1024, n), dim3(256), 0, s, xhat, zslot, zs, P, ids, new_mode, shown_recon, shown);
  return hipGetLastError();
}

// ---- brush: the sessions' latents into the decoder's latent slot (row i = session ids[i]; the slot's channel padding stays zero) ----
__global__ __launch_bounds__(128) void session_gather_z_kernel(SessionPool P, const int* __restrict__ ids, float* __restrict__ zslot, int zs) {
  const int i = blockIdx.x;
  const size_t src = (size_t)ids[i] * P.zl;
  for (int j = threadIdx.x; j < P.zl; j += 128) zslot[(size_t)i * zs + j] = P.z[src + j];
}
hipError_t launch_session_gather_z(const SessionPool& P, const int* ids, float* zslot, int zs, int n, hipStream_t s) {
  if (n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_gather_z_kernel, dim3(n), dim3(128), 0, s, P, ids, zslot, zs);
  return hipGetLastError();
}

// ---- brush / paint_latents, output side: one workgroup per item ---------------------------------------------------------------
// A paint event (items[7*i + 4] == 1; items == nullptr: paint_latents) on a session in photo mode: photo_blend_image (NPE.py:218-231 /
// 296-300) against the session's RECON / ERROR; store != 0 (a brush event) writes the result to the session's IM and copies it to
// shown[i], store == 0 (paint_latents: IM is local to that callback) writes shown[i] only.
// A session in sample mode, and a lighten event in either mode (NPE.scroll ends in update_photo(None), NPE.py:313-314):
// shown[i] = uint8(from_tanh(x)) (NPE.py:110), IM untouched.  The item's latent row goes back to the pool.
// LOCAL: a pool with the local reservation (ian_sessions_reserve_local).  The session's LOCAL flags choose, uniformly over the
// workgroup, what the blend does (npe_ops.photo_blend_local).  Bit 0: a paint event first max-es the footprint of its rectangle into
// the session's UMASK (set_latent, items == nullptr, adds none), then MASK_L = MASK * UMASK; bit 1: dampen.  Flags 0 take the same
// LOCAL instantiation with both switched off: MASK and D go through the operations of the plain one.  Sample mode and lighten events
// never look at the flags.  Mixed batches are one launch.
template <bool LOCAL>
__device__ __forceinline__ void session_blend_body(const SessionBlendArgs& a, double* m0, double* m1) {
  const int i = blockIdx.y;
  const int id = a.ids[i];
  const size_t row = (size_t)id * S_IMG;
  const float* xh = a.xhat + (size_t)i * S_IMG;
  unsigned char* sh = a.shown + (size_t)i * S_IMG;
  for (int j = threadIdx.x; j < a.P.zl; j += PB_T) a.P.z[(size_t)id * a.P.zl + j] = a.zslot[(size_t)i * a.zs + j];
  if (a.P.mode[id] != 0 || (a.items && a.items[i * 7 + 4] == 0)) {   // the plain sample (uniform over the workgroup)
    for (int e = threadIdx.x * 4; e < S_IMG; e += PB_T * 4) {
      const float4 v = *reinterpret_cast<const float4*>(xh + e);
      *reinterpret_cast<uchar4*>(sh + e) = from_tanh_u8(v);
      if (a.P.field) *reinterpret_cast<float4*>(a.P.field + row + e) = v;   // full-resolution pools: what is displayed is x (kind 1)
    }
    if (a.P.kind && threadIdx.x == 0) a.P.kind[id] = 1;
    return;
  }
  PhotoLocalArgs l;
  if constexpr (LOCAL) {
    const int flags = a.P.local[id];
    l.umask = (flags & 1) ? a.P.umask + (size_t)id * (64 * 64) : nullptr;
    // an item with a tip under ian_sessions_set_soft_mask has its tip's footprint in UMASK already (session_tip_umask_kernel): the
    // rectangle's would swallow it
    l.falloff = (a.items && !(a.tips && a.tips[i] >= 0)) ? a.falloff : nullptr;
    l.c1 = l.r1 = l.c2 = l.r2 = 0;
    if (a.items) {
      // a rectangle that is empty or not inside the image (the host refuses the latter) adds no footprint: the table has 64 entries
      const int c1 = a.items[i * 7], r1 = a.items[i * 7 + 1], c2 = a.items[i * 7 + 2], r2 = a.items[i * 7 + 3];
      if (c1 >= 0 && r1 >= 0 && c2 <= 64 && r2 <= 64 && c1 < c2 && r1 < r2) {
        l.c1 = c1;
        l.r1 = r1;
        l.c2 = c2;
        l.r2 = r2;
      }
    }
    l.dampen = flags & 2;
    l.thresh = a.thresh;
  }
  PhotoBlendArgs b;
  b.xhat = xh;
  b.recon = a.P.recon + row;
  b.error = a.P.error + row;
  b.im = a.store ? a.P.im + row : sh;
  b.mask = nullptr;
  b.field = a.P.field ? a.P.field + row : nullptr;   // full-resolution pools: the blend as an edit field (kind 0)
#pragma unroll
  for (int k = 0; k < 8; ++k) b.w[k] = a.w[k];
  b.radius = a.radius;
  photo_blend_image<LOCAL>(b, m0, m1, LOCAL ? &l : nullptr);
  if (a.P.kind && threadIdx.x == 0) a.P.kind[id] = 0;
  if (a.store) {   // every thread re-reads exactly the bytes it wrote (p = tid + k * PB_T per channel)
    for (int p = threadIdx.x; p < 64 * 64; p += PB_T)
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[c * 64 * 64 + p] = b.im[c * 64 * 64 + p];
  }
}
__global__ __launch_bounds__(PB_T) void session_blend_kernel(SessionBlendArgs a) {
  __shared__ double m0[64 * 64];
  __shared__ double m1[64 * 64];
  session_blend_body<false>(a, m0, m1);
}
// session_blend_kernel stays the code of every pool without the local reservation
__global__ __launch_bounds__(PB_T) void session_blend_local_kernel(SessionBlendArgs a) {
  __shared__ double m0[64 * 64];
  __shared__ double m1[64 * 64];
  session_blend_body<true>(a, m0, m1);
}
hipError_t launch_session_blend(const SessionBlendArgs& a, int n, hipStream_t s) {
  if (a.radius < 0 || a.radius > 7 || n < 1 || n > 65535 || !a.shown) return hipErrorInvalidValue;
  if (a.P.umask) {
    if (!a.P.local) return hipErrorInvalidValue;
    hipLaunchKernelGGL(session_blend_local_kernel, dim3(1, n), dim3(PB_T), 0, s, a);
  } else {
    hipLaunchKernelGGL(session_blend_kernel, dim3(1, n), dim3(PB_T), 0, s, a);
  }
  return hipGetLastError();
}

// ---- local edits: UMASK row of session ids[i] := 0 (open / Reset / commit: USER_MASK *= 0, NPE.py:267, :337) and, with flags,
// LOCAL[ids[i]] := flags[i] (ian_session_local).  One workgroup per session, a lane stores 16 bytes at a time.
__global__ __launch_bounds__(256) void session_local_set_kernel(SessionPool P, const int* __restrict__ ids, const int* __restrict__ flags) {
  const int i = blockIdx.x;
  const int id = ids[i];
  double2* row = reinterpret_cast<double2*>(P.umask + (size_t)id * (64 * 64));
  for (int j = threadIdx.x; j < 64 * 64 / 2; j += 256) row[j] = make_double2(0.0, 0.0);
  if (flags && threadIdx.x == 0) P.local[id] = flags[i];
}
hipError_t launch_session_local_set(const SessionPool& P, const int* ids, const int* flags, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || !P.umask || !P.local) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_local_set_kernel, dim3(n), dim3(256), 0, s, P, ids, flags);
  return hipGetLastError();
}

// ---- strokes: the footprints of ALL of a stroke's rectangles into the session's UMASK, before its first step --------
// ian_session_stroke blends only the last point of a stroke, and that blend max-es only its own rectangle's footprint into UMASK; the
// per-event calls would have max-ed every point's.  This kernel adds them under exactly the blend's conditions (uniform over the
// workgroup): LOCAL bit 0 of the session, a paint stroke (word 4 of its rows), photo mode.  max is exact and idempotent: the order of
// the points does not matter, and the last footprint added again by the final blend changes nothing.
// One workgroup per stroke.  Lane k < steps fetches the stroke's rectangle of step k into LDS (an empty one, or one that is not inside
// the image -- the host refuses those -- as all zeros: it adds nothing), lanes 0..63 the falloff table.  A lane owns whole pixels: 8
// pairs of neighbours in a row, one 16-byte load and one 16-byte store each (consecutive lanes, consecutive addresses), and in
// between the float64 product falloff[dy] * falloff[dx] of photo_blend_image per point and pixel, on gk's distances
// (PhotoLocalArgs / npe_ops.local_footprint), contraction off.  A stroke without any footprint stores nothing.
// stroke_rects: the fetch, shared with session_tip_umask_kernel.  rows == nullptr: the item's one row g (a brush or clone event).
// -> whether any rectangle adds a footprint; ends in a barrier, every thread of the workgroup calls it.
__device__ __forceinline__ int stroke_rects(const int* __restrict__ items, const int* __restrict__ rows, int steps, int g,
                                            const double* __restrict__ falloff, double* fall, int4* rect) {
  int valid = 0;
  if (threadIdx.x < 64) fall[threadIdx.x] = falloff[threadIdx.x];
  if (threadIdx.x < STROKE_MAX_POINTS) {
    const int k = threadIdx.x;
    int4 r = make_int4(0, 0, 0, 0);
    if (k < steps) {
      const int r0 = rows ? rows[k] : 0;
      if (rows ? g < rows[k + 1] - r0 : k == 0) {
        const int* it = items + (size_t)(r0 + g) * 7;
        const int c1 = it[0], r1 = it[1], c2 = it[2], r2 = it[3];
        if (c1 >= 0 && r1 >= 0 && c2 <= 64 && r2 <= 64 && c1 < c2 && r1 < r2) {
          r = make_int4(c1, r1, c2, r2);
          valid = 1;
        }
      }
    }
    rect[k] = r;
  }
  return __syncthreads_or(valid);
}
__global__ __launch_bounds__(256) void session_stroke_umask_kernel(SessionPool P, const int* __restrict__ ids, const int* __restrict__ items,
                                                                   const int* __restrict__ rows, int steps, int first,
                                                                   const double* __restrict__ falloff, const int* __restrict__ tips) {
  __shared__ double fall[64];
  __shared__ int4 rect[STROKE_MAX_POINTS];
  const int g = first + blockIdx.x;
  const int id = ids[g];
  if (tips && tips[g] >= 0) return;   // session_tip_umask_kernel's
  if (!(P.local[id] & 1) || P.mode[id] != 0 || items[(size_t)(rows[0] + g) * 7 + 4] != 1) return;
  if (!stroke_rects(items, rows, steps, g, falloff, fall, rect)) return;
  double2* row = reinterpret_cast<double2*>(P.umask + (size_t)id * (64 * 64));
  for (int j = threadIdx.x; j < 64 * 64 / 2; j += 256) {
    const int y = j >> 5, x = (j & 31) * 2;
    double2 u = row[j];
    for (int k = 0; k < steps; ++k) {
      const int4 r = rect[k];   // (c1, r1, c2, r2): the same address for every lane
      if (r.z <= r.x) continue;
      const int dy = y < r.y ? r.y - y : (y >= r.w ? y - r.w + 1 : 0);   // 0..63 for 0 <= r1 < r2 <= 64
      const int dx0 = x < r.x ? r.x - x : (x >= r.z ? x - r.z + 1 : 0);
      const int dx1 = x + 1 < r.x ? r.x - x - 1 : (x + 1 >= r.z ? x - r.z + 2 : 0);
      const double fy = fall[dy];
      const double f0 = fy * fall[dx0], f1 = fy * fall[dx1];
      u.x = u.x < f0 ? f0 : u.x;
      u.y = u.y < f1 ? f1 : u.y;
    }
    row[j] = u;
  }
}
hipError_t launch_session_stroke_umask(const SessionPool& P, const int* ids, const int* items, const int* rows, int steps, int first,
                                       const double* falloff, const int* tips, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || first < 0 || steps < 1 || steps > STROKE_MAX_POINTS || !P.umask || !P.local || !P.mode || !ids || !items || !rows ||
      !falloff)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_stroke_umask_kernel, dim3(n), dim3(256), 0, s, P, ids, items, rows, steps, first, falloff, tips);
  return hipGetLastError();
}

// ---- tip-shaped footprints (ian_sessions_set_soft_mask) ----------------------------------------------------------
// The stroke kernel's work for the items that name a tip: npe_ops.tip_footprint of every rectangle of item g, in the place of the
// rectangle's footprint, max-ed into the session's UMASK before the item's first step, under the same workgroup-uniform conditions.
//   R[qy][x] = max_qx s[qy][qx] * t[|x - (c1 + qx)|]      pass one, into LDS: th rows of 64 doubles
//   F[y][x]  = max_qy t[|y - (r1 + qy)|] * R[qy][x]       pass two, max-ed into the lane's pixels
// float64, one product each, contraction off; s = the tip's shape wn / max wn, which the host divided (tip_shape_slot).  Every factor
// is >= 0 and has no NaN, so a maximum may start from 0.  One workgroup per item, its rectangles one after the other: max is exact, so
// any order and any split would give the same bits.  R does not fit beside the blend's two planes, hence the kernel of its own.
// Pass one: wave w owns the tip rows w, w + 4, ...; a lane owns column x, so s[qy][qx] is one address for the whole wave.  Pass two and
// the UMASK traffic are the stroke kernel's: a lane owns 8 pairs of neighbours, one 16-byte load before the first rectangle and one
// 16-byte store after the last.  The host refused every rectangle whose size is not its tip's, and a tip's slot is 64 x 64 whatever its
// size: qy * 64 + qx stays inside it for every rectangle inside the image.
__global__ __launch_bounds__(256) void session_tip_umask_kernel(SessionPool P, const int* __restrict__ ids, const int* __restrict__ items,
                                                                const int* __restrict__ rows, int steps, int first,
                                                                const double* __restrict__ falloff, const int* __restrict__ tips,
                                                                const double* __restrict__ shapes) {
  __shared__ double fall[64];
  __shared__ int4 rect[STROKE_MAX_POINTS];
  __shared__ __attribute__((aligned(16))) double R[64 * 64];   // read as double2 in pass two
  const int g = first + blockIdx.x;
  const int id = ids[g];
  const int tip = tips[g];
  if (tip < 0) return;   // session_stroke_umask_kernel's, or the blend's
  if (!(P.local[id] & 1) || P.mode[id] != 0 || items[(size_t)((rows ? rows[0] : 0) + g) * 7 + 4] != 1) return;
  if (!stroke_rects(items, rows, steps, g, falloff, fall, rect)) return;
  const double* shape = shapes + (size_t)tip * (64 * 64);
  double2* row = reinterpret_cast<double2*>(P.umask + (size_t)id * (64 * 64));
  double2 u[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) u[e] = row[threadIdx.x + e * 256];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  for (int k = 0; k < steps; ++k) {
    const int4 r = rect[k];   // (c1, r1, c2, r2): the same address for every lane
    if (r.z <= r.x) continue;
    const int tw = r.z - r.x, th = r.w - r.y;
    for (int qy = wave; qy < th; qy += 4) {
      const double* srow = shape + qy * 64;
      double m = 0.0;
      for (int qx = 0; qx < tw; ++qx) {
        const int d = lane - (r.x + qx);
        const double v = srow[qx] * fall[d < 0 ? -d : d];
        m = m < v ? v : m;
      }
      R[qy * 64 + lane] = m;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = threadIdx.x + e * 256;
      const int y = j >> 5, x = (j & 31) * 2;
      double2 f = make_double2(0.0, 0.0);
      for (int qy = 0; qy < th; ++qy) {
        const int d = y - (r.y + qy);
        const double fy = fall[d < 0 ? -d : d];
        const double2 rr = *reinterpret_cast<const double2*>(R + qy * 64 + x);
        const double f0 = fy * rr.x, f1 = fy * rr.y;
        f.x = f.x < f0 ? f0 : f.x;
        f.y = f.y < f1 ? f1 : f.y;
      }
      u[e].x = u[e].x < f.x ? f.x : u[e].x;
      u[e].y = u[e].y < f.y ? f.y : u[e].y;
    }
    __syncthreads();   // R is rewritten by the next rectangle
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) row[threadIdx.x + e * 256] = u[e];
}
hipError_t launch_session_tip_umask(const SessionPool& P, const int* ids, const int* items, const int* rows, int steps, int first,
                                    const double* falloff, const int* tips, const double* shapes, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || first < 0 || steps < 1 || steps > STROKE_MAX_POINTS || (!rows && steps != 1) || !P.umask || !P.local || !P.mode ||
      !ids || !items || !falloff || !tips || !shapes)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_tip_umask_kernel, dim3(n), dim3(256), 0, s, P, ids, items, rows, steps, first, falloff, tips, shapes);
  return hipGetLastError();
}

// ---- ian_session_fit: the latent fitted to the session's own photo by Adam steps, all on the device -----------------
// IM := GIM of session ids[i], the first thing Reset does (NPE.py:332): session_store_kernel takes ERROR against IM.  grid (S_IMG / 1024, n),
// a lane owns 4 consecutive bytes.
__global__ __launch_bounds__(256) void session_fit_begin_kernel(SessionPool P, const int* __restrict__ ids) {
  const size_t o = (size_t)ids[blockIdx.y] * S_IMG + (size_t)(blockIdx.x * 256 + threadIdx.x) * 4;
  *reinterpret_cast<uchar4*>(P.im + o) = *reinterpret_cast<const uchar4*>(P.gim + o);
}
hipError_t launch_session_fit_begin(const SessionPool& P, const int* ids, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || !P.gim || !P.im) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_fit_begin_kernel, dim3(S_IMG / 1024, n), dim3(256), 0, s, P, ids);
  return hipGetLastError();
}

// Adam step t of item blockIdx.x: row i of the latent slot (stride zs) moves by ian_fit_adam_step with g = row i of the slot's
// gradient; m and v are rows of the workspace, [n][zl] each.  lr and the step's two bias corrections travel in the launch.
__global__ __launch_bounds__(128) void session_fit_adam_kernel(float* __restrict__ z, const float* __restrict__ g, int zs,
                                                               float* __restrict__ m, float* __restrict__ v, int zl, float lr, float c1,
                                                               float c2) {
  const int i = blockIdx.x;
  for (int j = threadIdx.x; j < zl; j += 128) {
    const size_t o = (size_t)i * zs + j, w = (size_t)i * zl + j;
    float mj = m[w], vj = v[w];
    z[o] = ian_fit_adam_step(z[o], g[o], &mj, &vj, c1, c2, lr);
    m[w] = mj;
    v[w] = vj;
  }
}
hipError_t launch_session_fit_adam(float* z, const float* g, int zs, float* m, float* v, int n, int zl, float lr, float c1, float c2,
                                   hipStream_t s) {
  if (n < 1 || n > 65535 || zl < 1 || zs < zl || !z || !g || !m || !v) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_fit_adam_kernel, dim3(n), dim3(128), 0, s, z, g, zs, m, v, zl, lr, c1, c2);
  return hipGetLastError();
}

// The API.py:64 loss of item blockIdx.x at the image in xhat: the float64 mean of (float64(x) - float64(T))^2 over the item's
// rectangle (words 0..3 of its ian_brush_item row), T = table[GIM byte] of session ids[i]; 0 for an empty rectangle.  One workgroup
// per item.  The order of the sum is fixed: lane t adds the rectangle's elements t, t + 256, ... (channel-major, then rows, then
// columns) in float64, one rounding per product and per sum, then the 256 partial sums meet in an LDS tree, [t] += [t + half].
// The rectangle was checked by the host (inside the image); the extents are clamped at 0 all the same.
__global__ __launch_bounds__(256) void session_fit_loss_kernel(const float* __restrict__ xhat, SessionPool P, const int* __restrict__ ids,
                                                               const int* __restrict__ items, const float* __restrict__ table,
                                                               double* __restrict__ loss, int loss_stride) {
  __shared__ float tab[256];
  __shared__ double part[256];
  stage_tanh_table<256>(tab, table);
  const int i = blockIdx.x;
  const int c1 = items[i * 7], r1 = items[i * 7 + 1];
  const int w = max(0, items[i * 7 + 2] - c1), hgt = max(0, items[i * 7 + 3] - r1);
  const int cnt = 3 * w * hgt;
  const float* xh = xhat + (size_t)i * S_IMG;
  const unsigned char* gim = P.gim + (size_t)ids[i] * S_IMG;
  double acc = 0.0;
  for (int k = threadIdx.x; k < cnt; k += 256) {
    const int co = k / (w * hgt), rem = k - co * (w * hgt);
    const int o = (co * 64 + r1 + rem / w) * 64 + c1 + rem % w;
    const double d = (double)xh[o] - (double)tab[gim[o]];
    acc = acc + d * d;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if (threadIdx.x < half) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[(size_t)i * loss_stride] = cnt > 0 ? part[0] / (double)cnt : 0.0;
}
hipError_t launch_session_fit_loss(const float* xhat, const SessionPool& P, const int* ids, const int* items, const float* table,
                                   double* loss, int loss_stride, int n, hipStream_t s) {
  if (n < 1 || n > 65535 || !xhat || !P.gim || !ids || !items || !table || !loss || loss_stride < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_fit_loss_kernel, dim3(n), dim3(256), 0, s, xhat, P, ids, items, table, loss, loss_stride);
  return hipGetLastError();
}

// ---- full-resolution sessions (the arithmetic is npe_ops.hires_downsample) ---------------------------------------------
// The photo lives in the pool at S x S, S = 64 * scale; the 64x64 state above is that of its exact box mean.  What a call displays is
// kept as FIELD / FIELD_KIND; the kernels that render a window of the picture from them are in kernels_window.hip.

// The box mean of one row of one channel of a session's 64x64 picture: the work of one workgroup in both kernels below.  The row is
// s rows of 64 * s bytes that start `lead` (0..3) bytes into the aligned uchar4 at `in`, `stride` bytes apart.  Lane q owns the
// aligned uchar4 at byte 4q of each of them -- (lead + 64s + 3) / 4 lanes, consecutive lanes, consecutive bytes; the lanes loop when
// that is more than the workgroup -- sums its bytes over the s rows in registers, leaves out the bytes before and behind the square,
// merges the bytes that fall into the same 64x64 pixel and does one LDS add per pixel touched.  Integer sums are exact in any order;
// (sum + s*s/2) / (s*s) is hires_downsample / canvas_crop_mean.  Lanes 0..15 then write GIM, IM and x through store_opened_px.
// COPY: every loaded uchar4 also goes to the same place of `copy` (nullptr: it is there already).
template <bool COPY>
__device__ __forceinline__ void box_mean_row(const unsigned char* in, unsigned char* copy, size_t stride, int lead, int s, const SessionPool& P,
                                             int id, int i, size_t o_row, const float* __restrict__ table, float* __restrict__ x, float* tab,
                                             int* sum) {
  if (threadIdx.x < 64) sum[threadIdx.x] = 0;
  stage_tanh_table(tab, table);
  const int S = 64 * s, nq = (lead + S + 3) >> 2;
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    int acc[4] = {0, 0, 0, 0};
    for (int r = 0; r < s; ++r) {
      const uchar4 v = *reinterpret_cast<const uchar4*>(in + (size_t)r * stride + 4 * q);
      if (COPY && copy) *reinterpret_cast<uchar4*>(copy + (size_t)r * stride + 4 * q) = v;
      acc[0] += v.x;
      acc[1] += v.y;
      acc[2] += v.z;
      acc[3] += v.w;
    }
    int bin = -1, t = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int u = 4 * q + e - lead;   // the byte's column in the square
      if (u < 0 || u >= S) continue;
      const int b = u / s;
      if (b != bin) {
        if (bin >= 0) atomicAdd(&sum[bin], t);
        bin = b;
        t = 0;
      }
      t += acc[e];
    }
    if (bin >= 0) atomicAdd(&sum[bin], t);
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int e = threadIdx.x * 4, d = s * s, half = d / 2;
    uchar4 v;
    v.x = (unsigned char)((sum[e] + half) / d);
    v.y = (unsigned char)((sum[e + 1] + half) / d);
    v.z = (unsigned char)((sum[e + 2] + half) / d);
    v.w = (unsigned char)((sum[e + 3] + half) / d);
    store_opened_px(P, id, i, o_row + e, v, tab, x);
  }
}

// open, input side.  grid (64, 3, n): one workgroup per row of one channel of the 64x64 picture, i.e. scale rows of S bytes of the
// photo, aligned (lead 0: 16 * scale lanes, one pass), each uchar4 copied to SRC on the way (photos == nullptr: the row is there
// already).  photos may be the SRC rows themselves, so neither pointer is __restrict__.
__global__ __launch_bounds__(256) void session_hires_open_kernel(const unsigned char* photos, SessionPool P, const int* __restrict__ ids,
                                                                 const float* __restrict__ table, float* __restrict__ x) {
  __shared__ float tab[256];
  __shared__ int sum[64];
  const int s = P.scale, S = 64 * s;
  const int gy = blockIdx.x, c = blockIdx.y, i = blockIdx.z;
  const int id = ids[i];
  const size_t plane = (size_t)S * S, first = (size_t)gy * s * S;
  unsigned char* dst = P.src + ((size_t)id * 3 + c) * plane + first;
  const unsigned char* in = photos ? photos + ((size_t)i * 3 + c) * plane + first : dst;
  box_mean_row<true>(in, photos ? dst : nullptr, (size_t)S, 0, s, P, id, i, (size_t)c * 64 * 64 + gy * 64, table, x, tab, sum);
}
hipError_t launch_session_hires_open(const unsigned char* photos, const SessionPool& P, const int* ids, const float* table, float* x, int n,
                                     hipStream_t s) {
  if (n < 1 || n > 65535 || P.scale < 1 || P.scale > 16 || !P.src) return hipErrorInvalidValue;
  hipLaunchKernelGGL(session_hires_open_kernel, dim3(64, 3, n), dim3((16 * P.scale + 63) / 64 * 64), 0, s, photos, P, ids, table, x);
  return hipGetLastError();
}

// ---- canvases (the arithmetic is npe_ops.canvas_crop_mean / canvas_ramp / canvas_compose) ------------------------------
// A canvas is a whole photo of w x hgt pixels in rows of C.max_w bytes; a session is placed on it as a square of 64 * s pixels at
// (ox, oy), s per placement.

// place, input side: box_mean_row on a square of a canvas.  grid (64, 3, n): one workgroup per row of one channel of the 64x64
// picture, i.e. s canvas rows of 64 * s bytes starting at byte ox of ANY alignment: lead = ox % 4, 16s lanes when it is 0 and 16s + 1
// otherwise (257 at s = 16: the lanes loop).  The aligned span ends at most at the next multiple of 4 after ox + 64s <= w, and
// w % 4 == 0: inside the picture's row.  No SRC copy.
__global__ __launch_bounds__(256) void canvas_place_kernel(SessionCanvases C, SessionPool P, const int* __restrict__ items,
                                                           const float* __restrict__ table, float* __restrict__ x) {
  __shared__ float tab[256];
  __shared__ int sum[64];
  const int gy = blockIdx.x, c = blockIdx.y, i = blockIdx.z;
  const int id = items[5 * i], cv = items[5 * i + 1], ox = items[5 * i + 2], oy = items[5 * i + 3], s = items[5 * i + 4];
  const int lead = ox & 3;
  const unsigned char* in = C.pix + (((size_t)cv * 3 + c) * C.max_h + (size_t)oy + (size_t)gy * s) * C.max_w + (ox - lead);
  box_mean_row<false>(in, nullptr, (size_t)C.max_w, lead, s, P, id, i, (size_t)c * 64 * 64 + gy * 64, table, x, tab, sum);
}
hipError_t launch_canvas_place(const SessionCanvases& C, const SessionPool& P, const int* items, const float* table, float* x, int n,
                               hipStream_t s) {
  if (n < 1 || n > 65535 || !canvases_ok(C) || !P.gim || !P.im || !items || !table || !x) return hipErrorInvalidValue;
  hipLaunchKernelGGL(canvas_place_kernel, dim3(64, 3, n), dim3(256), 0, s, C, P, items, table, x);
  return hipGetLastError();
}

// place, input side, for an oriented placement (npe_ops.canvas_crop_mean_oriented): grid (64, 3, n) as above, one
// workgroup per row gy of one channel of the 64x64 picture.  The row is n sub-rows of 64n nearest-pixel samples, n = 2^m; a lane owns
// sub-sample column k (and k + 256, ... at n > 4), sums its n samples in a register and does one LDS add into field pixel k >> m.
// The coordinates are the specification's, in 64 bits (U*ax reaches 2^30 and cx2 << (16+m) 2^34).  The host has checked that all
// four corner samples lie on the picture, and X, Y are monotone in (U, V); the clamp only keeps a corrupted table inside the array.
// Along a tilted row consecutive lanes read bytes 1/n of a step apart on a slanted line: the reads are not coalesced.  A place is
// rare and reads at most 3 * (64n)^2 bytes (3 MB at side 1024), so that is left as it is.
__global__ __launch_bounds__(256) void canvas_place_oriented_kernel(SessionCanvases C, SessionPool P, const int* __restrict__ items,
                                                                    const float* __restrict__ table, float* __restrict__ x) {
  __shared__ float tab[256];
  __shared__ int sum[64];
  const int gy = blockIdx.x, c = blockIdx.y, i = blockIdx.z;
  const int* it = items + 6 * i;
  const int id = it[0], cv = it[1], cx2 = it[2], cy2 = it[3], ax = it[4], ay = it[5];
  if (threadIdx.x < 64) sum[threadIdx.x] = 0;
  stage_tanh_table<256>(tab, table);
  const long long L2 = (long long)ax * ax + (long long)ay * ay;
  int m = 0;
  while (m < 4 && (1LL << (32 + 2 * m)) < L2) ++m;   // npe_ops.oriented_derive's m
  const int n = 1 << m, N = 64 * n, sh = 17 + m;
  const long long X00 = (long long)cx2 * (1LL << (16 + m)), Y00 = (long long)cy2 * (1LL << (16 + m));
  const unsigned char* plane = C.pix + ((size_t)cv * 3 + c) * C.max_h * C.max_w;
  for (int k = threadIdx.x; k < N; k += 256) {
    const long long U = 2 * k + 1 - N;
    int acc = 0;
    for (int r = 0; r < n; ++r) {
      const long long V = 2 * (gy * n + r) + 1 - N;
      const long long X = (X00 + U * ax - V * ay) >> sh, Y = (Y00 + U * ay + V * ax) >> sh;
      const int Xc = (int)min(max(X, 0LL), (long long)C.max_w - 1), Yc = (int)min(max(Y, 0LL), (long long)C.max_h - 1);
      acc += plane[(size_t)Yc * C.max_w + Xc];
    }
    atomicAdd(&sum[k >> m], acc);
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int e = threadIdx.x * 4, d = n * n, half = d / 2;
    uchar4 v;
    v.x = (unsigned char)((sum[e] + half) / d);
    v.y = (unsigned char)((sum[e + 1] + half) / d);
    v.z = (unsigned char)((sum[e + 2] + half) / d);
    v.w = (unsigned char)((sum[e + 3] + half) / d);
    store_opened_px(P, id, i, (size_t)c * 64 * 64 + gy * 64 + e, v, tab, x);
  }
}
hipError_t launch_canvas_place_oriented(const SessionCanvases& C, const SessionPool& P, const int* items, const float* table, float* x, int n,
                                        hipStream_t s) {
  if (n < 1 || n > 65535 || !canvases_ok(C) || !P.gim || !P.im || !items || !table || !x) return hipErrorInvalidValue;
  hipLaunchKernelGGL(canvas_place_oriented_kernel, dim3(64, 3, n), dim3(256), 0, s, C, P, items, table, x);
  return hipGetLastError();
}

}  // namespace ian
