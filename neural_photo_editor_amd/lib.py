"""ctypes binding of libian.so (include/ian.h).  No compute happens in Python.

The library is hand-written HIP for gfx950; there is deliberately NO fallback: if it cannot be built
or loaded, or no HIP device is present when a model is finalized, the caller gets an exception.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

IAN_MAX_SCALES = 4


class OpDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("segment", C.c_int32), ("src", C.c_int32), ("src2", C.c_int32), ("src3", C.c_int32),
        ("dst", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32),
        ("act", C.c_int32), ("has_bias", C.c_int32),
        ("flat_c", C.c_int32), ("flat_h", C.c_int32), ("flat_w", C.c_int32),
        ("unflat_c", C.c_int32), ("unflat_h", C.c_int32), ("unflat_w", C.c_int32),
        ("n_scales", C.c_int32), ("scales", C.c_int32 * IAN_MAX_SCALES),
        ("name", C.c_char_p), ("bn_name", C.c_char_p),
    ]


class SlotDesc(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_ops", C.c_int32), ("ops", C.POINTER(OpDesc)), ("n_slots", C.c_int32), ("slots", C.POINTER(SlotDesc)),
        ("x_slot", C.c_int32), ("zpre_slot", C.c_int32), ("z_slot", C.c_int32), ("out_slot", C.c_int32),
        ("num_latents", C.c_int32), ("deconv_flip", C.c_int32),
    ]


EXPORTS = (
    "ian_create", "ian_load_param", "ian_set_made_masks", "ian_finalize", "ian_encode", "ian_decode",
    "ian_encode_pre_iaf", "ian_iaf", "ian_reconstruct", "ian_grad_rgb", "ian_grad_light", "ian_decode_u8", "ian_photo_blend",
    "ian_read_slot", "ian_read_slot_grad",
    "ian_brush_step", "ian_grad_batch", "ian_brush_step_batch",
    "ian_sessions_reserve", "ian_sessions_set_blend", "ian_session_open", "ian_session_set_latent", "ian_session_brush", "ian_session_read",
    "ian_sessions_reserve_hires", "ian_session_open_hires", "ian_session_render", "ian_session_brush_view",
    "ian_sessions_reserve_guide", "ian_sessions_guide",
    "ian_sessions_reserve_local", "ian_sessions_set_local", "ian_session_local",
    "ian_sessions_reserve_history", "ian_session_mark", "ian_session_undo", "ian_session_history",
    "ian_session_fit", "ian_session_stroke", "ian_session_clone",
    "ian_sessions_reserve_tips", "ian_sessions_set_tip", "ian_sessions_tip", "ian_session_brush_tip", "ian_session_path_tip",
    "ian_session_record_info", "ian_session_save", "ian_session_load",
    "ian_sessions_reserve_canvas", "ian_canvas_put", "ian_canvas_place", "ian_canvas_compose", "ian_canvas_brush", "ian_canvas_commit",
    "ian_canvas_read", "ian_canvas_placements",
    "ian_sessions_reserve_edges", "ian_sessions_edges",
    "ian_session_zoom", "ian_session_brush_zoom", "ian_compose_zoom", "ian_compose_brush_zoom",
    "ian_place_oriented", "ian_placements_oriented",
    "ian_sessions_set_pixels", "ian_sessions_pixels",
    "ian_session_stamp_soft", "ian_compose_brush_soft", "ian_sessions_set_soft_mask", "ian_sessions_soft_mask",
    "ian_session_tanh_table", "ian_profile_enable", "ian_profile_read", "ian_autotune", "ian_set_option", "ian_box_probe", "ian_last_error", "ian_version", "ian_destroy",
)

_lib = None


def library_path():
    return _build.LIB


def is_ablation_build():
    """True when the loaded library is libian_ablation.so (IAN_ABLATION_BUILD=1 + IAN_LIB=...): the negative-result variants
    (tapgemm schedules 0 / 3, in-launch split-K combine, kernels_b1.hip, 4-wave tapwgrad tile) exist only there."""
    lib = load_library()
    lib.ian_version.restype = C.c_char_p
    return b"ablation" in (lib.ian_version() or b"")


def load_library():
    """Load (building first if the in-tree .so is absent or stale and hipcc exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    override = os.environ.get("IAN_LIB")     # tests/test_sanitize.py: the ASan/UBSan build of the same sources (build.py, IAN_SANITIZE=1)
    if override:
        if not os.path.exists(override):
            raise RuntimeError("IAN_LIB=%s does not exist" % override)
        path = override
    elif _build.have_hipcc():
        path = _build.build()      # a compile / link error propagates: never run stale kernels behind a failed build
    elif not os.path.exists(path):
        raise RuntimeError("libian.so is missing and hipcc is not available to build it")
    elif not _build.is_fresh():
        raise RuntimeError("libian.so does not match the sources under csrc/ (digest stamp differs) and hipcc is not "
                           "available to rebuild it")
    # Load order matters when PyTorch-ROCm lives in the same process (device buffers, streams, torch.distributed): it ships
    # its own HIP runtime next to the system one libian links.  With torch's loaded first both work side by side (every
    # test and bench.py run that way); with libian's loaded first, libian's runtime finds no device once torch has
    # initialised (measured on the MI355X box: build() followed by smoke() in one process).  So: torch first, if present.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    vp, i32, fp = C.c_void_p, C.c_int32, C.c_void_p
    lib.ian_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(vp)]
    lib.ian_load_param.argtypes = [vp, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), i32]
    lib.ian_set_made_masks.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p, i32]
    lib.ian_finalize.argtypes = [vp]
    for fn in ("ian_encode", "ian_decode", "ian_encode_pre_iaf", "ian_iaf", "ian_reconstruct"):
        getattr(lib, fn).argtypes = [vp, fp, i32, fp, vp]
    lib.ian_grad_rgb.argtypes = [vp, i32, i32, i32, i32, fp, fp, fp, vp]
    lib.ian_grad_light.argtypes = [vp, i32, i32, i32, i32, fp, fp, vp]
    lib.ian_decode_u8.argtypes = [vp, fp, i32, fp, vp]
    lib.ian_photo_blend.argtypes = [vp, fp, fp, fp, fp, i32, fp, fp, vp]
    lib.ian_brush_step.argtypes = [vp, i32, i32, i32, i32, fp, fp, C.c_float, C.c_float, fp, fp, fp, C.POINTER(PhotoArgs), vp]
    lib.ian_grad_batch.argtypes = [vp, i32, C.POINTER(BrushItem), fp, fp, fp, vp]
    lib.ian_brush_step_batch.argtypes = [vp, i32, C.POINTER(BrushItem), fp, fp, fp, fp, fp, C.POINTER(PhotoBatchArgs), vp]
    lib.ian_sessions_reserve.argtypes = [vp, i32]
    lib.ian_sessions_set_blend.argtypes = [vp, fp, i32]
    lib.ian_session_open.argtypes = [vp, i32, fp, fp, i32, fp, vp]
    lib.ian_session_set_latent.argtypes = [vp, i32, fp, fp, i32, fp, vp]
    lib.ian_session_brush.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, vp]
    lib.ian_session_read.argtypes = [vp, i32, i32, fp, vp]
    lib.ian_sessions_reserve_hires.argtypes = [vp, i32]
    lib.ian_session_open_hires.argtypes = [vp, i32, fp, fp, fp, vp]
    lib.ian_session_render.argtypes = [vp, i32, C.POINTER(SessionView), i32, i32, fp, vp]
    lib.ian_session_brush_view.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, C.POINTER(SessionView), i32, i32, fp, vp]
    lib.ian_sessions_reserve_guide.argtypes = [vp, fp, i32]
    lib.ian_sessions_guide.argtypes = [vp, fp]
    lib.ian_sessions_reserve_local.argtypes = [vp, i32]
    lib.ian_sessions_set_local.argtypes = [vp, fp, C.c_double]
    lib.ian_session_local.argtypes = [vp, i32, fp, fp, vp]
    lib.ian_sessions_reserve_history.argtypes = [vp, i32]
    lib.ian_session_mark.argtypes = [vp, i32, fp, vp]
    lib.ian_session_undo.argtypes = [vp, i32, fp, fp, fp, vp]
    lib.ian_session_history.argtypes = [vp, i32, fp]
    lib.ian_session_fit.argtypes = [vp, i32, C.POINTER(SessionFitItem), i32, C.c_float, fp, fp, vp]
    lib.ian_session_stroke.argtypes = [vp, i32, C.POINTER(SessionStroke), i32, C.POINTER(StrokeBox), i32, fp, vp]
    lib.ian_session_clone.argtypes = [vp, i32, C.POINTER(SessionCloneEvent), i32, fp, vp]
    lib.ian_sessions_reserve_tips.argtypes = [vp, i32]
    lib.ian_sessions_set_tip.argtypes = [vp, i32, i32, i32, fp]
    lib.ian_sessions_tip.argtypes = [vp, i32, fp, fp]
    lib.ian_session_brush_tip.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, fp, C.POINTER(SessionView), i32, i32, fp, vp]
    lib.ian_session_path_tip.argtypes = [vp, i32, C.POINTER(SessionStroke), fp, i32, C.POINTER(StrokeBox), i32, fp, vp]
    lib.ian_session_record_info.argtypes = [vp, C.POINTER(SessionMeta), fp, fp]
    lib.ian_session_save.argtypes = [vp, i32, fp, fp, fp, vp]
    lib.ian_session_load.argtypes = [vp, i32, fp, fp, fp, vp]
    lib.ian_sessions_reserve_canvas.argtypes = [vp, i32, i32, i32, i32]
    lib.ian_canvas_put.argtypes = [vp, i32, i32, i32, fp, vp]
    lib.ian_canvas_place.argtypes = [vp, i32, C.POINTER(CanvasPlacement), fp, vp]
    lib.ian_canvas_compose.argtypes = [vp, i32, C.POINTER(CanvasWindow), i32, i32, fp, vp]
    lib.ian_canvas_brush.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, i32, C.POINTER(CanvasWindow), i32, i32, fp, vp]
    lib.ian_canvas_commit.argtypes = [vp, i32, fp, vp]
    lib.ian_canvas_read.argtypes = [vp, i32, fp, fp, vp]
    lib.ian_canvas_placements.argtypes = [vp, i32, C.POINTER(CanvasPlacement), fp]
    lib.ian_sessions_reserve_edges.argtypes = [vp, fp, i32]
    lib.ian_sessions_edges.argtypes = [vp, fp]
    lib.ian_session_zoom.argtypes = [vp, i32, C.POINTER(SessionView), i32, i32, i32, fp, vp]
    lib.ian_session_brush_zoom.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, fp, C.POINTER(SessionView), i32, i32, i32, fp, vp]
    lib.ian_compose_zoom.argtypes = [vp, i32, C.POINTER(CanvasWindow), i32, i32, i32, fp, vp]
    lib.ian_compose_brush_zoom.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, i32, C.POINTER(CanvasWindow), i32, i32, i32, fp, vp]
    lib.ian_place_oriented.argtypes = [vp, i32, C.POINTER(CanvasOriented), fp, vp]
    lib.ian_placements_oriented.argtypes = [vp, i32, C.POINTER(CanvasOriented), fp]
    lib.ian_sessions_set_pixels.argtypes = [vp, i32]
    lib.ian_session_stamp_soft.argtypes = [vp, i32, C.POINTER(SessionCloneEvent), fp, i32, fp, vp]
    lib.ian_compose_brush_soft.argtypes = [vp, i32, C.POINTER(SessionEvent), fp, fp, i32, C.POINTER(CanvasWindow), i32, i32, fp, vp]
    lib.ian_sessions_set_soft_mask.argtypes = [vp, i32]
    lib.ian_sessions_soft_mask.argtypes = [vp, fp]
    lib.ian_sessions_pixels.argtypes = [vp]
    lib.ian_session_tanh_table.argtypes = [fp]
    lib.ian_session_tanh_table.restype = None
    lib.ian_read_slot.argtypes = [vp, i32, i32, fp, vp]
    lib.ian_read_slot_grad.argtypes = [vp, i32, i32, fp, vp]
    lib.ian_profile_enable.argtypes = [vp, i32]
    lib.ian_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double)]
    lib.ian_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.ian_autotune.argtypes = [vp, i32, i32, vp]
    lib.ian_box_probe.argtypes = [i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp]
    lib.ian_last_error.argtypes = [vp]
    lib.ian_last_error.restype = C.c_char_p
    lib.ian_version.restype = C.c_char_p
    lib.ian_destroy.argtypes = [vp]
    lib.ian_destroy.restype = None
    for fn in EXPORTS:
        if fn not in ("ian_last_error", "ian_version", "ian_destroy", "ian_session_tanh_table"):
            getattr(lib, fn).restype = i32
    _lib = lib
    return lib


class PhotoArgs(C.Structure):
    """ian_photo_args (include/ian.h)."""
    _fields_ = [("recon", C.c_void_p), ("error", C.c_void_p), ("gauss_half", C.c_void_p), ("radius", C.c_int32),
                ("im", C.c_void_p), ("mask", C.c_void_p)]


class BrushItem(C.Structure):
    """ian_brush_item (include/ian.h): one edit session's event in ian_grad_batch / ian_brush_step_batch."""
    _fields_ = [("c1", C.c_int32), ("r1", C.c_int32), ("c2", C.c_int32), ("r2", C.c_int32), ("mode", C.c_int32),
                ("coef", C.c_float), ("gscale", C.c_float)]


class PhotoBatchArgs(C.Structure):
    """ian_photo_batch_args (include/ian.h)."""
    _fields_ = [("recon", C.c_void_p), ("error", C.c_void_p), ("gauss_half", C.c_void_p), ("radius", C.c_int32),
                ("im", C.c_void_p), ("mask", C.c_void_p)]


class SessionEvent(C.Structure):
    """ian_session_event (include/ian.h): one brush event on a device-resident edit session (ian_session_brush)."""
    _fields_ = [("session", C.c_int32), ("c1", C.c_int32), ("r1", C.c_int32), ("c2", C.c_int32), ("r2", C.c_int32), ("mode", C.c_int32),
                ("coef", C.c_float), ("gscale", C.c_float), ("rgb", C.c_float * 3)]


class SessionView(C.Structure):
    """ian_session_view (include/ian.h): one window of a full-resolution session (ian_session_render / ian_session_brush_view)."""
    _fields_ = [("session", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


class SessionFitItem(C.Structure):
    """ian_session_fit_item (include/ian.h): one session of ian_session_fit and the rectangle its loss is taken over."""
    _fields_ = [("session", C.c_int32), ("c1", C.c_int32), ("r1", C.c_int32), ("c2", C.c_int32), ("r2", C.c_int32)]


STROKE_MAX_POINTS = 64       # IAN_STROKE_MAX_POINTS (include/ian.h)


class StrokeBox(C.Structure):
    """ian_stroke_box (include/ian.h): one rectangle of a stroke and the gradient scale that goes with it."""
    _fields_ = [("c1", C.c_int32), ("r1", C.c_int32), ("c2", C.c_int32), ("r2", C.c_int32), ("gscale", C.c_float)]


class SessionStroke(C.Structure):
    """ian_session_stroke_item (include/ian.h): one session's stroke in ian_session_stroke: its rectangles boxes[first .. first + count),
    and the mode, coefficient and colour of every point."""
    _fields_ = [("session", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("mode", C.c_int32), ("coef", C.c_float),
                ("rgb", C.c_float * 3)]


CLONE_MAX_STEPS = 64         # IAN_CLONE_MAX_STEPS (include/ian.h)


class SessionCloneEvent(C.Structure):
    """ian_session_clone_event (include/ian.h): one clone event of ian_session_clone: the destination's rectangle is pulled towards the
    rectangle shifted by (dc, dr) of the source session's GIM, IM or RECON (field = SESSION_FIELDS[...])."""
    _fields_ = [("session", C.c_int32), ("c1", C.c_int32), ("r1", C.c_int32), ("c2", C.c_int32), ("r2", C.c_int32), ("source", C.c_int32),
                ("field", C.c_int32), ("dc", C.c_int32), ("dr", C.c_int32), ("coef", C.c_float), ("gscale", C.c_float)]


class CanvasPlacement(C.Structure):
    """ian_canvas_placement (include/ian.h): one session placed on a canvas as a square of 64 * scale pixels at (x, y)."""
    _fields_ = [("session", C.c_int32), ("canvas", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("scale", C.c_int32)]


class CanvasOriented(C.Structure):
    """ian_canvas_oriented (include/ian.h): one session placed on a canvas as a square of any size and tilt: the centre in half pixels
    and the canvas displacement per field pixel in Q16 (npe_ops.oriented_placement)."""
    _fields_ = [("session", C.c_int32), ("canvas", C.c_int32), ("cx2", C.c_int32), ("cy2", C.c_int32), ("ax", C.c_int32), ("ay", C.c_int32)]


class CanvasWindow(C.Structure):
    """ian_canvas_window (include/ian.h): one window of a canvas (ian_canvas_compose / ian_canvas_brush)."""
    _fields_ = [("canvas", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


CANVAS_MAX_PLACED = 8               # IAN_CANVAS_MAX_PLACED


class SessionMeta(C.Structure):
    """ian_session_meta (include/ian.h): the 64-byte meta block of one saved session; npe_ops.SESSION_META_DTYPE is the same bytes."""
    _fields_ = [("magic", C.c_uint32), ("format", C.c_int32), ("num_latents", C.c_int32), ("scale", C.c_int32), ("local", C.c_int32),
                ("depth", C.c_int32), ("has_source", C.c_int32), ("local_flags", C.c_int32), ("hist_len", C.c_int32),
                ("hist_cur", C.c_int32), ("body_bytes", C.c_int64), ("reserved", C.c_int32 * 4)]


SESSION_RECORD_MAX_COLUMNS = 13     # IAN_SESSION_RECORD_MAX_COLUMNS


# enum ian_session_field (include/ian.h): name -> (code, dtype, shape; None = (num_latents,); "S" = (3, 64*scale, 64*scale))
SESSION_FIELDS = {"Z": (0, np.float32, None), "RECON": (1, np.uint8, (3, 64, 64)), "ERROR": (2, np.float32, (3, 64, 64)),
                  "IM": (3, np.uint8, (3, 64, 64)), "GIM": (4, np.uint8, (3, 64, 64)), "MODE": (5, np.int32, (1,)),
                  "FIELD": (6, np.float32, (3, 64, 64)), "FIELD_KIND": (7, np.int32, (1,)), "SOURCE": (8, np.uint8, "S"),
                  "UMASK": (9, np.float64, (64, 64)), "LOCAL": (10, np.int32, (1,))}


def session_tanh_table():
    """ian_session_tanh_table: the float32 value the open kernel gives each uint8 level (needs no device)."""
    out = np.empty(256, np.float32)
    load_library().ian_session_tanh_table(_ptr(out))
    return out


class IanError(RuntimeError):
    pass


def box_probe(iters=900, launches=250, stream=None):
    """ian_box_probe: sustained fp32-MFMA rate of this box (register-only loop, launches of ~200 us at iters = 900).
    -> {"tflops": ..., "us_per_launch": ...}"""
    lib = load_library()
    tf, us = C.c_double(), C.c_double()
    rc = lib.ian_box_probe(int(iters), int(launches), C.byref(tf), C.byref(us), C.c_void_p(stream or 0))
    if rc != 0:
        raise IanError("ian_box_probe failed (%d)" % rc)
    return {"tflops": tf.value, "us_per_launch": us.value}


def _ptr(buf):
    """Raw address of a numpy array (host) or of anything exposing data_ptr() (torch device tensor)."""
    if isinstance(buf, np.ndarray):
        return C.c_void_p(buf.__array_interface__["data"][0])    # (ndarray.ctypes builds a helper object per access: ~1 us each)
    if hasattr(buf, "data_ptr"):
        return C.c_void_p(buf.data_ptr())
    if isinstance(buf, int):
        return C.c_void_p(buf)
    raise TypeError("expected a numpy array, a tensor with data_ptr() or an address")


class Handle:
    """Thin RAII wrapper over ian_handle*."""

    def __init__(self, lowered, deconv_flip=True):
        self.lib = load_library()
        self.lowered = lowered
        n = len(lowered.ops)
        self._keep = []
        ops = (OpDesc * n)()
        for i, op in enumerate(lowered.ops):
            d = ops[i]
            d.kind, d.segment, d.src, d.src2, d.src3, d.dst = op.kind, op.segment, op.src, op.src2, op.src3, op.dst
            d.cin, d.cout, d.in_h, d.in_w, d.act, d.has_bias = op.cin, op.cout, op.in_h, op.in_w, op.act, op.has_bias
            d.flat_c, d.flat_h, d.flat_w = op.flat
            d.unflat_c, d.unflat_h, d.unflat_w = op.unflat
            d.n_scales = len(op.scales)
            for k, s in enumerate(op.scales):
                d.scales[k] = s
            nm = op.name.encode()
            self._keep.append(nm)
            d.name = nm
            if op.bn_name:
                bn = op.bn_name.encode()
                self._keep.append(bn)
                d.bn_name = bn
            else:
                d.bn_name = None
        slots = (SlotDesc * len(lowered.slots))()
        for i, (h, w, c) in enumerate(lowered.slots):
            slots[i].h, slots[i].w, slots[i].c = h, w, c
        desc = ModelDesc(n, ops, len(lowered.slots), slots, lowered.x_slot, lowered.zpre_slot, lowered.z_slot,
                         lowered.out_slot, lowered.num_latents, int(bool(deconv_flip)))
        self._h = C.c_void_p()
        rc = self.lib.ian_create(C.byref(desc), C.byref(self._h))
        if rc != 0:
            raise IanError("ian_create failed (%d)" % rc)

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.ian_last_error(self._h)
            raise IanError("libian error %d: %s" % (rc, msg.decode() if msg else "?"))

    def load_param(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        self._check(self.lib.ian_load_param(self._h, name.encode(), C.c_void_p(a.ctypes.data), shape, a.ndim))

    def set_made_masks(self, m0, m1, md):
        arrs = [np.ascontiguousarray(m, dtype=np.float32) for m in (m0, m1, md)]
        self._check(self.lib.ian_set_made_masks(self._h, *[C.c_void_p(a.ctypes.data) for a in arrs], arrs[0].shape[0]))

    def finalize(self):
        self._check(self.lib.ian_finalize(self._h))

    def call(self, fn, src, n, dst, stream=None):
        self._check(getattr(self.lib, fn)(self._h, _ptr(src), n, _ptr(dst), C.c_void_p(stream or 0)))

    def grad_rgb(self, c1, r1, c2, r2, rgb, z, dz, stream=None):
        self._check(self.lib.ian_grad_rgb(self._h, c1, r1, c2, r2, _ptr(rgb), _ptr(z), _ptr(dz), C.c_void_p(stream or 0)))

    def grad_light(self, c1, r1, c2, r2, z, dz, stream=None):
        self._check(self.lib.ian_grad_light(self._h, c1, r1, c2, r2, _ptr(z), _ptr(dz), C.c_void_p(stream or 0)))

    def photo_blend(self, z, recon_u8, error, gauss_half, im, mask=None, stream=None):
        self._check(self.lib.ian_photo_blend(self._h, _ptr(z), _ptr(recon_u8), _ptr(error), _ptr(gauss_half), len(gauss_half) - 1,
                                             _ptr(im), _ptr(mask) if mask is not None else C.c_void_p(0), C.c_void_p(stream or 0)))

    def brush_step(self, c1, r1, c2, r2, rgb, z, coef, gscale, z_new, dz=None, x=None, photo=None, stream=None):
        """ian_brush_step; photo = (recon_u8, error, gauss_half, im, mask or None)."""
        null = C.c_void_p(0)
        pa = None
        if photo is not None:
            recon, err, half, im, mask = photo
            pa = PhotoArgs(_ptr(recon).value, _ptr(err).value, _ptr(half).value, len(half) - 1, _ptr(im).value,
                           _ptr(mask).value if mask is not None else None)
        self._check(self.lib.ian_brush_step(self._h, c1, r1, c2, r2, _ptr(rgb) if rgb is not None else null, _ptr(z), coef, gscale,
                                            _ptr(z_new), _ptr(dz) if dz is not None else null, _ptr(x) if x is not None else null,
                                            C.byref(pa) if pa is not None else None, C.c_void_p(stream or 0)))

    def grad_batch(self, items, rgb, z, dz, stream=None):
        """ian_grad_batch; items = a ctypes array of BrushItem (n = its length)."""
        self._check(self.lib.ian_grad_batch(self._h, len(items), items, _ptr(rgb) if rgb is not None else C.c_void_p(0), _ptr(z),
                                            _ptr(dz), C.c_void_p(stream or 0)))

    def brush_step_batch(self, items, rgb, z, z_new, dz=None, x=None, photo=None, stream=None):
        """ian_brush_step_batch; photo = (recon_u8 [n,3,64,64], error [n,3,64,64], gauss_half, im [n,3,64,64], mask [n,64,64] or None)."""
        null = C.c_void_p(0)
        pa = None
        if photo is not None:
            recon, err, half, im, mask = photo
            pa = PhotoBatchArgs(_ptr(recon).value, _ptr(err).value, _ptr(half).value, len(half) - 1, _ptr(im).value,
                                _ptr(mask).value if mask is not None else None)
        self._check(self.lib.ian_brush_step_batch(self._h, len(items), items, _ptr(rgb) if rgb is not None else null, _ptr(z),
                                                  _ptr(z_new), _ptr(dz) if dz is not None else null,
                                                  _ptr(x) if x is not None else null, C.byref(pa) if pa is not None else None,
                                                  C.c_void_p(stream or 0)))

    # ---- device-resident edit sessions (ian_session_*) ----
    def sessions_reserve(self, capacity):
        self._check(self.lib.ian_sessions_reserve(self._h, int(capacity)))

    def sessions_set_blend(self, gauss_half):
        half = np.ascontiguousarray(gauss_half, np.float64)
        self._check(self.lib.ian_sessions_set_blend(self._h, _ptr(half), len(half) - 1))

    def session_open(self, ids, photos=None, source=0, shown=None, stream=None):
        """ian_session_open; ids = int32 array (n = its length), photos u8[n,3,64,64] or None, shown u8[n,3,64,64] or None."""
        null = C.c_void_p(0)
        self._check(self.lib.ian_session_open(self._h, len(ids), _ptr(ids), _ptr(photos) if photos is not None else null, int(source),
                                              _ptr(shown) if shown is not None else null, C.c_void_p(stream or 0)))

    def session_set_latent(self, ids, z, as_sample, shown=None, stream=None):
        self._check(self.lib.ian_session_set_latent(self._h, len(ids), _ptr(ids), _ptr(z), int(as_sample),
                                                    _ptr(shown) if shown is not None else C.c_void_p(0), C.c_void_p(stream or 0)))

    def session_brush(self, events, shown=None, stream=None):
        """ian_session_brush; events = a ctypes array of SessionEvent (n = its length)."""
        self._check(self.lib.ian_session_brush(self._h, len(events), events, _ptr(shown) if shown is not None else C.c_void_p(0),
                                               C.c_void_p(stream or 0)))

    def sessions_reserve_hires(self, scale):
        self._check(self.lib.ian_sessions_reserve_hires(self._h, int(scale)))

    def session_open_hires(self, ids, photos, shown=None, stream=None):
        """ian_session_open_hires; ids = int32 array (n = its length), photos u8[n,3,S,S], shown u8[n,3,64,64] or None."""
        self._check(self.lib.ian_session_open_hires(self._h, len(ids), _ptr(ids), _ptr(photos),
                                                    _ptr(shown) if shown is not None else C.c_void_p(0), C.c_void_p(stream or 0)))

    def session_render(self, views, vw, vh, out, stream=None):
        """ian_session_render; views = a ctypes array of SessionView (n = its length), out u8[n,3,vh,vw]."""
        self._check(self.lib.ian_session_render(self._h, len(views), views, int(vw), int(vh), _ptr(out), C.c_void_p(stream or 0)))

    def session_brush_view(self, events, views, vw, vh, out, shown=None, stream=None):
        """ian_session_brush_view; events / views = ctypes arrays of SessionEvent / SessionView of the same length."""
        self._check(self.lib.ian_session_brush_view(self._h, len(events), events, _ptr(shown) if shown is not None else C.c_void_p(0),
                                                    views, int(vw), int(vh), _ptr(out), C.c_void_p(stream or 0)))

    def session_zoom(self, views, vw, vh, zoom, out, stream=None):
        """ian_session_zoom: session_render at 1/zoom; vw, vh = the output size, out u8[n,3,vh,vw]."""
        self._check(self.lib.ian_session_zoom(self._h, len(views), views, int(vw), int(vh), int(zoom), _ptr(out), C.c_void_p(stream or 0)))

    def session_brush_zoom(self, events, tips, shown, views, vw, vh, zoom, out, stream=None):
        """ian_session_brush_zoom: session_brush_view (tips None) or session_brush_tip with views (tips int32[n]) at 1/zoom."""
        self._check(self.lib.ian_session_brush_zoom(self._h, len(events), events, _ptr(tips) if tips is not None else C.c_void_p(0),
                                                    _ptr(shown) if shown is not None else C.c_void_p(0), views, int(vw), int(vh),
                                                    int(zoom), _ptr(out), C.c_void_p(stream or 0)))

    def sessions_reserve_guide(self, table=None):
        """ian_sessions_reserve_guide; table = 766 float32 range weights (npe_ops.guide_table), or None to switch the guide off."""
        if table is None:
            self._check(self.lib.ian_sessions_reserve_guide(self._h, C.c_void_p(0), 0))
            return
        t = np.ascontiguousarray(table, np.float32)
        if t.ndim != 1:
            raise ValueError("the guide table is one-dimensional, got shape %s" % (t.shape,))
        self._check(self.lib.ian_sessions_reserve_guide(self._h, _ptr(t), t.shape[0]))

    def sessions_guide(self):
        """ian_sessions_guide -> the float32[766] table of the reserved guide, or None without one."""
        t = np.empty(766, np.float32)
        rc = self.lib.ian_sessions_guide(self._h, _ptr(t))
        if rc < 0:
            self._check(rc)
        return t if rc == 1 else None

    def sessions_set_pixels(self, fmt):
        """ian_sessions_set_pixels; fmt = 0 planar, 1 rgb, 2 rgba, 3 bgra (npe_ops.PIXEL_FORMATS): what `out` of every window call holds."""
        self._check(self.lib.ian_sessions_set_pixels(self._h, int(fmt)))

    def sessions_pixels(self):
        """ian_sessions_pixels -> the pixel format in force, 0..3."""
        rc = self.lib.ian_sessions_pixels(self._h)
        if rc < 0:
            self._check(rc)
        return rc

    def sessions_reserve_local(self, on=True):
        self._check(self.lib.ian_sessions_reserve_local(self._h, int(bool(on))))

    def sessions_set_local(self, falloff64, dampen_thresh=0.75):
        """ian_sessions_set_local; falloff64 = 64 float64 values (npe_ops.local_falloff_table)."""
        t = np.ascontiguousarray(falloff64, np.float64)
        if t.shape != (64,):
            raise ValueError("the falloff table has 64 entries, got shape %s" % (t.shape,))
        self._check(self.lib.ian_sessions_set_local(self._h, _ptr(t), float(dampen_thresh)))

    def session_local(self, ids, flags, stream=None):
        """ian_session_local; ids, flags = int32 arrays of the same length n."""
        ids, flags = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(flags, np.int32)
        if ids.ndim != 1 or flags.shape != ids.shape:
            raise ValueError("ids and flags must be 1-D arrays of the same length, got %s and %s" % (ids.shape, flags.shape))
        self._check(self.lib.ian_session_local(self._h, len(ids), _ptr(ids), _ptr(flags), C.c_void_p(stream or 0)))

    def sessions_reserve_history(self, depth):
        self._check(self.lib.ian_sessions_reserve_history(self._h, int(depth)))

    def session_mark(self, ids, stream=None):
        """ian_session_mark; ids = int32 array (n = its length)."""
        ids = np.ascontiguousarray(ids, np.int32)
        if ids.ndim != 1:
            raise ValueError("ids must be a 1-D array, got shape %s" % (ids.shape,))
        self._check(self.lib.ian_session_mark(self._h, len(ids), _ptr(ids), C.c_void_p(stream or 0)))

    def session_undo(self, ids, steps=None, shown=None, stream=None):
        """ian_session_undo; ids and steps (or None: one undo each) = int32 arrays of the same length n, shown u8[n,3,64,64] or None."""
        ids = np.ascontiguousarray(ids, np.int32)
        if steps is not None:
            steps = np.ascontiguousarray(steps, np.int32)
        if ids.ndim != 1 or (steps is not None and steps.shape != ids.shape):
            raise ValueError("ids and steps must be 1-D arrays of the same length, got %s and %s" % (ids.shape, None if steps is None else steps.shape))
        null = C.c_void_p(0)
        self._check(self.lib.ian_session_undo(self._h, len(ids), _ptr(ids), _ptr(steps) if steps is not None else null,
                                              _ptr(shown) if shown is not None else null, C.c_void_p(stream or 0)))

    def session_history(self, sid):
        """ian_session_history -> (depth, undoable, redoable) of one opened session; host only."""
        out = np.zeros(3, np.int32)
        self._check(self.lib.ian_session_history(self._h, int(sid), _ptr(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def session_fit(self, items, steps, lr, loss=None, shown=None, stream=None):
        """ian_session_fit; items = a ctypes array of SessionFitItem (n = its length), loss f64[n, steps+1] or None, shown
        u8[n,3,64,64] or None."""
        null = C.c_void_p(0)
        self._check(self.lib.ian_session_fit(self._h, len(items), items, int(steps), float(lr), _ptr(loss) if loss is not None else null,
                                             _ptr(shown) if shown is not None else null, C.c_void_p(stream or 0)))

    def session_stroke(self, strokes, boxes, flags=0, shown=None, stream=None):
        """ian_session_stroke; strokes / boxes = ctypes arrays of SessionStroke (n = its length, counts non-increasing) and StrokeBox,
        flags bit 0 = mark first, shown u8[n,3,64,64] or None."""
        self._check(self.lib.ian_session_stroke(self._h, len(strokes), strokes, len(boxes), boxes, int(flags),
                                                _ptr(shown) if shown is not None else C.c_void_p(0), C.c_void_p(stream or 0)))

    def session_clone(self, events, steps=1, shown=None, stream=None):
        """ian_session_clone; events = a ctypes array of SessionCloneEvent (n = its length), steps 1..CLONE_MAX_STEPS, shown
        u8[n,3,64,64] or None."""
        self._check(self.lib.ian_session_clone(self._h, len(events), events, int(steps), _ptr(shown) if shown is not None else C.c_void_p(0),
                                               C.c_void_p(stream or 0)))

    # ---- brush tips (ian_sessions_reserve_tips, ian_session_brush_tip, ian_session_path_tip) ----
    def sessions_reserve_tips(self, count):
        self._check(self.lib.ian_sessions_reserve_tips(self._h, int(count)))

    def sessions_set_tip(self, tip, wn):
        """ian_sessions_set_tip; wn = float32 [th][tw] weights, taken as given (npe_ops.tip_weights normalises a shape)."""
        wn = np.ascontiguousarray(wn, np.float32)
        if wn.ndim != 2:
            raise ValueError("a tip is a 2-D weight image [th][tw], got shape %s" % (wn.shape,))
        self._check(self.lib.ian_sessions_set_tip(self._h, int(tip), wn.shape[1], wn.shape[0], _ptr(wn)))

    def sessions_tip(self, tip):
        """ian_sessions_tip -> the float32 [th][tw] weights of one tip."""
        wh = np.zeros(2, np.int32)
        self._check(self.lib.ian_sessions_tip(self._h, int(tip), _ptr(wh), C.c_void_p(0)))
        wn = np.empty((int(wh[1]), int(wh[0])), np.float32)
        self._check(self.lib.ian_sessions_tip(self._h, int(tip), _ptr(wh), _ptr(wn)))
        return wn

    def session_brush_tip(self, events, tips, shown=None, views=None, vw=0, vh=0, out=None, stream=None):
        """ian_session_brush_tip; events = a ctypes array of SessionEvent (n = its length), tips = int32[n] (-1: no tip); views (a
        ctypes array of SessionView of the same length) with vw, vh, out as in session_brush_view, or None."""
        tips = np.ascontiguousarray(tips, np.int32)
        if tips.shape != (len(events),):
            raise ValueError("tips must hold one index per event (%d), got shape %s" % (len(events), tips.shape))
        null = C.c_void_p(0)
        self._check(self.lib.ian_session_brush_tip(self._h, len(events), events, _ptr(tips), _ptr(shown) if shown is not None else null,
                                                   views, int(vw), int(vh), _ptr(out) if out is not None else null, C.c_void_p(stream or 0)))

    def session_path_tip(self, strokes, tips, boxes, flags=0, shown=None, stream=None):
        """ian_session_path_tip; the arguments of session_stroke and tips = int32[n], one per stroke (-1: no tip)."""
        tips = np.ascontiguousarray(tips, np.int32)
        if tips.shape != (len(strokes),):
            raise ValueError("tips must hold one index per stroke (%d), got shape %s" % (len(strokes), tips.shape))
        self._check(self.lib.ian_session_path_tip(self._h, len(strokes), strokes, _ptr(tips), len(boxes), boxes, int(flags),
                                                  _ptr(shown) if shown is not None else C.c_void_p(0), C.c_void_p(stream or 0)))

    def session_clone_tip(self, events, tips, steps=1, shown=None, stream=None):
        """ian_session_stamp_soft; the arguments of session_clone and tips = int32[n], one per event (-1: no tip)."""
        tips = np.ascontiguousarray(tips, np.int32)
        if tips.shape != (len(events),):
            raise ValueError("tips must hold one index per event (%d), got shape %s" % (len(events), tips.shape))
        self._check(self.lib.ian_session_stamp_soft(self._h, len(events), events, _ptr(tips), int(steps),
                                                   _ptr(shown) if shown is not None else C.c_void_p(0), C.c_void_p(stream or 0)))

    def sessions_set_tip_footprint(self, on):
        """ian_sessions_set_soft_mask; on = 1: a tipped paint event leaves its tip's shape in the user mask, 0: its rectangle's."""
        self._check(self.lib.ian_sessions_set_soft_mask(self._h, 1 if on else 0))

    def sessions_tip_footprint(self):
        """ian_sessions_soft_mask -> bool, the setting in force."""
        on = np.zeros(1, np.int32)
        self._check(self.lib.ian_sessions_soft_mask(self._h, _ptr(on)))
        return bool(on[0])

    def session_record_info(self):
        """ian_session_record_info -> (the pool's layout as a SessionMeta, the byte offsets of its arrays in a body); host only."""
        layout = SessionMeta()
        offsets = np.zeros(SESSION_RECORD_MAX_COLUMNS, np.int64)
        ncols = np.zeros(1, np.int32)
        self._check(self.lib.ian_session_record_info(self._h, C.byref(layout), _ptr(offsets), _ptr(ncols)))
        return layout, [int(v) for v in offsets[:int(ncols[0])]]

    def session_save(self, ids, meta, body, stream=None):
        """ian_session_save; ids = int32 array (n = its length), meta = n 64-byte entries (host), body = n * body_bytes bytes, a numpy
        array or a device tensor, 16-byte aligned."""
        self._check(self.lib.ian_session_save(self._h, len(ids), _ptr(ids), _ptr(meta), _ptr(body), C.c_void_p(stream or 0)))

    def session_load(self, ids, meta, body, stream=None):
        """ian_session_load; the arguments of session_save, read instead of written."""
        self._check(self.lib.ian_session_load(self._h, len(ids), _ptr(ids), _ptr(meta), _ptr(body), C.c_void_p(stream or 0)))

    # ---- canvases (ian_sessions_reserve_canvas, ian_canvas_*) ----
    def sessions_reserve_canvas(self, count, max_w=0, max_h=0, feather=0):
        self._check(self.lib.ian_sessions_reserve_canvas(self._h, int(count), int(max_w), int(max_h), int(feather)))

    def sessions_reserve_edges(self, table=None):
        """ian_sessions_reserve_edges; table = 766 float32 range weights (npe_ops.guide_table), or None for the plain compose."""
        if table is None:
            self._check(self.lib.ian_sessions_reserve_edges(self._h, C.c_void_p(0), 0))
            return
        t = np.ascontiguousarray(table, np.float32)
        if t.ndim != 1:
            raise ValueError("the guide table is one-dimensional, got shape %s" % (t.shape,))
        self._check(self.lib.ian_sessions_reserve_edges(self._h, _ptr(t), t.shape[0]))

    def sessions_edges(self):
        """ian_sessions_edges -> the float32[766] table of the edge-aware compose, or None without one."""
        t = np.empty(766, np.float32)
        rc = self.lib.ian_sessions_edges(self._h, _ptr(t))
        if rc < 0:
            self._check(rc)
        return t if rc == 1 else None

    def canvas_put(self, canvas, pixels, stream=None):
        """ian_canvas_put; pixels u8[3,hgt,w], a contiguous numpy array or a device tensor."""
        hgt, w = int(pixels.shape[1]), int(pixels.shape[2])
        self._check(self.lib.ian_canvas_put(self._h, int(canvas), w, hgt, _ptr(pixels), C.c_void_p(stream or 0)))

    def canvas_place(self, items, shown=None, stream=None):
        """ian_canvas_place; items = a ctypes array of CanvasPlacement (n = its length), shown u8[n,3,64,64] or None."""
        self._check(self.lib.ian_canvas_place(self._h, len(items), items, _ptr(shown) if shown is not None else C.c_void_p(0),
                                              C.c_void_p(stream or 0)))

    def canvas_compose(self, windows, vw, vh, out, stream=None):
        """ian_canvas_compose; windows = a ctypes array of CanvasWindow (n = its length), out u8[n,3,vh,vw]."""
        self._check(self.lib.ian_canvas_compose(self._h, len(windows), windows, int(vw), int(vh), _ptr(out), C.c_void_p(stream or 0)))

    def canvas_brush(self, events, windows, vw, vh, out, shown=None, stream=None):
        """ian_canvas_brush; events = a ctypes array of SessionEvent, windows = one of CanvasWindow (m = its length), out u8[m,3,vh,vw]."""
        self._check(self.lib.ian_canvas_brush(self._h, len(events), events, _ptr(shown) if shown is not None else C.c_void_p(0),
                                              len(windows), windows, int(vw), int(vh), _ptr(out), C.c_void_p(stream or 0)))

    def canvas_brush_tip(self, events, tips, windows, vw, vh, out, shown=None, stream=None):
        """ian_compose_brush_soft; the arguments of canvas_brush and tips = int32[n], one per event (-1: no tip)."""
        tips = np.ascontiguousarray(tips, np.int32)
        if tips.shape != (len(events),):
            raise ValueError("tips must hold one index per event (%d), got shape %s" % (len(events), tips.shape))
        self._check(self.lib.ian_compose_brush_soft(self._h, len(events), events, _ptr(tips), _ptr(shown) if shown is not None else C.c_void_p(0),
                                                  len(windows), windows, int(vw), int(vh), _ptr(out), C.c_void_p(stream or 0)))

    def compose_zoom(self, windows, vw, vh, zoom, out, stream=None):
        """ian_compose_zoom: canvas_compose at 1/zoom; vw, vh = the output size, out u8[n,3,vh,vw]."""
        self._check(self.lib.ian_compose_zoom(self._h, len(windows), windows, int(vw), int(vh), int(zoom), _ptr(out), C.c_void_p(stream or 0)))

    def compose_brush_zoom(self, events, windows, vw, vh, zoom, out, shown=None, stream=None):
        """ian_compose_brush_zoom: canvas_brush with the windows at 1/zoom."""
        self._check(self.lib.ian_compose_brush_zoom(self._h, len(events), events, _ptr(shown) if shown is not None else C.c_void_p(0),
                                                    len(windows), windows, int(vw), int(vh), int(zoom), _ptr(out), C.c_void_p(stream or 0)))

    def canvas_commit(self, canvas, shown=None, stream=None):
        """ian_canvas_commit; shown u8[k,3,64,64] for the k sessions placed on the canvas, or None."""
        self._check(self.lib.ian_canvas_commit(self._h, int(canvas), _ptr(shown) if shown is not None else C.c_void_p(0),
                                               C.c_void_p(stream or 0)))

    def canvas_read(self, canvas, stream=None):
        """ian_canvas_read -> the stored picture of one canvas, u8 (3,hgt,w): two calls, the size first."""
        wh = np.zeros(2, np.int32)
        self._check(self.lib.ian_canvas_read(self._h, int(canvas), C.c_void_p(0), _ptr(wh), C.c_void_p(stream or 0)))
        out = np.empty((3, int(wh[1]), int(wh[0])), np.uint8)
        self._check(self.lib.ian_canvas_read(self._h, int(canvas), _ptr(out), _ptr(wh), C.c_void_p(stream or 0)))
        return out

    def canvas_placements(self, canvas):
        """ian_canvas_placements -> [(session, x, y, scale)] of one canvas in ascending session id; host only."""
        out = (CanvasPlacement * CANVAS_MAX_PLACED)()
        count = np.zeros(1, np.int32)
        self._check(self.lib.ian_canvas_placements(self._h, int(canvas), out, _ptr(count)))
        return [(p.session, p.x, p.y, p.scale) for p in out[:int(count[0])]]

    def place_oriented(self, items, shown=None, stream=None):
        """ian_place_oriented; items = a ctypes array of CanvasOriented (n = its length), shown u8[n,3,64,64] or None."""
        self._check(self.lib.ian_place_oriented(self._h, len(items), items, _ptr(shown) if shown is not None else C.c_void_p(0),
                                                C.c_void_p(stream or 0)))

    def placements_oriented(self, canvas):
        """ian_placements_oriented -> [(session, cx2, cy2, ax, ay)] of one canvas in ascending session id; host only."""
        out = (CanvasOriented * CANVAS_MAX_PLACED)()
        count = np.zeros(1, np.int32)
        self._check(self.lib.ian_placements_oriented(self._h, int(canvas), out, _ptr(count)))
        return [(p.session, p.cx2, p.cy2, p.ax, p.ay) for p in out[:int(count[0])]]

    def session_read(self, sid, what, stream=None, scale=0):
        code, dtype, shape = SESSION_FIELDS[what]
        if shape == "S":
            if not 1 <= int(scale) <= 16:       # the library writes 3 * S * S bytes: never into a buffer sized from a wrong scale
                raise ValueError("reading %s needs the pool's scale (1..16), got %r" % (what, scale))
            shape = (3, 64 * int(scale), 64 * int(scale))
        out = np.empty(shape if shape is not None else (self.lowered.num_latents,), dtype)
        self._check(self.lib.ian_session_read(self._h, int(sid), code, _ptr(out), C.c_void_p(stream or 0)))
        return out

    def read_slot(self, slot, n):
        h, w, c = self.lowered.slots[slot]
        out = np.empty((n, c, h, w), np.float32)
        self._check(self.lib.ian_read_slot(self._h, slot, n, _ptr(out), C.c_void_p(0)))
        return out

    def read_slot_grad(self, slot, n=1):
        h, w, c = self.lowered.slots[slot]
        out = np.empty((n, c, h, w), np.float32)
        self._check(self.lib.ian_read_slot_grad(self._h, slot, n, _ptr(out), C.c_void_p(0)))
        return out

    def profile_enable(self, on=True):
        self._check(self.lib.ian_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, n, fl, tot = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        self._check(self.lib.ian_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(fl), C.byref(tot)))
        return {"tapgemm_ms": ms.value, "tapgemm_launches": n.value, "tapgemm_flops": fl.value, "total_ms": tot.value}

    def autotune(self, n, what=1, stream=None):
        self._check(self.lib.ian_autotune(self._h, int(n), int(what), C.c_void_p(stream or 0)))

    def set_option(self, key, value):
        self._check(self.lib.ian_set_option(self._h, key.encode(), int(value)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.ian_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- include/ian_train.h: layer objects + element-wise ops of the training step -------------------------------------
_TRAIN_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ian_train.h")
_train_ready = False


def parse_header_prototypes(path):
    """[(return type, name, [argument C types])] of every function declared in a C header (plain C, one per ';')."""
    import re
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#.*", " ", text)
    out = []
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(ian_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "typedef" in ret:
            continue
        argt = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                argt.append("ptr" if "*" in a or "[" in a else a.rsplit(" ", 1)[0].replace("const ", "").strip())
        out.append((ret, name, argt))
    return out


_CT = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "int": C.c_int, "ptr": C.c_void_p}


def load_train_library():
    """libian.so with argtypes/restype of every include/ian_train.h entry point set from the header itself."""
    global _train_ready
    lib = load_library()
    if not _train_ready:
        for ret, name, argt in parse_header_prototypes(_TRAIN_HEADER):
            fn = getattr(lib, name)
            fn.argtypes = [_CT[t] for t in argt]
            fn.restype = C.c_char_p if "char" in ret else (None if ret == "void" else (C.c_int64 if "int64" in ret else C.c_int32))
        _train_ready = True
    return lib


def train_exports():
    return [name for _, name, _ in parse_header_prototypes(_TRAIN_HEADER)]
