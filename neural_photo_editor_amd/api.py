"""Plat-style model facade: the drop-in for the reference's API.py.

``IAN(config_path, dnn)`` keeps API.py's surface (API.py:11-110) so that NPE.py's call sequence
(NPE.py:18,110,205,218,257,261,296,311,323,333,335) runs unchanged:

    model = IAN(config_path='IAN_simple.py', dnn=True)
    z  = model.encode_images(x)            # f32[n,3,64,64] in [-1,1] -> f32[n,100]
    x_ = model.sample_at(z)                # f32[n,100] -> f32[n,3,64,64]
    g  = model.imgradRGB(c1,r1,c2,r2,RGB,z); g2 = model.imgrad(c1,r1,c2,r2,z)
    model.get_zdim(); model.cfg; model.model

Everything numerical happens in libian.so (hand-written HIP, include/ian.h); this class only reads
the config, loads the checkpoint and moves numpy buffers across the C ABI.  Extra methods give the
four function equivalents sample_IAN.py compiles for itself (sample_IAN.py:86-94).
"""
from __future__ import annotations

import logging
import os
import warnings

import numpy as np

from . import checkpoints, config_loader, lowering, made
from .lib import CLONE_MAX_STEPS, SESSION_FIELDS, STROKE_MAX_POINTS, BrushItem, Handle, SessionCloneEvent, SessionEvent, SessionFitItem
from .lib import SessionStroke, SessionView, StrokeBox

BATCH_MAX = 256     # ian_grad_batch / ian_brush_step_batch: 1 <= n <= 256


def per_item(v, what, n, top=None):
    """One value for all n items, or one per item -> n values: floats, or (top given) integers or booleans in 0..top as int32."""
    if top is None:
        a = np.asarray(v, np.float64)
        if a.ndim == 0:
            return [float(a)] * n
        if a.shape != (n,):
            raise ValueError("%s must be a scalar or have shape (%d,), got %s" % (what, n, a.shape))
        return [float(t) for t in a]
    a = np.asarray(v)
    if a.ndim == 0:
        a = np.tile(a, n)
    if a.shape != (n,) or not (np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
        raise ValueError("%s must be one value or %d values of an integer or boolean type, got %s %s" % (what, n, a.dtype, a.shape))
    for i, t in enumerate(int(t) for t in a):
        if not 0 <= t <= top:
            raise ValueError("item %d: %s %d outside 0..%d" % (i, what, t, top))
    return a.astype(np.int32)


def pack_brush_items(boxes, n_rgb=None, modes=None, weight=0.0, sign=1.0):
    """Python arguments of the batched brush calls -> a ctypes array of ian_brush_item (include/ian.h), validated before the
    library sees anything.  boxes (n,4) as (c1, r1, c2, r2) -- floats from Tk are truncated as imgrad's int() does; n_rgb = the
    leading size of the RGB batch, or None when no RGB was given; modes default to 1 with RGB and 0 without; weight and sign are
    scalars or length-n arrays: coef = float32(sign*weight) and gscale = float32(1 + (c2 - c1)), exactly as brush_step forms them."""
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError("boxes must have shape (n,4) as (c1,r1,c2,r2), got %s" % (b.shape,))
    n = b.shape[0]
    if not 1 <= n <= BATCH_MAX:
        raise ValueError("a batch holds 1..%d brush events, got %d" % (BATCH_MAX, n))
    if n_rgb is not None and n_rgb != n:
        raise ValueError("RGB holds %d images for %d boxes" % (n_rgb, n))
    if modes is None:
        m = [1 if n_rgb is not None else 0] * n
    else:
        m = [int(v) for v in np.asarray(modes).reshape(-1)]
        if len(m) != n:
            raise ValueError("modes must have length %d, got %d" % (n, len(m)))
        if any(v not in (0, 1) for v in m):
            raise ValueError("modes must be 0 (imgrad) or 1 (imgradRGB)")
        if n_rgb is None and any(m):
            raise ValueError("item %d has mode 1 (imgradRGB) but no RGB was given" % m.index(1))
    w, sg = per_item(weight, "weight", n), per_item(sign, "sign", n)
    items = (BrushItem * n)()
    for i in range(n):
        c1, r1, c2, r2 = [int(v) for v in b[i]]
        it = items[i]
        it.c1, it.r1, it.c2, it.r2, it.mode = c1, r1, c2, r2, m[i]
        it.coef = sg[i] * w[i]                 # rounded to float32 by ctypes, as numpy rounds the scalar
        it.gscale = float(1 + (c2 - c1))
    return items


def brush_colour(levels):
    """Brush colour levels (0..255 per channel, NPE.py:87,359 myRGB) -> the tanh-space float32 triple of ian_session_event:
    np.float32(to_tanh(np.float32(level))), exactly what npe_ops.paint_event feeds brush_step."""
    from . import npe_ops
    c = np.float32(npe_ops.to_tanh(np.float32(np.asarray(levels))))
    if c.shape != (3,):
        raise ValueError("a brush colour has 3 levels, got shape %s" % (c.shape,))
    return c


def check_session_ids(ids, capacity=None, opened=None, repeats=False, what="sessions"):
    """Session ids of one call -> a contiguous int32 array, or ValueError: 1..256 integers, each inside the pool (when capacity is
    given), opened (when `opened`, a container of opened ids, is given) and, unless `repeats`, named once."""
    a = np.asarray(ids)
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("ids must be a 1-D array of integers, got shape %s dtype %s" % (a.shape, a.dtype))
    if not 1 <= a.shape[0] <= BATCH_MAX:
        raise ValueError("a call holds 1..%d %s, got %d" % (BATCH_MAX, what, a.shape[0]))
    seen = {}
    for i, v in enumerate(int(t) for t in a):
        if v < 0 or (capacity is not None and v >= capacity):
            raise ValueError("item %d: session %d outside the pool%s" % (i, v, "" if capacity is None else " (capacity %d)" % capacity))
        if opened is not None and v not in opened:
            raise ValueError("item %d: session %d has not been opened" % (i, v))
        if v in seen and not repeats:
            raise ValueError("item %d: session %d already appears as item %d of this call" % (i, v, seen[v]))
        seen[v] = i
    return np.ascontiguousarray(a, np.int32)


def _colours_and_modes(colours, modes, n):
    """colours (n,3) or (3,) or None and modes (n,), a scalar or None of n session events or strokes -> (col (n,3) or None, modes as a
    list): every mode is 0 without colours and defaults to 1 with them; mode 1 needs a colour."""
    col = None
    if colours is not None:
        col = np.asarray(colours)
        if col.shape == (3,):
            col = np.tile(col, (n, 1))
        if col.shape != (n, 3):
            raise ValueError("colours must have shape (%d,3) or (3,), got %s" % (n, col.shape))
    if modes is None:
        m = [1 if col is not None else 0] * n
    else:
        ma = np.asarray(modes).reshape(-1)
        m = [int(v) for v in (np.tile(ma, n) if ma.shape == (1,) else ma)]
        if len(m) != n:
            raise ValueError("modes must be a scalar or have length %d, got %d" % (n, len(m)))
        for i, v in enumerate(m):
            if v not in (0, 1):
                raise ValueError("item %d has mode %d (0 = imgrad, 1 = imgradRGB)" % (i, v))
        if col is None and any(m):
            raise ValueError("item %d has mode 1 (imgradRGB) but no colour was given" % m.index(1))
    return col, m


def pack_session_events(ids, boxes, colours=None, modes=None, weight=0.05, sign=-1.0, capacity=None, opened=None):
    """Python arguments of ian_session_brush -> a ctypes array of ian_session_event (include/ian.h), validated before the library
    sees anything.  ids (n,) session ids; boxes (n,4) or (4,) as (c1, r1, c2, r2), floats truncated as imgrad's int() does;
    colours (n,3) or (3,) uint8-range levels, or None (then every mode is 0); modes default to 1 with colours and 0 without;
    weight and sign are scalars or length-n arrays: coef = float32(sign*weight), gscale = float32(1 + (c2 - c1)).
    capacity / opened (a container of opened ids), when given, bound and vet the ids."""
    idl = [int(v) for v in check_session_ids(ids, capacity, opened)]
    n = len(idl)
    b = np.asarray(boxes)
    if b.ndim == 1 and b.shape == (4,):
        b = np.tile(b, (n, 1))
    if b.ndim != 2 or b.shape != (n, 4):
        raise ValueError("boxes must have shape (%d,4) or (4,) as (c1,r1,c2,r2), got %s" % (n, b.shape))
    col, m = _colours_and_modes(colours, modes, n)
    w, sg = per_item(weight, "weight", n), per_item(sign, "sign", n)
    ev = (SessionEvent * n)()
    for i in range(n):
        c1, r1, c2, r2 = [int(v) for v in b[i]]
        if c1 < 0 or r1 < 0 or c2 > 64 or r2 > 64:
            raise ValueError("item %d: patch (%d,%d,%d,%d) outside the 64x64 image" % (i, c1, r1, c2, r2))
        e = ev[i]
        e.session, e.c1, e.r1, e.c2, e.r2, e.mode = idl[i], c1, r1, c2, r2, m[i]
        e.coef = sg[i] * w[i]                  # rounded to float32 by ctypes, as numpy rounds the scalar
        e.gscale = float(1 + (c2 - c1))
        if col is not None:
            e.rgb[0], e.rgb[1], e.rgb[2] = [float(v) for v in brush_colour(col[i])]
    return ev


def pack_session_strokes(ids, paths, colours=None, modes=None, weight=0.05, sign=-1.0, capacity=None, opened=None):
    """Python arguments of ian_session_stroke -> (a ctypes array of ian_session_stroke_item, one of ian_stroke_box, perm), validated
    before the library sees anything.  ids (n,) session ids; paths a sequence of n arrays of shape (K_i, 4), 1 <= K_i <= 64: the
    rectangles (c1, r1, c2, r2) of session i's stroke in the order they are applied, floats truncated as imgrad's int() does;
    colours, modes, weight and sign as in pack_session_events, one value per STROKE: coef = float32(sign*weight) for every point,
    gscale = float32(1 + (c2 - c1)) per rectangle.  The library wants the strokes with non-increasing K: they are sorted stably by
    descending K, the boxes laid out in that order, and perm[j] is the caller's index of sorted stroke j (what the library returns
    for stroke j belongs to ids[perm[j]])."""
    idl = [int(v) for v in check_session_ids(ids, capacity, opened)]
    n = len(idl)
    if isinstance(paths, np.ndarray) and paths.ndim == 3:
        paths = list(paths)
    if len(paths) != n:
        raise ValueError("paths must hold one (K,4) array per session: %d for %d sessions" % (len(paths), n))
    pl = []
    for i, p in enumerate(paths):
        b = np.asarray(p)
        if b.ndim != 2 or b.shape[1] != 4:
            raise ValueError("item %d: a path has shape (K,4) as (c1,r1,c2,r2) per point, got %s" % (i, b.shape))
        if not 1 <= b.shape[0] <= STROKE_MAX_POINTS:
            raise ValueError("item %d: a stroke has 1..%d points, got %d" % (i, STROKE_MAX_POINTS, b.shape[0]))
        rows = [[int(v) for v in r] for r in b]
        for k, (c1, r1, c2, r2) in enumerate(rows):
            if c1 < 0 or r1 < 0 or c2 > 64 or r2 > 64:
                raise ValueError("item %d: point %d: patch (%d,%d,%d,%d) outside the 64x64 image" % (i, k, c1, r1, c2, r2))
        pl.append(rows)
    col, m = _colours_and_modes(colours, modes, n)
    w, sg = per_item(weight, "weight", n), per_item(sign, "sign", n)
    perm = sorted(range(n), key=lambda i: -len(pl[i]))      # stable: equal lengths keep the caller's order
    strokes = (SessionStroke * n)()
    boxes = (StrokeBox * sum(len(p) for p in pl))()
    first = 0
    for j, i in enumerate(perm):
        s = strokes[j]
        s.session, s.first, s.count, s.mode = idl[i], first, len(pl[i]), m[i]
        s.coef = sg[i] * w[i]                  # rounded to float32 by ctypes, as numpy rounds the scalar
        if col is not None:
            s.rgb[0], s.rgb[1], s.rgb[2] = [float(v) for v in brush_colour(col[i])]
        for k, (c1, r1, c2, r2) in enumerate(pl[i]):
            b = boxes[first + k]
            b.c1, b.r1, b.c2, b.r2 = c1, r1, c2, r2
            b.gscale = float(1 + (c2 - c1))
        first += len(pl[i])
    return strokes, boxes, perm


def pack_session_tips(tips, boxes, tip_sizes, count=None):
    """The tips argument of ian_session_brush_tip / ian_session_path_tip -> int32 (n,), refusing on the host what the library would
    refuse, naming the item.  tips: one integer for all n items or one per item, -1 = no tip; boxes: per item an array (K,4) (or (4,))
    of the rectangles (c1, r1, c2, r2) it is applied to, n = len(boxes); tip_sizes: {tip: (tw, th)} of the tips that were set; count:
    the reservation (None: not checked)."""
    n = len(boxes)
    a = np.asarray(tips)
    if a.ndim == 0:
        a = np.tile(a, n)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("tips must be one integer or %d integers, got %s %s" % (n, a.dtype, a.shape))
    for i, t in enumerate(int(t) for t in a):
        if t == -1:
            continue
        if t < -1 or (count is not None and t >= count):
            raise ValueError("item %d: tip %d outside -1..%s" % (i, t, "count-1" if count is None else count - 1))
        if t not in tip_sizes:
            raise ValueError("item %d: tip %d has never been set (set_tip)" % (i, t))
        tw, th = tip_sizes[t]
        for k, (c1, r1, c2, r2) in enumerate([int(v) for v in r] for r in np.asarray(boxes[i]).reshape(-1, 4)):
            if c2 - c1 != tw or r2 - r1 != th:
                raise ValueError("item %d: point %d: patch (%d,%d,%d,%d) is not the %d x %d of tip %d" % (i, k, c1, r1, c2, r2, tw, th, t))
    return np.ascontiguousarray(a, np.int32)


CLONE_FIELDS = ("GIM", "IM", "RECON")       # what a clone event may read of its source


def check_clone_steps(steps):
    """steps of ian_session_clone -> int, refused with the library's wording."""
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= CLONE_MAX_STEPS:
        raise ValueError("steps = %r outside 1..%d" % (steps, CLONE_MAX_STEPS))
    return int(steps)


def pack_session_clones(ids, boxes, sources, offsets=(0, 0), field="GIM", weight=0.05, sign=-1.0, capacity=None, opened=None):
    """Python arguments of ian_session_clone -> a ctypes array of ian_session_clone_event (include/ian.h), validated with the library's
    own rules and wording before the library sees anything.  ids (n,) destination session ids, each once; boxes (n,4) or (4,) as
    (c1, r1, c2, r2) on the destination, floats truncated as imgrad's int() does; sources (n,) or one id: the sessions the targets are
    read from (a source may equal its destination, and serve several items); offsets (n,2) or (2,) as (dc, dr): the target of
    destination pixel (r, c) is source pixel (r + dr, c + dc); field "GIM", "IM" or "RECON", one for all or one per item; weight and
    sign scalars or length-n arrays: coef = float32(sign*weight), gscale = float32(1 + (c2 - c1)) (NPE.py:206).
    capacity / opened (a container of opened ids), when given, bound and vet destinations and sources alike."""
    idl = [int(v) for v in check_session_ids(ids, capacity, opened)]
    n = len(idl)
    b = np.asarray(boxes)
    if b.ndim == 1 and b.shape == (4,):
        b = np.tile(b, (n, 1))
    if b.ndim != 2 or b.shape != (n, 4):
        raise ValueError("boxes must have shape (%d,4) or (4,) as (c1,r1,c2,r2), got %s" % (n, b.shape))
    src = np.asarray(sources)
    if src.ndim == 0:
        src = np.tile(src, n)
    if src.shape != (n,) or not np.issubdtype(src.dtype, np.integer):
        raise ValueError("sources must be one session id or %d of them, got %s %s" % (n, src.dtype, src.shape))
    off = _int_pairs(offsets, n, "offsets")
    fl = [field] * n if isinstance(field, str) else list(field)
    if len(fl) != n:
        raise ValueError("field must be one name or %d of them, got %d" % (n, len(fl)))
    w, sg = per_item(weight, "weight", n), per_item(sign, "sign", n)
    dest = {v: i for i, v in enumerate(idl)}
    ev = (SessionCloneEvent * n)()
    for i in range(n):
        c1, r1, c2, r2 = [int(v) for v in b[i]]
        s, dc, dr = int(src[i]), int(off[i, 0]), int(off[i, 1])
        if c1 < 0 or r1 < 0 or c2 > 64 or r2 > 64:
            raise ValueError("item %d: patch (%d,%d,%d,%d) outside the 64x64 image" % (i, c1, r1, c2, r2))
        if s < 0 or (capacity is not None and s >= capacity):
            raise ValueError("item %d: source session %d outside the pool%s" % (i, s, "" if capacity is None else " (capacity %d)" % capacity))
        if opened is not None and s not in opened:
            raise ValueError("item %d: source session %d has not been opened" % (i, s))
        if fl[i] not in CLONE_FIELDS:
            raise ValueError("item %d: field %r (GIM, IM or RECON of the source)" % (i, fl[i]))
        if c1 < c2 and r1 < r2 and (c1 + dc < 0 or c2 + dc > 64 or r1 + dr < 0 or r2 + dr > 64):
            raise ValueError("item %d: patch (%d,%d,%d,%d) shifted by (%d,%d) leaves the 64x64 image" % (i, c1, r1, c2, r2, dc, dr))
        if fl[i] == "IM" and s in dest:
            raise ValueError("item %d: source session %d is read from IM, which item %d of this call writes" % (i, s, dest[s]))
        e = ev[i]
        e.session, e.c1, e.r1, e.c2, e.r2 = idl[i], c1, r1, c2, r2
        e.source, e.field, e.dc, e.dr = s, SESSION_FIELDS[fl[i]][0], dc, dr
        e.coef = sg[i] * w[i]                  # rounded to float32 by ctypes, as numpy rounds the scalar
        e.gscale = float(1 + (c2 - c1))
    return ev


def check_zoom(zoom):
    """The zoom of a view -> int in 1..16."""
    if isinstance(zoom, (bool, np.bool_)) or not isinstance(zoom, (int, np.integer)) or not 1 <= int(zoom) <= 16:
        raise ValueError("zoom must be an integer in 1..16, got %r" % (zoom,))
    return int(zoom)


def _window_outside(i, x, y, vw, vh, zoom, w, h, what):
    """The refusal of window i whose source (x, y, zoom*vw, zoom*vh) leaves the w x h picture, or None."""
    if x < 0 or y < 0 or x + zoom * vw > w or y + zoom * vh > h:
        at = "" if zoom == 1 else " at zoom %d" % zoom
        return "item %d: window (%d,%d) + %d x %d%s outside the %d x %d %s" % (i, x, y, vw, vh, at, w, h, what)
    return None


def pack_session_views(ids, origins, size, scale, capacity=None, opened=None, sourced=None, events=None, zoom=1):
    """Python arguments of ian_session_render / ian_session_brush_view -> (a ctypes array of ian_session_view, vw, vh), validated
    before the library sees anything.  ids (n,) session ids -- the same id may appear several times, as tiles of one picture;
    origins (n,2) or (2,) as (x, y), the windows' top-left corners in the S x S picture, S = 64 * scale; size = (vw, vh) or one
    integer for a square window.  x and vw must be multiples of 4, the window inside the picture.  zoom (1..16): size is that of the
    view at 1/zoom, and the source window (x, y, zoom*vw, zoom*vh) is the one that must lie inside.  scale is the pool's (None or
    0: there is no full-resolution reservation).  capacity / opened / sourced (containers of opened ids and of ids that hold a
    full-resolution source), when given, bound and vet the ids; events (a ctypes array of ian_session_event), when given, must name
    the same sessions in the same order."""
    if not scale:
        raise ValueError("the pool has no full-resolution reservation (reserve_hires)")
    scale = int(scale)
    if not 1 <= scale <= 16:
        raise ValueError("scale must be in 1..16, got %d" % scale)
    S = 64 * scale
    zoom = check_zoom(zoom)
    a = check_session_ids(ids, capacity, opened, repeats=True, what="views")
    n = a.shape[0]
    sz = np.asarray(size)
    if sz.ndim == 0:
        sz = np.tile(sz, 2)
    if sz.shape != (2,) or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError("size must be (vw, vh) or one integer, got %r" % (size,))
    vw, vh = int(sz[0]), int(sz[1])
    if vw < 1 or vh < 1:
        raise ValueError("window %d x %d: both sizes must be at least 1" % (vw, vh))
    if vw % 4:
        raise ValueError("window width %d is not a multiple of 4" % vw)
    o = np.asarray(origins)
    if o.shape == (2,):
        o = np.tile(o, (n, 1))
    if o.shape != (n, 2) or not np.issubdtype(o.dtype, np.integer):
        raise ValueError("origins must be integers of shape (%d,2) or (2,) as (x, y), got %s %s" % (n, o.dtype, o.shape))
    if events is not None and len(events) != n:
        raise ValueError("%d views for %d events" % (n, len(events)))
    views = (SessionView * n)()
    for i in range(n):
        sid, x, y = int(a[i]), int(o[i, 0]), int(o[i, 1])
        if events is not None and events[i].session != sid:
            raise ValueError("item %d: the view names session %d, the event session %d" % (i, sid, events[i].session))
        if sourced is not None and sid not in sourced:
            raise ValueError("item %d: session %d has no full-resolution source (open_hires)" % (i, sid))
        if x % 4:
            raise ValueError("item %d: window x %d is not a multiple of 4" % (i, x))
        bad = _window_outside(i, x, y, vw, vh, zoom, S, S, "picture")
        if bad:
            raise ValueError(bad)
        v = views[i]
        v.session, v.x, v.y = sid, x, y
    return views, vw, vh


def _int_pairs(v, n, what):
    a = np.asarray(v)
    if a.shape == (2,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 2) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must be integers of shape (%d,2) or (2,) as (x, y), got %s %s" % (what, n, a.dtype, a.shape))
    return a


def _canvas_ids(cids, n, sizes):
    """One canvas id for all n items or one per item -> n ints, each a canvas of the reservation that holds a picture.
    sizes = {canvas id: (w, h)} of the canvases that were put, or a list with None for those that were not."""
    a = np.asarray(cids)
    if a.ndim == 0:
        a = np.tile(a, n)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("canvas ids must be one integer or %d integers, got %s %s" % (n, a.dtype, a.shape))
    out = [int(v) for v in a]
    for i, c in enumerate(out):
        if not 0 <= c < len(sizes):
            raise ValueError("item %d: canvas %d outside 0..%d" % (i, c, len(sizes) - 1))
        if sizes[c] is None:
            raise ValueError("item %d: canvas %d holds no picture (canvas_put)" % (i, c))
    return out


def pack_canvas_placements(ids, cids, origins, scales, sizes, placed=None, capacity=None):
    """Python arguments of ian_canvas_place -> a ctypes array of ian_canvas_placement (include/ian.h), validated before the library
    sees anything.  ids (n,) session ids, each once; cids one canvas id or (n,); origins (n,2) or (2,) as (x, y), the squares'
    top-left corners at any alignment; scales one integer or (n,), 1..16: a square is 64 * scale pixels a side and must lie inside
    its canvas.  sizes = per canvas (w, h) or None for a canvas that holds no picture; placed = {session id: canvas id} as it is now
    (a session already placed moves), from which the ninth session on one canvas is refused; capacity bounds the ids."""
    from .lib import CANVAS_MAX_PLACED, CanvasPlacement
    idv = check_session_ids(ids, capacity)
    n = len(idv)
    cv = _canvas_ids(cids, n, sizes)
    o = _int_pairs(origins, n, "origins")
    sc = np.asarray(scales)
    if sc.ndim == 0:
        sc = np.tile(sc, n)
    if sc.shape != (n,) or not np.issubdtype(sc.dtype, np.integer):
        raise ValueError("scales must be one integer or %d integers, got %s %s" % (n, sc.dtype, sc.shape))
    after = dict(placed or {})
    items = (CanvasPlacement * n)()
    for i in range(n):
        sid, c, x, y, s = int(idv[i]), cv[i], int(o[i, 0]), int(o[i, 1]), int(sc[i])
        if not 1 <= s <= 16:
            raise ValueError("item %d: scale %d outside 1..16" % (i, s))
        w, h = sizes[c]
        if x < 0 or y < 0 or x + 64 * s > w or y + 64 * s > h:
            raise ValueError("item %d: square (%d,%d) + %d outside the %d x %d canvas" % (i, x, y, 64 * s, w, h))
        after.pop(sid, None)                   # a session that moves leaves its square first
        p = items[i]
        p.session, p.canvas, p.x, p.y, p.scale = sid, c, x, y, s
    for i in range(n):
        after[int(idv[i])] = cv[i]
        if sum(1 for c in after.values() if c == cv[i]) > CANVAS_MAX_PLACED:
            raise ValueError("item %d: canvas %d already holds %d sessions" % (i, cv[i], CANVAS_MAX_PLACED))
    return items


def pack_canvas_oriented(ids, cids, items, sizes, placed=None, capacity=None):
    """Python arguments of ian_place_oriented -> a ctypes array of ian_canvas_oriented (include/ian.h), validated before the library
    sees anything.  ids (n,) session ids, each once; cids one canvas id or (n,); items (n,4) or (4,) integers (cx2, cy2, ax, ay):
    the square's centre in half pixels and the canvas displacement per field pixel in Q16 (npe_ops.oriented_placement), with
    ax*ax + ay*ay in 2^32..2^40 and every gather sample on the canvas.  sizes, placed and capacity as in pack_canvas_placements."""
    from . import npe_ops
    from .lib import CANVAS_MAX_PLACED, CanvasOriented
    idv = check_session_ids(ids, capacity)
    n = len(idv)
    cv = _canvas_ids(cids, n, sizes)
    a = np.asarray(items)
    if a.shape == (4,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 4) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("items must be integers of shape (%d,4) or (4,) as (cx2, cy2, ax, ay), got %s %s" % (n, a.dtype, a.shape))
    after = dict(placed or {})
    out = (CanvasOriented * n)()
    for i in range(n):
        sid, c = int(idv[i]), cv[i]
        cx2, cy2, ax, ay = (int(v) for v in a[i])
        if max(abs(cx2), abs(cy2), abs(ax), abs(ay)) >= 2 ** 31:
            raise ValueError("item %d: (%d,%d,%d,%d) are not int32" % (i, cx2, cy2, ax, ay))
        if not npe_ops.ORIENTED_L2_MIN <= ax * ax + ay * ay <= npe_ops.ORIENTED_L2_MAX:
            raise ValueError("item %d: ax*ax + ay*ay of (%d,%d) outside 2^32..2^40 (a side of 64..1024 pixels)" % (i, ax, ay))
        w, h = sizes[c]
        if not npe_ops.oriented_inside(w, h, cx2, cy2, ax, ay):
            raise ValueError("item %d: square (%d,%d,%d,%d) samples outside the %d x %d canvas" % (i, cx2, cy2, ax, ay, w, h))
        after.pop(sid, None)                   # a session that moves leaves its square first
        p = out[i]
        p.session, p.canvas, p.cx2, p.cy2, p.ax, p.ay = sid, c, cx2, cy2, ax, ay
    for i in range(n):
        after[int(idv[i])] = cv[i]
        if sum(1 for c in after.values() if c == cv[i]) > CANVAS_MAX_PLACED:
            raise ValueError("item %d: canvas %d already holds %d sessions" % (i, cv[i], CANVAS_MAX_PLACED))
    return out


def pack_canvas_windows(cids, origins, size, sizes, zoom=1):
    """Python arguments of ian_canvas_compose / ian_canvas_brush -> (a ctypes array of ian_canvas_window, vw, vh), validated before
    the library sees anything.  cids (n,) canvas ids -- the same canvas may appear several times, as tiles; origins (n,2) or (2,)
    as (x, y); size = (vw, vh) or one integer.  x and vw must be multiples of 4, the window inside the canvas's picture.  zoom as in
    pack_session_views.  sizes as in pack_canvas_placements."""
    from .lib import CanvasWindow
    zoom = check_zoom(zoom)
    a = np.asarray(cids)
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim != 1 or not 1 <= a.shape[0] <= BATCH_MAX:
        raise ValueError("a call holds 1..%d windows, got shape %s" % (BATCH_MAX, a.shape))
    n = a.shape[0]
    cv = _canvas_ids(a, n, sizes)
    sz = np.asarray(size)
    if sz.ndim == 0:
        sz = np.tile(sz, 2)
    if sz.shape != (2,) or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError("size must be (vw, vh) or one integer, got %r" % (size,))
    vw, vh = int(sz[0]), int(sz[1])
    if vw < 1 or vh < 1:
        raise ValueError("window %d x %d: both sizes must be at least 1" % (vw, vh))
    if vw % 4:
        raise ValueError("window width %d is not a multiple of 4" % vw)
    o = _int_pairs(origins, n, "origins")
    win = (CanvasWindow * n)()
    for i in range(n):
        x, y = int(o[i, 0]), int(o[i, 1])
        w, h = sizes[cv[i]]
        if x % 4:
            raise ValueError("item %d: window x %d is not a multiple of 4" % (i, x))
        bad = _window_outside(i, x, y, vw, vh, zoom, w, h, "canvas")
        if bad:
            raise ValueError(bad)
        win[i].canvas, win[i].x, win[i].y = cv[i], x, y
    return win, vw, vh


def pack_session_local(ids, local=True, dampen=False, flags=None, capacity=None, opened=None):
    """Python arguments of ian_session_local -> (ids int32 (n,), flags int32 (n,)), validated before the library sees anything.
    local and dampen are booleans, one for all or one per session: flags = local + 2 * dampen.  flags, when given, replaces both: a
    scalar or (n,) integers in 0..3 (bit 0 local, bit 1 dampen).  capacity / opened (a container of opened ids), when given, bound and
    vet the ids."""
    idv = check_session_ids(ids, capacity, opened)
    n = len(idv)
    if flags is not None:
        f = per_item(flags, "flags", n, 3)
    else:
        f = per_item(local, "local", n, 1) + 2 * per_item(dampen, "dampen", n, 1)
    return idv, np.ascontiguousarray(f, np.int32)


def pack_session_undo(ids, steps=1, capacity=None, opened=None):
    """Python arguments of ian_session_undo -> (ids int32 (n,), steps int32 (n,)), validated before the library sees anything.
    steps is one integer for all or one per session: > 0 undoes that many marks, < 0 redoes as many; 0, a non-integer and more than
    the largest depth (64) either way are refused.  Whether a session HAS that many steps only the library knows.  capacity / opened
    (a container of opened ids), when given, bound and vet the ids."""
    idv = check_session_ids(ids, capacity, opened)
    n = len(idv)
    a = np.asarray(steps)
    if a.ndim == 0:
        a = np.tile(a, n)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("steps must be one integer or %d integers, got %s %s" % (n, a.dtype, a.shape))
    for i, t in enumerate(int(t) for t in a):
        if t == 0 or not -64 <= t <= 64:
            raise ValueError("item %d: steps %d (1..64 undoes, -1..-64 redoes)" % (i, t))
    return idv, np.ascontiguousarray(a, np.int32)


FIT_MAX_STEPS = 512     # ian_session_fit: 1 <= steps <= 512


def pack_session_fit(ids, steps=20, lr=0.02, boxes=None, capacity=None, opened=None):
    """Python arguments of ian_session_fit -> (a ctypes array of ian_session_fit_item, steps, lr), validated with the library's own
    rules before the library sees anything.  ids (n,) session ids, each once; boxes (n,4) or (4,) as (c1, r1, c2, r2), floats
    truncated as imgrad's int() does, None = the whole picture; steps an integer in 1..512; lr finite and > 0 as a float32."""
    idl = [int(v) for v in check_session_ids(ids, capacity, opened)]
    n = len(idl)
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= FIT_MAX_STEPS:
        raise ValueError("steps must be an integer in 1..%d, got %r" % (FIT_MAX_STEPS, steps))
    lr32 = float(np.float32(lr))
    if not (np.isfinite(lr32) and lr32 > 0.0):
        raise ValueError("lr must be finite and positive as a float32, got %r" % (lr,))
    b = np.asarray((0, 0, 64, 64) if boxes is None else boxes)
    if b.ndim == 1 and b.shape == (4,):
        b = np.tile(b, (n, 1))
    if b.ndim != 2 or b.shape != (n, 4):
        raise ValueError("boxes must have shape (%d,4) or (4,) as (c1,r1,c2,r2), got %s" % (n, b.shape))
    items = (SessionFitItem * n)()
    for i in range(n):
        c1, r1, c2, r2 = [int(v) for v in b[i]]
        if c1 < 0 or r1 < 0 or c2 > 64 or r2 > 64:
            raise ValueError("item %d: rectangle (%d,%d,%d,%d) outside the 64x64 image" % (i, c1, r1, c2, r2))
        it = items[i]
        it.session, it.c1, it.r1, it.c2, it.r2 = idl[i], c1, r1, c2, r2
    return items, int(steps), lr32


class SessionRecords:
    """n saved sessions (EditSessions.save): `meta`, a structured array of n ian_session_meta entries (npe_ops.SESSION_META_DTYPE),
    and `body`, uint8 (n, body_bytes) -- a numpy array, or a torch device tensor when the save was asked for device memory.
    tobytes / frombytes are what a project file on disk is: a 16-byte header ("IANR", format, n, body_bytes), the metas,
    the bodies."""
    FILE_MAGIC = b"IANR"

    def __init__(self, meta, body):
        from . import npe_ops
        meta = np.asarray(meta)
        if meta.dtype != npe_ops.SESSION_META_DTYPE or meta.ndim != 1:
            raise ValueError("meta must be a 1-D array of npe_ops.SESSION_META_DTYPE, got %s %s" % (meta.dtype, meta.shape))
        self.meta = np.ascontiguousarray(meta)
        self.body = body if hasattr(body, "data_ptr") else np.ascontiguousarray(body, np.uint8)
        if len(self.body.shape) != 2 or self.body.shape[0] != len(self.meta):
            raise ValueError("body must have shape (%d, body_bytes), got %s" % (len(self.meta), tuple(self.body.shape)))

    def __len__(self):
        return len(self.meta)

    @property
    def on_device(self):
        return hasattr(self.body, "data_ptr")

    def host(self):
        """-> the same records with the body in host memory."""
        return SessionRecords(self.meta, self.body.cpu().numpy()) if self.on_device else self

    def __getitem__(self, i):
        """A single record or a slice of them, as SessionRecords."""
        if isinstance(i, (int, np.integer)):
            k = range(len(self))[i]
            i = slice(k, k + 1)
        return SessionRecords(self.meta[i], self.body[i])

    def tobytes(self):
        h = self.host()
        bb = int(h.body.shape[1])
        head = self.FILE_MAGIC + np.array([1, len(h), bb], "<i4").tobytes()
        return head + h.meta.tobytes() + h.body.tobytes()

    @classmethod
    def frombytes(cls, data):
        from . import npe_ops
        data = bytes(data)
        if len(data) < 16 or data[:4] != cls.FILE_MAGIC:
            raise ValueError("not a session record file")
        fmt, n, bb = (int(v) for v in np.frombuffer(data, "<i4", 3, 4))
        if fmt != 1 or n < 0 or bb < 0 or bb % 16 or len(data) != 16 + n * (64 + bb):
            raise ValueError("a session record file of format %d with %d records of %d bytes cannot be %d bytes long" % (fmt, n, bb, len(data)))
        meta = np.frombuffer(data, npe_ops.SESSION_META_DTYPE, n, 16).copy()
        body = np.empty((n, bb), np.uint8)                                # a fresh array: 16-byte aligned, writable
        body[...] = np.frombuffer(data, np.uint8, n * bb, 16 + 64 * n).reshape(n, bb)
        return cls(meta, body)


def pack_session_records(ids, records, zl, scale=0, local=False, depth=0, capacity=None):
    """Python arguments of ian_session_load -> (ids int32 (n,), meta (n,), body (n, body_bytes)), validated before the library sees
    anything: the ids (the targets need not be opened), one record per id, a body of the layout's size, and every meta against the
    layout (zl, scale, local, depth) of the pool: npe_ops.check_session_meta.  A host body comes back 16-byte aligned."""
    from . import npe_ops
    idv = check_session_ids(ids, capacity, None)
    if not isinstance(records, SessionRecords):
        raise ValueError("records must be SessionRecords, got %s" % type(records).__name__)
    n = len(idv)
    if len(records) != n:
        raise ValueError("%d records for %d sessions" % (len(records), n))
    bb = npe_ops.session_record_layout(zl, scale, local, depth)[1]
    if tuple(records.body.shape) != (n, bb):
        raise ValueError("body must have shape (%d,%d) for this pool, got %s" % (n, bb, tuple(records.body.shape)))
    for i in range(n):
        bad = npe_ops.check_session_meta(records.meta[i], zl, scale, local, depth)
        if bad:
            raise ValueError("item %d: the record's %s = %d does not fit this pool (num_latents %d, scale %d, local %d, depth %d, body_bytes %d)"
                             % (i, bad, int(np.asarray(records.meta[i][bad]).reshape(-1)[0]), zl, scale, int(bool(local)), depth, bb))
    body = records.body
    if not records.on_device:
        if body.dtype != np.uint8:
            raise ValueError("body must be uint8, got %s" % body.dtype)
        if not body.flags.c_contiguous or body.ctypes.data % 16:
            body = _aligned_bytes(body)
    elif not body.is_contiguous() or body.data_ptr() % 16:
        raise ValueError("a device body must be contiguous and 16-byte aligned")
    return idv, records.meta, body


def _aligned_bytes(a):
    """A C-contiguous uint8 copy of `a` whose first byte sits at a multiple of 16."""
    raw = np.empty(a.size + 16, np.uint8)
    off = -raw.ctypes.data % 16
    out = raw[off:off + a.size].reshape(a.shape)
    out[...] = a
    return out


class EditSessions:
    """Device-resident edit sessions of one model (ian_session_*, include/ian.h): the state NPE.py keeps in host globals per
    editor (GIM, IM, RECON, ERROR, Z, SAMPLE_FLAG) lives in device memory under a caller-chosen id in 0..capacity-1.  A call takes
    up to 256 sessions in one submission and returns what the canvases show: uint8 (n,3,64,64).
        open    infer (NPE.py:239-274)          reset   Reset (:330-340)           commit  UpdateGIM (:342-345)
        sample  sample (:317-327), z from the caller                                set_latent  paint_latents (:286-302)
        paint   NPE.paint (:192-235)            scroll  NPE.scroll (:305-316)      brush   the general form of both
        stroke / paint_stroke  a whole drag per session (K rectangles along the mouse track) in one submission -> the picture at its end
        clone / restore  paint towards a rectangle of another session's picture, or back towards the session's own photo, several steps
    Photos larger than 64x64 (no counterpart in NPE.py): reserve_hires(scale) keeps every session's photo at 64*scale pixels a side;
        open_hires  infer from the full-size photo     render  windows of the edited picture at full size
        brush_view / paint(view=) / scroll(view=)      the event and its window in one submission
        reserve_guide(sigma) / guide()                 edge-aware render: the edit stops at the photo's edges (joint bilateral upsampling)
    Local edits (NPE.py's unimplemented USER_MASK, gk and dampen): reserve_local() keeps a user mask per session;
        set_local(ids, local, dampen)  from then on a paint on those sessions changes the photo only around the strokes made since
    Undo (no counterpart in NPE.py): reserve_history(depth) keeps a ring of saved latents (and user masks) per session on the device;
        mark(ids)  a stroke begins     undo(ids, steps) / redo(ids, steps)  back and forth -> shown     history(sid)  what is possible
    A closer reconstruction (the encoder + optimisation hybrid the NPE paper compares itself to): fit(ids, steps, lr) runs Adam steps
        on the device from the sessions' current latents towards their own photos -> (RECON, loss trace); every later edit blends
        against a smaller ERROR
    Leaving the pool (no counterpart in NPE.py): save(ids) -> SessionRecords, everything above as bytes; load(ids, records) puts them
        into any ids of a pool of the same layout: a project file, a move to another handle, parking an idle editor
    Whole photos (no counterpart in NPE.py): reserve_canvases(count, max_w, max_h, feather) keeps photos of any size (canvases) in
    device memory beside a full-resolution pool; canvas_put(cid, photo) loads one.
        place(ids, cids, origins, scales)  each session opens on the box mean of a square of its canvas, 64*scale pixels a side
        compose(cids, origins, size)       windows of the photos with every placed session's edit on top, feathered at the squares' rims
        brush_compose(..., windows=)       the event and the windows in one submission -> (shown, out)
        canvas_commit(cid)                 the composed photo becomes the canvas, its sessions start again from it -> shown
        canvas_read(cid) / placements(cid) the stored photo / [(session, x, y, scale)]
        place_oriented(ids, cids, centres, sides, angles)   the same for squares of any side (64..1024) and tilt; place_oriented_raw
                                           takes the integers (cx2, cy2, ax, ay); placements_oriented(cid) lists them.  A canvas holds one form
        reserve_canvas_guide(sigma) / canvas_guide()   edge-aware compose: every placed session's edit stops at the photo's edges
    open, open_hires and load un-place a session; commit on a placed session is refused (canvas_commit is its form).
    Brush tips (no counterpart in NPE.py, whose brush is a square): reserve_tips(count) keeps weight images of up to 64x64 per handle;
        set_tip(tip, weights) / tip(tip)   e.g. npe_ops.round_tip(diameter, hardness): a round brush with a soft edge
        brush / brush_view / paint / scroll / stroke (tips=) and paint_stroke(tip=)   the event's loss weighted by the tip"""

    def __init__(self, handle, capacity, zdim, sigma=0.7):
        from . import npe_ops
        self._h = handle
        self._zdim = zdim
        self.capacity = 0
        self.scale = 0                  # full-resolution reservation: photos are (3, 64*scale, 64*scale); 0 = none
        self.guided = False             # guide reservation: the full-resolution render weights the field's taps by the photo
        self.local = False              # local reservation: UMASK and the LOCAL flags per session
        self.history_depth = 0          # history reservation: how many marks a session can undo; 0 = none
        self._opened = set()
        self._sourced = set()           # ids whose SRC holds a photo
        self.canvases = 0               # canvas reservation: how many photos of up to canvas_max = (max_w, max_h); 0 = none
        self.canvas_max = (0, 0)
        self.feather = 0
        self.canvas_guided = False      # edge-aware compose: the placed sessions' fields are weighted by the canvas (reserve_canvas_guide)
        self._canvas_wh = []            # per canvas (w, h) of its picture, None before canvas_put
        self._placed = {}               # session id -> (canvas id, x, y, scale), or oriented (canvas id, cx2, cy2, ax, ay)
        self.tips = 0                   # tip reservation: how many brush tips the handle keeps; 0 = none
        self._tips = {}                 # tip -> (tw, th) of the tips that were set
        self._tip_footprint = False     # tip_footprint(): a tipped paint event leaves its tip's shape in the user mask
        self.pixels = 0                 # the pixel format of every window result (pixel_format): 0 planar, 1 rgb, 2 rgba, 3 bgra
        self.reserve(capacity)
        self._h.sessions_set_blend(npe_ops.gaussian_half_kernel(sigma, int(4.0 * float(sigma) + 0.5)))

    def reserve(self, capacity):
        """Grow (or shrink) the pool; sessions whose ids remain keep their state."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("a session pool holds at least one session, got %d" % capacity)
        self._h.sessions_reserve(capacity)
        self.capacity = capacity
        self._opened = {v for v in self._opened if v < capacity}
        self._sourced = {v for v in self._sourced if v < capacity}
        self._placed = {v: p for v, p in self._placed.items() if v < capacity}

    def pixel_format(self, fmt=None):
        """What render, brush_view, paint(view=), scroll(view=), compose and brush_compose return from now on: "planar" (0, the
        default) uint8 (n,3,vh,vw); "rgb" (1) uint8 (n,vh,vw,3); "rgba" (2) and "bgra" (3) uint8 (n,vh,vw,4) with A = 255 --
        npe_ops.pack_window of the planar result, stored that way by the device.  A name or an id sets the format; None changes
        nothing.  -> the name of the format in force.  shown, read(), canvas_read() and what the pool stores stay planar."""
        from . import npe_ops
        if fmt is not None:
            fid = npe_ops.pixel_format_id(fmt)
            self._h.sessions_set_pixels(fid)
            self.pixels = fid
        return npe_ops.PIXEL_FORMATS[self.pixels]

    def _window_out(self, n, vw, vh):
        """The array a window call writes: n windows of vw x vh in the pool's pixel format."""
        from . import npe_ops
        return np.empty(npe_ops.window_shape(n, vw, vh, self.pixels), np.uint8)

    def reserve_hires(self, scale):
        """Keep every session's photo at (3, 64*scale, 64*scale), scale in 1..16; 0 frees that again.  Changing the scale drops the
        sessions' sources (their 64x64 state stays)."""
        scale = int(scale)
        if not 0 <= scale <= 16:
            raise ValueError("scale must be in 0..16, got %d" % scale)
        if scale == 0 and self.canvases:
            raise ValueError("canvases are reserved: free them first (reserve_canvases(0))")
        self._h.sessions_reserve_hires(scale)
        if scale != self.scale:
            self._sourced = set()
        self.scale = scale
        if not scale:
            self.guided = False

    def reserve_guide(self, sigma=None, table=None):
        """Edge-aware render: from now on render, brush_view / paint(view=) and commit weight the edit field's four bilinear taps by
        how close the photo's pixel is to each tap's pixel of the 64x64 picture (joint bilateral upsampling), so an edit no longer
        bleeds over the photo's edges.  Exactly one of sigma (levels per channel; the table is npe_ops.guide_table(sigma)) and table
        (766 positive float32 weights by summed absolute byte difference); neither switches the guide off again.  Needs reserve_hires
        first, and no canvases: compose renders with the plain bilinear tap."""
        from . import npe_ops
        if sigma is not None and table is not None:
            raise ValueError("give sigma or table, not both")
        if sigma is None and table is None:
            if self.scale:
                self._h.sessions_reserve_guide(None)
            self.guided = False
            return
        if not self.scale:
            raise ValueError("the pool has no full-resolution reservation (reserve_hires)")
        if self.canvases:
            raise ValueError("canvases are reserved: free them first (reserve_canvases(0))")
        if sigma is not None:
            table = npe_ops.guide_table(sigma)
        else:
            table = np.ascontiguousarray(np.asarray(table), np.float32)
            if table.shape != (npe_ops.GUIDE_TABLE_LEN,):
                raise ValueError("a guide table has %d entries, got shape %s" % (npe_ops.GUIDE_TABLE_LEN, table.shape))
            if not (np.isfinite(table).all() and (table > 0).all()):
                raise ValueError("every entry of a guide table is a finite positive weight")
        self._h.sessions_reserve_guide(table)
        self.guided = True

    def guide(self):
        """-> the float32 (766,) table of the reserved guide, from the library, or None without one."""
        if not self.scale:
            return None
        return self._h.sessions_guide()

    def reserve_local(self, on=True, sigma=0.3, dampen_thresh=0.75):
        """Keep a user mask (UMASK float64 (64,64)) and the LOCAL flags per session, 32 772 bytes each, and set the brush footprint's
        falloff (npe_ops.local_falloff_table(sigma); NPE.py:170 has 0.3) and the dampen threshold (NPE.py:187 has 0.75).  on=False
        frees them again.  Sessions start with flags 0: nothing changes until set_local."""
        from . import npe_ops
        if not on:
            self._h.sessions_reserve_local(False)
            self.local = False
            return
        sigma, dampen_thresh = float(sigma), float(dampen_thresh)
        if not (sigma > 0.0 and np.isfinite(sigma)):
            raise ValueError("sigma must be a positive number, got %r" % (sigma,))
        if not np.isfinite(dampen_thresh):
            raise ValueError("dampen_thresh must be finite, got %r" % (dampen_thresh,))
        table = npe_ops.local_falloff_table(sigma)
        self._h.sessions_reserve_local(True)
        self._h.sessions_set_local(table, dampen_thresh)
        self.local = True

    def set_local(self, ids, local=True, dampen=False, flags=None):
        """The sessions' LOCAL flags (bit 0 local: the blend is masked by where the user has brushed; bit 1 dampen), one value for
        all or one per session; their user masks are cleared, whichever flags are given."""
        if not self.local:
            raise ValueError("the pool has no local reservation (reserve_local)")
        idv, f = pack_session_local(ids, local, dampen, flags, self.capacity, self._opened)
        self._h.session_local(idv, f)

    def reserve_history(self, depth=16):
        """Keep up to `depth` (1..64) undoable states per session in device memory: (depth + 1) * (4 * zdim [+ 32 768 with the local
        reservation]) bytes each; 0 frees them.  Another depth clears every history.  Reserve the local edits first: while a history
        exists the library refuses to add or free them."""
        depth = int(depth)
        if not 0 <= depth <= 64:
            raise ValueError("depth must be in 0..64, got %d" % depth)
        self._h.sessions_reserve_history(depth)
        self.history_depth = depth

    def _need_history(self):
        if not self.history_depth:
            raise ValueError("the pool has no history reservation (reserve_history)")

    def mark(self, ids):
        """A stroke begins: the sessions' current states become undo targets (their redo tails go)."""
        self._need_history()
        self._h.session_mark(self._ids(ids, True))

    def undo(self, ids, steps=1):
        """Back `steps` marks (one value for all or one per session) -> what the canvases show, uint8 (n,3,64,64): the stored blend
        at the restored latent (photo mode) or the sample (sample mode)."""
        self._need_history()
        idv, st = pack_session_undo(ids, steps, self.capacity, self._opened)
        shown = np.empty((len(idv), 3, 64, 64), np.uint8)
        self._h.session_undo(idv, st, shown)
        return shown

    def redo(self, ids, steps=1):
        """Forward again `steps` states that undo went back over -> shown, as undo."""
        self._need_history()
        idv, st = pack_session_undo(ids, steps, self.capacity, self._opened)
        shown = np.empty((len(idv), 3, 64, 64), np.uint8)
        self._h.session_undo(idv, -st, shown)
        return shown

    def history(self, sid):
        """-> {"depth", "undo", "redo"}: the pool's depth and how many steps undo / redo can take on this session now.  The library
        owns the counters; nothing touches the device."""
        self._need_history()
        sid = int(sid)
        if not 0 <= sid < self.capacity:
            raise ValueError("session %d outside the pool (capacity %d)" % (sid, self.capacity))
        if sid not in self._opened:
            raise ValueError("session %d has not been opened" % sid)
        depth, undo, redo = self._h.session_history(sid)
        return {"depth": depth, "undo": undo, "redo": redo}

    def _layout(self):
        return self._zdim, self.scale, self.local, self.history_depth

    def record_info(self):
        """The record layout of this pool, from the library -> {"num_latents", "scale", "local", "depth", "body_bytes", "offsets"}:
        offsets are the byte offsets of the pool's arrays in a body, in npe_ops.session_record_columns' order."""
        layout, offsets = self._h.session_record_info()
        out = {k: int(getattr(layout, k)) for k in ("num_latents", "scale", "local", "depth", "body_bytes")}
        out["offsets"] = offsets
        return out

    def save(self, ids, device=False):
        """The whole state of the opened sessions `ids` -- pictures, latent, source, edit field, user mask, flags, undo history and
        cursor -- as SessionRecords, in one submission; the sessions stay as they are.  device=True keeps the bodies in device
        memory (a torch uint8 tensor, written on torch's current stream)."""
        from . import npe_ops
        idv = self._ids(ids, True)
        n, bb = len(idv), npe_ops.session_record_layout(*self._layout())[1]
        meta = np.zeros(n, npe_ops.SESSION_META_DTYPE)
        if device:
            import torch
            body = torch.empty((n, bb), dtype=torch.uint8, device="cuda")
            self._h.session_save(idv, meta, body, stream=torch.cuda.current_stream().cuda_stream)
        else:
            body = np.empty((n, bb), np.uint8)
            self._h.session_save(idv, meta, body)
        return SessionRecords(meta, body)

    def load(self, ids, records):
        """records[i] becomes session ids[i], opened or not: everything save() took, the undo history and its cursor included.  The
        records must come from a pool of this layout (latent size, scale, local, history depth) and belong to this model's weights.
        Nothing is displayed: read the session or redisplay it."""
        idv, meta, body = pack_session_records(ids, records, *self._layout(), capacity=self.capacity)
        if records.on_device:
            import torch
            self._h.session_load(idv, meta, body, stream=torch.cuda.current_stream().cuda_stream)
        else:
            self._h.session_load(idv, meta, body)
        for v, m in zip((int(v) for v in idv), meta):
            self._opened.add(v)
            self._placed.pop(v, None)
            (self._sourced.add if int(m["has_source"]) else self._sourced.discard)(v)

    # ---- brush tips ----
    def reserve_tips(self, count):
        """Room for `count` brush tips (0..64; 0 frees them).  Another count drops the tips that were set."""
        count = int(count)
        if not 0 <= count <= 64:
            raise ValueError("count must be in 0..64, got %d" % count)
        self._h.sessions_reserve_tips(count)
        if count != self.tips:
            self._tips = {}
            self._tip_footprint = False
        self.tips = count

    def tip_footprint(self, on=None):
        """on = True: from now on a paint event (brush, stroke, clone, restore, brush_compose, paint) that names a tip leaves the tip's
        own shape in the user mask (npe_ops.umask_paint_tip) where it left its rectangle's (npe_ops.umask_paint): under local edits a
        round brush no longer bleeds into the corners of its square.  False switches back; None changes nothing.  -> the setting in
        force.  Needs reserve_tips; another tip count switches it off.  Without reserve_local it changes nothing."""
        if on is not None:
            if not self.tips:
                raise ValueError("the pool has no tip reservation (reserve_tips)")
            self._h.sessions_set_tip_footprint(bool(on))
            self._tip_footprint = bool(on)
        return self._tip_footprint

    def _need_tip(self, tip):
        tip = int(tip)
        if not self.tips:
            raise ValueError("the pool has no tip reservation (reserve_tips)")
        if not 0 <= tip < self.tips:
            raise ValueError("tip %d outside the reservation (0..%d)" % (tip, self.tips - 1))
        return tip

    def set_tip(self, tip, weights, normalise=True):
        """Tip `tip` := weights (th, tw), both sides 1..64, every weight finite and >= 0.  normalise=True: a brush shape, e.g.
        npe_ops.round_tip(d, hardness), made a weighted mean by npe_ops.tip_weights (an all-ones shape is then the rectangle brush, bit
        for bit); False: the float32 weights as given (ian_sessions_set_tip's general weighted loss; all zero gives a zero gradient)."""
        from . import npe_ops
        tip = self._need_tip(tip)
        wn = npe_ops.tip_weights(weights) if normalise else np.ascontiguousarray(weights, np.float32)
        if wn.ndim != 2 or not 1 <= wn.shape[0] <= 64 or not 1 <= wn.shape[1] <= 64:
            raise ValueError("a tip has shape (th, tw) with both sides 1..64, got %s" % (wn.shape,))
        if not np.all(np.isfinite(wn)) or np.any(wn < 0):
            raise ValueError("the weights of a tip are finite and >= 0")
        self._h.sessions_set_tip(tip, wn)
        self._tips[tip] = (wn.shape[1], wn.shape[0])

    def tip(self, tip):
        """-> the float32 (th, tw) weights tip `tip` holds on the device."""
        tip = self._need_tip(tip)
        if tip not in self._tips:
            raise ValueError("tip %d has never been set (set_tip)" % tip)
        return self._h.sessions_tip(tip)

    def _tipsel(self, tips, boxes):
        if not self.tips:
            raise ValueError("the pool has no tip reservation (reserve_tips)")
        return pack_session_tips(tips, boxes, self._tips, self.tips)

    def _ids(self, ids, need_opened):
        return check_session_ids(ids, self.capacity, self._opened if need_opened else None)

    def _latents(self, z, n):
        z = np.ascontiguousarray(np.asarray(z, dtype=np.float32)).reshape(-1, self._zdim)
        if z.shape[0] != n:
            raise ValueError("z holds %d latents for %d sessions" % (z.shape[0], n))
        return z

    @staticmethod
    def _photos(photos, n, S):
        p = np.asarray(photos)
        if p.dtype != np.uint8:
            raise ValueError("photos must be uint8, got %s" % p.dtype)
        if p.shape == (3, S, S):
            p = p[None]
        if p.shape != (n, 3, S, S):
            raise ValueError("photos must have shape (%d,3,%d,%d), got %s" % (n, S, S, p.shape))
        return np.ascontiguousarray(p)

    def open(self, ids, photos):
        """infer: photos uint8 (n,3,64,64) (or (3,64,64) for one id) -> IM."""
        ids = self._ids(ids, False)
        shown = np.empty((len(ids), 3, 64, 64), np.uint8)
        self._h.session_open(ids, self._photos(photos, len(ids), 64), 0, shown)
        self._opened.update(int(v) for v in ids)
        self._sourced.difference_update(int(v) for v in ids)
        self._unplace(ids)
        return shown

    def open_hires(self, ids, photos):
        """infer from full-size photos: uint8 (n,3,S,S), S = 64*scale (or (3,S,S) for one id) -> IM, the 64x64 box mean."""
        if not self.scale:
            raise ValueError("the pool has no full-resolution reservation (reserve_hires)")
        ids = self._ids(ids, False)
        shown = np.empty((len(ids), 3, 64, 64), np.uint8)
        self._h.session_open_hires(ids, self._photos(photos, len(ids), 64 * self.scale), shown)
        self._opened.update(int(v) for v in ids)
        self._sourced.update(int(v) for v in ids)
        self._unplace(ids)
        return shown

    def _views(self, ids, origins, size, events=None, zoom=1):
        return pack_session_views(ids, origins, size, self.scale, self.capacity, self._opened, self._sourced, events, zoom)

    def render(self, ids, origins, size, zoom=1):
        """Windows of the pictures at full resolution, as last displayed -> uint8 (n,3,vh,vw) (pixel_format: (n,vh,vw,3|4)).  origins (n,2) or (2,) as (x, y),
        size (vw, vh) or one integer; x and vw multiples of 4.  The same id may appear several times (tiles).  zoom = k > 1: the
        views at 1/k (npe_ops.hires_render_zoom): origins stay in full-resolution pixels, size is the output's, and the source
        window (x, y, k*vw, k*vh) must lie inside the picture (npe_ops.zoom_window gives the size that shows all of it)."""
        views, vw, vh = self._views(ids, origins, size, None, zoom)
        out = self._window_out(len(views), vw, vh)
        if zoom == 1:
            self._h.session_render(views, vw, vh, out)
        else:
            self._h.session_zoom(views, vw, vh, zoom, out)
        return out

    def brush_view(self, ids, boxes, colours=None, modes=None, weight=0.05, sign=-1.0, origins=(0, 0), size=64, tips=None, zoom=1):
        """brush, and window i of session ids[i] at full resolution after its event, in ONE submission -> (shown, out).  tips: as in
        brush.  zoom: as in render."""
        ev = pack_session_events(ids, boxes, colours, modes, weight, sign, capacity=self.capacity, opened=self._opened)
        views, vw, vh = self._views(ids, origins, size, ev, zoom)
        shown = np.empty((len(ev), 3, 64, 64), np.uint8)
        out = self._window_out(len(ev), vw, vh)
        sel = None if tips is None else self._tipsel(tips, self._event_boxes(ev))
        if zoom != 1:
            self._h.session_brush_zoom(ev, sel, shown, views, vw, vh, zoom, out)
        elif tips is None:
            self._h.session_brush_view(ev, views, vw, vh, out, shown)
        else:
            self._h.session_brush_tip(ev, sel, shown, views, vw, vh, out)
        return shown, out

    @staticmethod
    def _event_boxes(ev):
        return [[(e.c1, e.r1, e.c2, e.r2)] for e in ev]

    # ---- canvases ----
    def _unplace(self, ids):
        for v in ids:
            self._placed.pop(int(v), None)

    def _need_canvases(self):
        if not self.canvases:
            raise ValueError("the pool has no canvas reservation (reserve_canvases)")

    def _canvas(self, cid, need_put=True):
        self._need_canvases()
        if int(cid) != cid or not 0 <= int(cid) < self.canvases:
            raise ValueError("canvas %r outside 0..%d" % (cid, self.canvases - 1))
        if need_put and self._canvas_wh[int(cid)] is None:
            raise ValueError("canvas %d holds no picture (canvas_put)" % int(cid))
        return int(cid)

    def reserve_canvases(self, count, max_w=0, max_h=0, feather=4):
        """Keep `count` (1..64) photos of up to max_w x max_h pixels (64..8192 each, max_w a multiple of 4) in device memory,
        3 * max_w * max_h bytes each; feather (0..16) is the width, in 64x64 field pixels, over which a placed session's edit fades
        towards the edge of its square.  0 frees them and every placement.  Needs reserve_hires first.  A second reservation starts
        from nothing: no canvas holds a picture, no session is placed, the compose is the plain one (reserve_canvas_guide)."""
        count, max_w, max_h, feather = int(count), int(max_w), int(max_h), int(feather)
        if not 0 <= count <= 64:
            raise ValueError("count must be in 0..64, got %d" % count)
        if count:
            if not self.scale:
                raise ValueError("the pool has no full-resolution reservation (reserve_hires)")
            if self.guided:
                raise ValueError("a guide is reserved: free it first (reserve_guide())")
            if not (64 <= max_w <= 8192 and 64 <= max_h <= 8192):
                raise ValueError("max_w and max_h must be in 64..8192, got %d x %d" % (max_w, max_h))
            if max_w % 4:
                raise ValueError("max_w %d is not a multiple of 4" % max_w)
            if not 0 <= feather <= 16:
                raise ValueError("feather must be in 0..16, got %d" % feather)
        self._h.sessions_reserve_canvas(count, max_w, max_h, feather)
        self.canvases, self.canvas_max, self.feather = count, ((max_w, max_h) if count else (0, 0)), (feather if count else 0)
        self._canvas_wh = [None] * count
        self._placed = {}
        self.canvas_guided = False

    def reserve_canvas_guide(self, sigma=None, table=None):
        """Edge-aware compose: from now on compose, brush_compose and canvas_commit weight the four bilinear taps of every photo-mode
        placement's edit field by how close the canvas's pixel is to each tap's pixel of the session's 64x64 picture
        (npe_ops.canvas_compose_guided), so an edit no longer bleeds over the photo's edges, by up to `scale` pixels.  Exactly one of
        sigma (levels per channel; the table is npe_ops.guide_table(sigma)) and table (766 positive float32 weights by summed absolute
        byte difference); neither switches back to the plain compose.  Needs reserve_canvases first; a new canvas reservation
        switches it off."""
        from . import npe_ops
        if sigma is not None and table is not None:
            raise ValueError("give sigma or table, not both")
        if sigma is None and table is None:
            if self.canvases:
                self._h.sessions_reserve_edges(None)
            self.canvas_guided = False
            return
        self._need_canvases()
        if any(len(q) == 5 for q in self._placed.values()):
            raise ValueError("oriented placements exist: the edge-aware compose is for upright squares")
        if sigma is not None:
            table = npe_ops.guide_table(sigma)
        else:
            table = np.ascontiguousarray(np.asarray(table), np.float32)
            if table.shape != (npe_ops.GUIDE_TABLE_LEN,):
                raise ValueError("a guide table has %d entries, got shape %s" % (npe_ops.GUIDE_TABLE_LEN, table.shape))
            if not (np.isfinite(table).all() and (table > 0).all()):
                raise ValueError("every entry of a guide table is a finite positive weight")
        self._h.sessions_reserve_edges(table)
        self.canvas_guided = True

    def canvas_guide(self):
        """-> the float32 (766,) table of the edge-aware compose, from the library, or None while the compose is the plain one."""
        if not self.canvases:
            return None
        return self._h.sessions_edges()

    def canvas_put(self, cid, photo):
        """The picture of canvas cid := photo, uint8 (3,h,w) (a numpy array, or a torch device tensor), 64 <= w <= max_w with w a
        multiple of 4, 64 <= h <= max_h.  Every session placed on that canvas is un-placed; its 64x64 state stays."""
        cid = self._canvas(cid, need_put=False)
        dev = hasattr(photo, "data_ptr")
        p = photo if dev else np.ascontiguousarray(photo)
        if str(p.dtype).split(".")[-1] != "uint8" or len(p.shape) != 3 or p.shape[0] != 3:
            raise ValueError("a canvas photo is uint8 (3,h,w), got %s %s" % (p.dtype, tuple(p.shape)))
        if dev and not p.is_contiguous():
            raise ValueError("a device photo must be contiguous")
        h, w = int(p.shape[1]), int(p.shape[2])
        if not (64 <= w <= self.canvas_max[0] and 64 <= h <= self.canvas_max[1]):
            raise ValueError("photo %d x %d outside 64 x 64 .. %d x %d" % (w, h, self.canvas_max[0], self.canvas_max[1]))
        if w % 4:
            raise ValueError("photo width %d is not a multiple of 4 (pad it)" % w)
        self._h.canvas_put(cid, p)
        self._canvas_wh[cid] = (w, h)
        self._placed = {v: q for v, q in self._placed.items() if q[0] != cid}

    def place(self, ids, cids, origins, scales):
        """Sessions ids[i] open on the exact box mean of the square origins[i] + 64*scales[i] of canvas cids[i] (pack_canvas_placements)
        and are placed there -> IM, uint8 (n,3,64,64).  Exactly open() of that box mean, in one submission; a session already placed moves."""
        self._need_canvases()
        items = pack_canvas_placements(ids, cids, origins, scales, self._canvas_wh, {v: q[0] for v, q in self._placed.items()},
                                       self.capacity)
        self._one_form(items, 4)
        shown = np.empty((len(items), 3, 64, 64), np.uint8)
        self._h.canvas_place(items, shown)
        for p in items:
            self._opened.add(p.session)
            self._sourced.discard(p.session)
            self._placed[p.session] = (p.canvas, p.x, p.y, p.scale)
        return shown

    def _one_form(self, items, words):
        """A canvas holds placements of one form (words = 4: upright, 5: oriented): refused while any of the other form remains."""
        moving = {p.session for p in items}
        for i, p in enumerate(items):
            k = sum(1 for v, q in self._placed.items() if q[0] == p.canvas and len(q) != words and v not in moving)
            if k:
                raise ValueError("item %d: canvas %d holds %d %s placements: a canvas holds one form (place upright squares at angle 0)"
                                 % (i, p.canvas, k, "oriented" if words == 4 else "upright"))

    def place_oriented_raw(self, ids, cids, items):
        """Sessions ids[i] open on the oriented gather (npe_ops.canvas_crop_mean_oriented) of the square items[i] = (cx2, cy2, ax, ay)
        of canvas cids[i] (pack_canvas_oriented) and are placed there -> IM, uint8 (n,3,64,64).  Exactly open() of that picture, in
        one submission; a session already placed, in either form, moves.  A canvas holds placements of one form, and the edge-aware
        compose (reserve_canvas_guide) has no oriented form."""
        self._need_canvases()
        if self.canvas_guided:
            raise ValueError("the edge-aware compose is on: free it first (reserve_canvas_guide())")
        items = pack_canvas_oriented(ids, cids, items, self._canvas_wh, {v: q[0] for v, q in self._placed.items()}, self.capacity)
        self._one_form(items, 5)
        shown = np.empty((len(items), 3, 64, 64), np.uint8)
        self._h.place_oriented(items, shown)
        for p in items:
            self._opened.add(p.session)
            self._sourced.discard(p.session)
            self._placed[p.session] = (p.canvas, p.cx2, p.cy2, p.ax, p.ay)
        return shown

    def place_oriented(self, ids, cids, centres, sides, angles):
        """place_oriented_raw with the squares given as centres (n,2) or (2,) in canvas pixels (pixel X covers [X, X+1): 0.5 steps are
        exact), sides in pixels (64..1024; one value or (n,)) and angles in degrees (one value or (n,)), through
        npe_ops.oriented_placement.  A side of exactly 64 or 1024 is safe at multiples of 90 degrees only: elsewhere the rounding of
        (ax, ay) may leave ax*ax + ay*ay just outside its range."""
        from . import npe_ops
        n = len(np.asarray(ids).reshape(-1))
        c = np.asarray(centres, np.float64)
        if c.shape == (2,):
            c = np.tile(c, (n, 1))
        sd, an = np.asarray(sides, np.float64), np.asarray(angles, np.float64)
        sd = np.tile(sd, n) if sd.ndim == 0 else sd
        an = np.tile(an, n) if an.ndim == 0 else an
        if c.shape != (n, 2) or sd.shape != (n,) or an.shape != (n,) or not (np.isfinite(c).all() and np.isfinite(sd).all() and np.isfinite(an).all()):
            raise ValueError("centres must be finite of shape (%d,2) or (2,), sides and angles one finite value or %d" % (n, n))
        items = [npe_ops.oriented_placement(c[i, 0], c[i, 1], sd[i], an[i]) for i in range(n)]
        return self.place_oriented_raw(ids, cids, np.asarray(items, np.int64).reshape(n, 4))

    def placements_oriented(self, cid):
        """-> [(session, cx2, cy2, ax, ay)] of the oriented sessions placed on canvas cid, in ascending session id."""
        cid = self._canvas(cid, need_put=False)
        return sorted((v,) + tuple(q[1:]) for v, q in self._placed.items() if q[0] == cid and len(q) == 5)

    def _windows(self, cids, origins, size, zoom=1):
        self._need_canvases()
        return pack_canvas_windows(cids, origins, size, self._canvas_wh, zoom)

    def compose(self, cids, origins, size, zoom=1):
        """Windows of the canvases with every placed session's edit on top (npe_ops.canvas_compose; after reserve_canvas_guide
        npe_ops.canvas_compose_guided) -> uint8 (n,3,vh,vw) (pixel_format: (n,vh,vw,3|4)).  origins (n,2) or (2,) as (x, y), size (vw, vh) or one integer; x and vw
        multiples of 4.  The same canvas may appear several times.  zoom = k > 1: the windows at 1/k (npe_ops.canvas_compose_zoom),
        as in render."""
        win, vw, vh = self._windows(cids, origins, size, zoom)
        out = self._window_out(len(win), vw, vh)
        if zoom == 1:
            self._h.canvas_compose(win, vw, vh, out)
        else:
            self._h.compose_zoom(win, vw, vh, zoom, out)
        return out

    def brush_compose(self, ids, boxes, colours=None, modes=None, weight=0.05, sign=-1.0, windows=None, tips=None):
        """brush on sessions ids, and the windows = (cids, origins, size) or (cids, origins, size, zoom) of compose() after it, in ONE
        submission -> (shown, out).  The sessions need not be placed, the windows need not show them.  After reserve_canvas_guide
        the windows are npe_ops.canvas_compose_guided's.  tips: as in brush (ian_compose_brush_soft); windows at a zoom have no
        tipped form."""
        if windows is None or len(windows) not in (3, 4):
            raise ValueError("windows must be (cids, origins, size) or (cids, origins, size, zoom)")
        ev = pack_session_events(ids, boxes, colours, modes, weight, sign, capacity=self.capacity, opened=self._opened)
        win, vw, vh = self._windows(*windows)
        zoom = windows[3] if len(windows) == 4 else 1
        shown = np.empty((len(ev), 3, 64, 64), np.uint8)
        out = self._window_out(len(win), vw, vh)
        if tips is not None:
            if zoom != 1:
                raise ValueError("brush_compose with tips has no zoomed form: compose(zoom=) after brush(tips=)")
            self._h.canvas_brush_tip(ev, self._tipsel(tips, self._event_boxes(ev)), win, vw, vh, out, shown)
        elif zoom == 1:
            self._h.canvas_brush(ev, win, vw, vh, out, shown)
        else:
            self._h.compose_brush_zoom(ev, win, vw, vh, zoom, out, shown)
        return shown, out

    def canvas_commit(self, cid):
        """The canvas becomes its own compose, in place; the sessions placed on it open again on the box means of the new picture, where
        they are -> IM of those sessions in ascending id, uint8 (k,3,64,64).  After reserve_canvas_guide the new picture is
        npe_ops.canvas_compose_guided of the whole canvas."""
        cid = self._canvas(cid)
        k = sum(1 for q in self._placed.values() if q[0] == cid)
        shown = np.empty((k, 3, 64, 64), np.uint8)
        self._h.canvas_commit(cid, shown if k else None)
        return shown

    def canvas_read(self, cid):
        """The stored picture of a canvas, uint8 (3,h,w): without the placed sessions' edits until canvas_commit.  A synchronising copy."""
        return self._h.canvas_read(self._canvas(cid))

    def placements(self, cid):
        """-> [(session, x, y, scale)] of the sessions placed on canvas cid, in ascending session id."""
        cid = self._canvas(cid, need_put=False)
        return sorted((v, q[1], q[2], q[3]) for v, q in self._placed.items() if q[0] == cid and len(q) == 4)

    def reset(self, ids):
        """Reset: re-open from the stored GIM."""
        ids = self._ids(ids, True)
        shown = np.empty((len(ids), 3, 64, 64), np.uint8)
        self._h.session_open(ids, None, 0, shown)
        return shown

    def commit(self, ids):
        """UpdateGIM: GIM := IM, then Reset.  A session placed on a canvas is refused: canvas_commit is its form."""
        ids = self._ids(ids, True)
        for i, v in enumerate(int(v) for v in ids):
            if v in self._placed:
                raise ValueError("item %d: session %d is placed on canvas %d: commit the canvas instead (canvas_commit)" % (i, v, self._placed[v][0]))
        shown = np.empty((len(ids), 3, 64, 64), np.uint8)
        self._h.session_open(ids, None, 1, shown)
        return shown

    def sample(self, ids, z):
        """sample with the caller's z (n, zdim): the sessions go to sample mode -> RECON."""
        ids = self._ids(ids, True)
        shown = np.empty((len(ids), 3, 64, 64), np.uint8)
        self._h.session_set_latent(ids, self._latents(z, len(ids)), 1, shown)
        return shown

    def set_latent(self, ids, z):
        """paint_latents: Z := z -> the blended photo (photo mode) or the sample (sample mode); the stored IM stays."""
        ids = self._ids(ids, True)
        shown = np.empty((len(ids), 3, 64, 64), np.uint8)
        self._h.session_set_latent(ids, self._latents(z, len(ids)), 0, shown)
        return shown

    def fit(self, ids, steps=20, lr=0.02, boxes=None, want_loss=True):
        """Fit the sessions' latents to their own photos (ian_session_fit): `steps` Adam steps at learning rate lr on the API.py:64
        loss between sample_at(Z) and the photo, over boxes (n,4) or (4,) as (c1,r1,c2,r2) (None: the whole picture), all on the
        device in one submission; then the sessions stand as after reset() but at the fitted latent: RECON and ERROR belong to
        it, photo mode, user mask and undo history cleared.  -> (RECON uint8 (n,3,64,64), loss float64 (n, steps+1) or None):
        loss[i, t] is the loss at the latent after t steps.  The defaults 20 and 0.02 are a starting point nobody has measured."""
        items, steps, lr = pack_session_fit(ids, steps, lr, boxes, self.capacity, self._opened)
        recon = np.empty((len(items), 3, 64, 64), np.uint8)
        loss = np.empty((len(items), steps + 1), np.float64) if want_loss else None
        self._h.session_fit(items, steps, lr, loss, recon)
        return recon, loss

    def brush(self, ids, boxes, colours=None, modes=None, weight=0.05, sign=-1.0, tips=None):
        """n brush events (pack_session_events) in one submission -> shown.  tips: one tip index for all events or one per event
        (-1 = none, the plain rectangle event): the event's loss is weighted by that tip (set_tip), whose size the box must have."""
        ev = pack_session_events(ids, boxes, colours, modes, weight, sign, capacity=self.capacity, opened=self._opened)
        shown = np.empty((len(ev), 3, 64, 64), np.uint8)
        if tips is None:
            self._h.session_brush(ev, shown)
        else:
            self._h.session_brush_tip(ev, self._tipsel(tips, self._event_boxes(ev)), shown)
        return shown

    def clone(self, ids, boxes, sources, offsets=(0, 0), field="GIM", steps=1, weight=0.05, sign=-1.0, tips=None):
        """The clone brush (ian_session_clone): the rectangle boxes[i] of session ids[i] is pulled towards the rectangle shifted by
        offsets[i] = (dc, dr) of session sources[i]'s GIM, IM or RECON (pack_session_clones), `steps` gradient steps (1..64) in one
        submission -> shown uint8 (n,3,64,64).  Each step is a paint event whose target is that picture instead of a flat colour; the
        sessions end byte for byte where `steps` calls with steps=1 leave them.  For one undo step call mark(ids) first.  tips: one
        tip index for all events or one per event (-1 = none, the plain clone event): the event's loss is weighted by that tip
        (ian_session_stamp_soft; npe_ops.clone_tip_seed), whose size the box must have: a soft round clone stamp."""
        steps = check_clone_steps(steps)
        ev = pack_session_clones(ids, boxes, sources, offsets, field, weight, sign, capacity=self.capacity, opened=self._opened)
        shown = np.empty((len(ev), 3, 64, 64), np.uint8)
        if tips is None:
            self._h.session_clone(ev, steps, shown)
        else:
            self._h.session_clone_tip(ev, self._tipsel(tips, self._event_boxes(ev)), steps, shown)
        return shown

    def restore(self, ids, boxes, steps=1, weight=0.05, tips=None):
        """The restore brush: the rectangles are pulled back towards the sessions' own photos -- clone from each session's own GIM at
        offset 0.  The user mask, the edit field and the undo history go on as for a paint event (reset and fit would clear them).
        tips: as in clone."""
        idv = self._ids(ids, True)
        return self.clone(idv, boxes, idv, (0, 0), "GIM", steps, weight, -1.0, tips)

    def stroke(self, ids, paths, colours=None, modes=None, weight=0.05, sign=-1.0, mark=False, tips=None):
        """Whole brush paths in one submission (ian_session_stroke): paths = one (K_i,4) array of rectangles per session, 1..64 points,
        applied in order with the stroke's one colour / mode / weight / sign (pack_session_strokes).  The sessions end byte for byte
        where the loop `for k: brush(the sessions with more than k points)` leaves them -> shown uint8 (n,3,64,64), in the caller's
        order: what each session's LAST point displays.  mark=True saves the states first, as mark(ids) would, in the same
        submission: one stroke is one undo step.  For windows call render or compose afterwards.  tips: one tip index for all strokes
        or one per stroke, in the caller's order (-1 = none); every rectangle of a stroke must have its tip's size."""
        if mark:
            self._need_history()
        strokes, boxes, perm = pack_session_strokes(ids, paths, colours, modes, weight, sign, capacity=self.capacity, opened=self._opened)
        got = np.empty((len(strokes), 3, 64, 64), np.uint8)
        if tips is None:
            self._h.session_stroke(strokes, boxes, 1 if mark else 0, got)
        else:
            sel = self._tipsel(tips, [np.asarray(p).reshape(-1, 4) for p in (list(paths) if not isinstance(paths, list) else paths)])
            self._h.session_path_tip(strokes, np.ascontiguousarray(sel[perm]), boxes, 1 if mark else 0, got)    # sorted stroke j carries the tip of the caller's item perm[j]
        shown = np.empty_like(got)
        shown[perm] = got                      # sorted stroke j is the caller's item perm[j]
        return shown

    def paint_stroke(self, ids, points, colours_uint8, d=12, weight=0.05, mark=True, tip=None):
        """A drag of NPE.paint per session: points = one (K_i,2) array of (x, y) mouse positions in 64-pixel space per session (NPE.py:148
        has event.x//4), d = the brush-size slider (npe_ops.brush_rect gives each point move_mouse's rectangle), painted toward
        colours_uint8 (levels 0..255) -> shown, as stroke.  tip: paint with that brush tip instead: every point becomes the
        npe_ops.tip_rect rectangle of the tip's size, and d is ignored."""
        from . import npe_ops
        paths = []
        if tip is not None:
            tip = self._need_tip(tip)
            if tip not in self._tips:
                raise ValueError("tip %d has never been set (set_tip)" % tip)
            tw, th = self._tips[tip]
        for i, p in enumerate(points):
            q = np.asarray(p)
            if q.ndim != 2 or q.shape[1] != 2:
                raise ValueError("item %d: the points of a stroke have shape (K,2) as (x,y), got %s" % (i, q.shape))
            rect = (lambda x, y: npe_ops.brush_rect(x, y, d)) if tip is None else (lambda x, y: npe_ops.tip_rect(x, y, tw, th))
            paths.append(np.array([rect(x, y) for x, y in q], np.int64).reshape(-1, 4))
        return self.stroke(ids, paths, colours_uint8, None, weight, -1.0, mark, tip)

    def paint(self, ids, boxes, colours_uint8, weight=0.05, view=None, tips=None):
        """NPE.paint: Z -= weight * grad toward the brush colour (levels 0..255 per channel).  view = (origins, size) or (origins,
        size, zoom): also the full-resolution windows, as brush_view -> (shown, out).  tips: as in brush."""
        if view is not None:
            origins, size, zoom = self._view3(view)
            return self.brush_view(ids, boxes, colours_uint8, None, weight, -1.0, origins, size, tips, zoom)
        return self.brush(ids, boxes, colours_uint8, None, weight, -1.0, tips)

    @staticmethod
    def _view3(view):
        if len(view) not in (2, 3):
            raise ValueError("view must be (origins, size) or (origins, size, zoom)")
        return tuple(view) if len(view) == 3 else (view[0], view[1], 1)

    def scroll(self, ids, boxes, signs, weight=0.1, view=None, tips=None):
        """NPE.scroll: Z += sign(event.delta) * weight * grad of the patch mean.  view = (origins, size): as in paint.  tips: as in
        brush."""
        if view is not None:
            origins, size, zoom = self._view3(view)
            return self.brush_view(ids, boxes, None, None, weight, signs, origins, size, tips, zoom)
        return self.brush(ids, boxes, None, None, weight, signs, tips)

    def read(self, sid):
        """-> {"Z" (zdim,), "RECON", "ERROR", "IM", "GIM" (3,64,64), "MODE" int}; in a full-resolution pool also "FIELD" (3,64,64),
        "FIELD_KIND" int and, for a session that holds one, "SOURCE" (3,S,S); in a pool with the local reservation also "UMASK"
        float64 (64,64) and "LOCAL" int.  One synchronising copy (ian_session_read) per field:
        for tests and for saving a picture, not for the event loop."""
        sid = int(sid)
        if not 0 <= sid < self.capacity:
            raise ValueError("session %d outside the pool (capacity %d)" % (sid, self.capacity))
        if sid not in self._opened:
            raise ValueError("session %d has not been opened" % sid)
        out = {k: self._h.session_read(sid, k) for k in ("Z", "RECON", "ERROR", "IM", "GIM")}
        out["MODE"] = int(self._h.session_read(sid, "MODE")[0])
        if self.scale:
            out["FIELD"] = self._h.session_read(sid, "FIELD")
            out["FIELD_KIND"] = int(self._h.session_read(sid, "FIELD_KIND")[0])
            if sid in self._sourced:
                out["SOURCE"] = self._h.session_read(sid, "SOURCE", scale=self.scale)
        if self.local:
            out["UMASK"] = self._h.session_read(sid, "UMASK")
            out["LOCAL"] = int(self._h.session_read(sid, "LOCAL")[0])
        return out

    def close(self):
        """Free the pool."""
        if self.capacity:
            self._h.sessions_reserve(0)
            self.capacity = 0
            self.scale = 0
            self.local = False
            self.history_depth = 0
            self._opened = set()
            self._sourced = set()
            self.canvases, self.canvas_max, self.feather, self._canvas_wh, self._placed = 0, (0, 0), 0, [], {}
            self.tips, self._tips = 0, {}
            self.pixels = 0


class IAN:
    def __init__(self, config_path, dnn=True, params=None, deconv_flip=True):
        """config_path, dnn: as API.py:12.  ``params`` (optional extension): dict of Theano-named arrays
        used instead of the '<config>.npz' checkpoint (tests and the benchmark use synthetic weights
        because the reference's weight files are absent)."""
        config_module = config_loader.load_config(config_path)
        self.cfg = config_module.cfg                                   # API.py:19
        self.weights_fname = str(config_path)[:-3] + ".npz"            # API.py:20
        self.model = config_loader.build_model(config_module, dnn=dnn)  # API.py:21
        self.lowered = lowering.lower_model(self.model)
        self._h = Handle(self.lowered, deconv_flip=deconv_flip)
        self.metadata = {}

        # Load weights (API.py:23-30)
        specs = self.lowered.params
        if params is None:
            params = {}
            if os.path.exists(self.weights_fname):
                try:
                    params, self.metadata = checkpoints.load_weights(self.weights_fname, lowering.all_param_specs(self.model))
                except Exception as exc:  # e.g. a git-LFS pointer instead of the archive
                    warnings.warn("could not read %s (%s); parameters keep their initial values" % (self.weights_fname, exc))
            else:
                warnings.warn("weights file %s not found; parameters keep their initial values" % self.weights_fname)
        rs = np.random.RandomState(0)
        for p in specs:
            arr = params.get(p.name)
            if arr is None:
                logging.warning("unable to load parameter %s", p.name)
                arr = p.init.sample(p.shape, rs)
            elif tuple(np.shape(arr)) != p.shape:
                raise ValueError("parameter %s has shape %s, expected %s" % (p.name, np.shape(arr), p.shape))
            self._h.load_param(p.name, arr)

        # Shuffle weights if using IAF with MADE (API.py:32-36): reset("Once") on both MADEs
        if "l_IAF_mu" in self.model:
            self.model["l_IAF_mu"].reset("Once")
            self.model["l_IAF_ls"].reset("Once")
        if self.lowered.has_made:
            self.made_masks = made.masks_once(self.lowered.num_latents)
            self._h.set_made_masks(*self.made_masks)
        self._h.finalize()
        self._zdim = self.lowered.num_latents

    # ---- helpers -------------------------------------------------------------------------------------
    @staticmethod
    def _f32(a, shape_tail, what):
        if not (type(a) is np.ndarray and a.dtype == np.float32 and a.flags.c_contiguous):    # the interactive loop passes ready arrays
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        if a.ndim != len(shape_tail) + 1 or tuple(a.shape[1:]) != tuple(shape_tail):
            raise ValueError("%s must have shape (n,%s), got %s" % (what, ",".join(map(str, shape_tail)), a.shape))
        if a.shape[0] < 1:
            raise ValueError("%s is empty" % what)
        return a

    def _grad_out(self, z):
        """API.py:59,64 differentiate a loss on X_hat[0] with respect to the WHOLE Z: the result has Z's shape (n, zdim) and, the
        decoder being deterministic (per-sample), rows 1.. are exactly zero.  NPE.py only ever passes n = 1."""
        return np.empty((1, self._zdim), np.float32) if z.shape[0] == 1 else np.zeros((z.shape[0], self._zdim), np.float32)

    def _run(self, fn, src, out_tail):
        out = np.empty((src.shape[0],) + tuple(out_tail), np.float32)
        self._h.call(fn, src, src.shape[0], out)
        return out

    # ---- API.py surface ------------------------------------------------------------------------------
    def imgrad(self, c1, r1, c2, r2, z):
        """API.py:66-70: change in latents which would lighten the local image patch."""
        z = self._f32(z, (self._zdim,), "z")
        dz = self._grad_out(z)
        self._h.grad_light(int(c1), int(r1), int(c2), int(r2), z[:1], dz[:1])
        return dz

    def imgradRGB(self, c1, r1, c2, r2, RGB, z):
        """API.py:72-76: change in latents which would move the patch towards RGB."""
        z = self._f32(z, (self._zdim,), "z")
        rgb = self._f32(RGB, (3, 64, 64), "RGB")
        dz = self._grad_out(z)
        self._h.grad_rgb(int(c1), int(r1), int(c2), int(r2), rgb[:1], z[:1], dz[:1])
        return dz

    def encode_images(self, images):
        """API.py:78-90: n x 3 x 64 x 64 in [-1,1] -> n x zdim."""
        return self._run("ian_encode", self._f32(images, (3, 64, 64), "images"), (self._zdim,))

    def get_zdim(self):
        """API.py:92-96."""
        return self.cfg["num_latents"]

    def sample_at(self, z):
        """API.py:98-110: n x zdim -> n x 3 x 64 x 64."""
        return self._run("ian_decode", self._f32(z, (self._zdim,), "z"), (3, 64, 64))

    # ---- what NPE.py does with the decoder output on every edit, on the device ----------
    def sample_at_uint8(self, z):
        """np.uint8(from_tanh(sample_at(z))) as in NPE.py:110,261 (update_photo, RECON): n x zdim -> uint8 n x 3 x 64 x 64;
        the float image never leaves the device."""
        z = self._f32(z, (self._zdim,), "z")
        out = np.empty((z.shape[0], 3, 64, 64), np.uint8)
        self._h.call("ian_decode_u8", z, z.shape[0], out)
        return out

    def photo_blend(self, z, recon_uint8, error, sigma=0.7):
        """NPE.paint's photo-mode blend (NPE.py:218-231) chained after the decoder on the device:
        -> (IM uint8 (3,64,64), MASK float64 (64,64)), bit-exact with the numpy/scipy expression (npe_ops.photo_blend_host)."""
        from . import npe_ops
        z = self._f32(z, (self._zdim,), "z")
        recon = np.ascontiguousarray(recon_uint8, dtype=np.uint8)
        err = np.ascontiguousarray(error, dtype=np.float32)
        if recon.shape != (3, 64, 64) or err.shape != (3, 64, 64):
            raise ValueError("RECON and ERROR must have shape (3,64,64)")
        half = npe_ops.gaussian_half_kernel(sigma, int(4.0 * float(sigma) + 0.5))
        im, mask = np.empty((3, 64, 64), np.uint8), np.empty((64, 64), np.float64)
        self._h.photo_blend(z[:1], recon, err, half, im, mask)
        return im, mask

    def brush_step(self, c1, r1, c2, r2, z, RGB=None, weight=0.05, sign=-1.0, image=True, photo=None, sigma=0.7, want_mask=False):
        """One whole NPE.paint / NPE.scroll event on the device (ian_brush_step): the latent gradient (imgradRGB when RGB is
        given, imgrad otherwise), Z + sign*weight*(dZ*(1+(c2-c1))) in float32 exactly as NPE.py:205-209 / 313-314 compute it,
        and sample_at of the new latent -- one submission instead of two calls with a host update between them.
        -> (z_new (1,zdim), image (1,3,64,64) or None)  or, with photo=(RECON uint8, ERROR float32),
           (z_new, image or None, IM uint8 (3,64,64), MASK float64 (64,64) if want_mask else None)  (photo mode,
           NPE.py:218-231; NPE.paint itself only displays IM, so the 32 KB mask stays on the device unless asked for)."""
        z = self._f32(z, (self._zdim,), "z")
        rgb = self._f32(RGB, (3, 64, 64), "RGB")[:1] if RGB is not None else None
        z_new = np.empty((1, self._zdim), np.float32)
        x = np.empty((1, 3, 64, 64), np.float32) if image else None
        pa = None
        if photo is not None:
            recon = np.ascontiguousarray(photo[0], dtype=np.uint8)
            err = np.ascontiguousarray(photo[1], dtype=np.float32)
            if recon.shape != (3, 64, 64) or err.shape != (3, 64, 64):
                raise ValueError("RECON and ERROR must have shape (3,64,64)")
            from . import npe_ops
            half = npe_ops.gaussian_half_kernel(sigma, int(4.0 * float(sigma) + 0.5))
            im, mask = np.empty((3, 64, 64), np.uint8), (np.empty((64, 64), np.float64) if want_mask else None)
            pa = (recon, err, half, im, mask)
        coef = float(sign) * float(weight)      # rounded to float32 at the boundary, as numpy rounds the scalar
        self._h.brush_step(int(c1), int(r1), int(c2), int(r2), rgb, z[:1], coef, float(1 + (int(c2) - int(c1))), z_new, None, x, pa)
        if photo is not None:
            return z_new, x, pa[3], pa[4]
        return z_new, x

    # ---- several editors: n brush events in one submission (ian_grad_batch / ian_brush_step_batch) ----------------------
    def imgrad_batch(self, boxes, z, RGB=None, modes=None):
        """Row i = imgradRGB(*boxes[i], RGB[i:i+1], z[i:i+1]) (mode 1) or imgrad(*boxes[i], z[i:i+1]) (mode 0), for n sessions in one
        submission.  boxes (n,4) as (c1,r1,c2,r2); modes default to 1 with RGB, 0 without.  -> dz (n, zdim)"""
        z = self._f32(z, (self._zdim,), "z")
        rgb = self._f32(RGB, (3, 64, 64), "RGB") if RGB is not None else None
        items = pack_brush_items(boxes, rgb.shape[0] if rgb is not None else None, modes)
        if z.shape[0] != len(items):
            raise ValueError("z holds %d latents for %d boxes" % (z.shape[0], len(items)))
        dz = np.empty((len(items), self._zdim), np.float32)
        self._h.grad_batch(items, rgb, z, dz)
        return dz

    def brush_step_batch(self, boxes, z, RGB=None, weight=0.05, sign=-1.0, modes=None, image=True, photo=None, sigma=0.7,
                         want_mask=False):
        """brush_step for n edit sessions in one submission (ian_brush_step_batch): per item the gradient, z + coef*(dz*gscale) with
        coef = float32(sign*weight) and gscale = 1 + (c2 - c1), and sample_at(z_new); weight / sign are scalars or length-n arrays.
        -> (z_new (n,zdim), x (n,3,64,64) or None)  or, with photo=(RECON uint8 (n,3,64,64), ERROR float32 (n,3,64,64)),
           (z_new, x or None, IM uint8 (n,3,64,64), MASK float64 (n,64,64) if want_mask else None)."""
        z = self._f32(z, (self._zdim,), "z")
        rgb = self._f32(RGB, (3, 64, 64), "RGB") if RGB is not None else None
        items = pack_brush_items(boxes, rgb.shape[0] if rgb is not None else None, modes, weight, sign)
        n = len(items)
        if z.shape[0] != n:
            raise ValueError("z holds %d latents for %d boxes" % (z.shape[0], n))
        z_new = np.empty((n, self._zdim), np.float32)
        x = np.empty((n, 3, 64, 64), np.float32) if image else None
        pa = None
        if photo is not None:
            recon = np.ascontiguousarray(photo[0], dtype=np.uint8)
            err = np.ascontiguousarray(photo[1], dtype=np.float32)
            if recon.shape != (n, 3, 64, 64) or err.shape != (n, 3, 64, 64):
                raise ValueError("RECON and ERROR must have shape (%d,3,64,64)" % n)
            from . import npe_ops
            half = npe_ops.gaussian_half_kernel(sigma, int(4.0 * float(sigma) + 0.5))
            im, mask = np.empty((n, 3, 64, 64), np.uint8), (np.empty((n, 64, 64), np.float64) if want_mask else None)
            pa = (recon, err, half, im, mask)
        self._h.brush_step_batch(items, rgb, z, z_new, None, x, pa)
        if photo is not None:
            return z_new, x, pa[3], pa[4]
        return z_new, x

    def sessions(self, capacity, sigma=0.7):
        """Device-resident edit sessions of this model (ian_session_*): -> EditSessions with `capacity` ids.  One pool per model:
        a second call re-sizes it (sessions whose ids remain keep their state) and the earlier object's bookkeeping is stale."""
        return EditSessions(self._h, capacity, self._zdim, sigma)

    # ---- sample_IAN.py function equivalents ----------------------------------------------
    def sampleZ(self, z):
        """sample_IAN.py:88: l_Z -> l_out (same as sample_at)."""
        return self.sample_at(z)

    def Zfn(self, images):
        """sample_IAN.py:90-91: image -> l_Z_IAF (deterministic)."""
        return self._run("ian_encode_pre_iaf", self._f32(images, (3, 64, 64), "images"), (self._zdim,))

    def Z_IAF_fn(self, z):
        """sample_IAN.py:93-94: l_Z_IAF -> l_Z."""
        return self._run("ian_iaf", self._f32(z, (self._zdim,), "z"), (self._zdim,))

    def sample(self, z):
        """sample_IAN.py:86: l_Z_IAF -> l_out."""
        return self.sample_at(self.Z_IAF_fn(z))

    def reconstruct(self, images):
        """encode_images followed by sample_at with the latent kept on the device (bench config 2)."""
        return self._run("ian_reconstruct", self._f32(images, (3, 64, 64), "images"), (3, 64, 64))

    # ---- introspection ---------------------------------------------------------------------------------
    def activation(self, name, n):
        """Activation (NCHW) of the named layer output from the last call (tests / debugging)."""
        return self._h.read_slot(self.lowered.slot_by_name(name), n)

    @property
    def handle(self):
        return self._h

    def close(self):
        self._h.close()
