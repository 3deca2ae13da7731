"""The steps that sit right after the hot path in every NPE edit (NPE.py:192-235, 276-314): the latent update and
the photo blend.  In the reference they are 64x64x3 numpy/scipy expressions inside the Tk callbacks; here

  * ``brush_step`` / ``lighten_step`` are the latent updates of NPE.paint / NPE.scroll (host arithmetic on 100 floats
    around the HIP gradient call); ``paint_event`` is the whole NPE.paint body as one device submission
    (``ian_brush_step``: gradient, latent update, decoder, optional blend);
  * ``photo_blend`` is NPE.paint's photo-mode blend (NPE.py:218-231).  With a ``neural_photo_editor_amd.IAN`` model it
    runs as ONE 64x64 HIP kernel chained after the decoder (``ian_photo_blend``, include/ian.h): the decoded image never
    leaves the device, the edit needs one 12 KB uint8 device->host copy;
  * ``photo_blend_host`` is the reference's expression itself, dtype for dtype (float32 DELTA, float64 MASK / D, the
    bare ``np.uint8`` cast) -- the oracle the kernel is tested against bit-for-bit, and the fallback for models that
    are not the HIP class (a test double).
"""
from __future__ import annotations

import numpy as np
from scipy.ndimage import gaussian_filter

BLEND_SIGMA = 0.7       # NPE.py:224
BLEND_RADIUS = 3        # scipy: int(truncate * sigma + 0.5) with truncate = 4.0


def to_tanh(x):
    """NPE.py:37-38 (dtype follows numpy promotion, as in the reference: uint8 -> float64, float32 -> float32)."""
    return 2.0 * (x / 255.0) - 1.0


def from_tanh(x):
    """NPE.py:40-41"""
    return 255.0 * (x + 1) / 2.0


def gaussian_half_kernel(sigma=BLEND_SIGMA, radius=BLEND_RADIUS):
    """Weights w[0..radius] (centre outwards) of scipy.ndimage's 1-D Gaussian (_filters._gaussian_kernel1d, order 0)."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], np.float64)


def separable_reflect_filter(a, half):
    """scipy.ndimage.gaussian_filter restated: axis 0 then axis 1, 'reflect' boundary (d c b a | a b c d | d c b a),
    float64, and NI_Correlate1D's summation order for a symmetric kernel:
        t = x[l]*w0;  for j = R..1:  t += (x[l-j] + x[l+j]) * w[j]
    -- the order the HIP kernel reproduces (kernels_npe.hip), so that its mask equals scipy's bit for bit."""
    a = np.asarray(a, np.float64)
    R = len(half) - 1
    for axis in (0, 1):
        x = np.moveaxis(a, axis, 0)
        n = x.shape[0]
        idx = np.arange(-R, n + R)
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
        xe = x[idx]
        t = xe[R:R + n] * half[0]
        for j in range(R, 0, -1):
            t = t + (xe[R - j:R - j + n] + xe[R + j:R + j + n]) * half[j]
        a = np.moveaxis(t, 0, axis)
    return a


def photo_blend_host(xhat, recon_uint8, error):
    """NPE.py:218-231 verbatim.  xhat = model.sample_at(Z)[0] (float32 (3,64,64)), recon_uint8 = RECON, error = ERROR
    (float32).  Returns (IM uint8, MASK float64)."""
    RECON = np.asarray(recon_uint8)
    DELTA = np.asarray(xhat, np.float32) - to_tanh(np.float32(RECON))
    MASK = gaussian_filter(np.min([np.mean(np.abs(DELTA), axis=0), np.ones((64, 64))], axis=0), BLEND_SIGMA)
    D = MASK * DELTA + (1 - MASK) * np.asarray(error)
    with np.errstate(invalid="ignore"):
        IM = np.uint8(from_tanh(to_tanh(RECON) + D))     # bare cast, as NPE.py:231: no clipping (out-of-range wraps)
    return IM, MASK


def brush_step(model, Z, box, rgb_uint8, weight=0.05):
    """NPE.paint's latent update (NPE.py:199-209), in the reference's order on a float32 Z:
    grad = dL/dZ * (1 + (x2 - x1));  Z -= weight * grad.
    Z: (10,10) or (1,100) float32; box = (x1, y1, x2, y2) in 64-pixel space; rgb_uint8: (3,64,64) brush colour image."""
    x1, y1, x2, y2 = [int(v) for v in box]
    shape = np.shape(Z)
    z = np.float32(np.reshape(Z, (1, -1)))
    g = np.asarray(model.imgradRGB(x1, y1, x2, y2, np.float32(to_tanh(np.float32(rgb_uint8)))[None], z)[0])
    grad = g * np.float32(1 + (x2 - x1))
    return (z[0] - np.float32(weight) * grad).reshape(shape).astype(np.float32)


def lighten_step(model, Z, box, weight=0.1, sign=1.0):
    """NPE.scroll (NPE.py:305-314): grad = d mean(patch)/dZ * (1 + (x2 - x1));  Z += sign(event.delta) * weight * grad."""
    x1, y1, x2, y2 = [int(v) for v in box]
    shape = np.shape(Z)
    z = np.float32(np.reshape(Z, (1, -1)))
    grad = np.asarray(model.imgrad(x1, y1, x2, y2, z)[0]) * np.float32(1 + (x2 - x1))
    return (z[0] + np.float32(float(sign) * float(weight)) * grad).reshape(shape).astype(np.float32)


def paint_event(model, Z, box, rgb_uint8, recon_uint8=None, error=None, weight=0.05):
    """The whole body of NPE.paint (NPE.py:199-231) for a float32 Z: brush step, then the sample (sample mode) or the blended
    photo (photo mode, when RECON / ERROR are given).  With the HIP model this is ONE device submission
    (``IAN.brush_step`` -> ian_brush_step); otherwise the composition of the calls above.
    -> (Z_new in Z's shape, image): image = float32 (3,64,64) sample in sample mode, uint8 (3,64,64) IM in photo mode."""
    x1, y1, x2, y2 = [int(v) for v in box]
    shape = np.shape(Z)
    z = np.float32(np.reshape(Z, (1, -1)))
    photo = (recon_uint8, error) if recon_uint8 is not None else None
    if hasattr(model, "brush_step"):
        rgb = np.float32(to_tanh(np.float32(rgb_uint8)))[None]
        if photo is None:
            z_new, x = model.brush_step(x1, y1, x2, y2, z, RGB=rgb, weight=weight)
            return z_new.reshape(shape), x[0]
        z_new, _, im, _ = model.brush_step(x1, y1, x2, y2, z, RGB=rgb, weight=weight, image=False, photo=photo)
        return z_new.reshape(shape), im
    z_new = brush_step(model, z, box, rgb_uint8, weight)
    if photo is None:
        return z_new.reshape(shape), model.sample_at(z_new)[0]
    return z_new.reshape(shape), photo_blend(model, z_new, recon_uint8, error)[0]


def photo_blend(model, Z, recon_uint8, error):
    """NPE.py:218-231: DELTA = G(Z) - to_tanh(RECON); MASK = gaussian_filter(min(mean|DELTA|, 1), 0.7);
    IM = uint8(from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR)).  recon_uint8, error: (3,64,64).
    -> (IM uint8 (3,64,64), MASK float64 (64,64)).  Runs on the device when the model offers it."""
    z = np.float32(np.reshape(Z, (1, -1)))
    if hasattr(model, "photo_blend"):
        return model.photo_blend(z, recon_uint8, error)
    return photo_blend_host(model.sample_at(z)[0], recon_uint8, error)


# ---- full-resolution sessions (ian_sessions_reserve_hires, include/ian.h) ------------------------------------------------
# The reference has no counterpart (NPE.py:152: "This 64 may need to change if the canvas size changes"), so these four functions ARE
# the specification: the device (kernels_session.hip the box mean, kernels_window.hip the render) matches them bit for bit.  s is the pool's integer scale, 1 <= s <= 16; a source
# photo is uint8 (3, 64*s, 64*s).
HIRES_MAX_SCALE = 16


def _hires_scale(s):
    if int(s) != s or not 1 <= int(s) <= HIRES_MAX_SCALE:
        raise ValueError("scale must be an integer in 1..%d, got %r" % (HIRES_MAX_SCALE, s))
    return int(s)


def hires_downsample(src, s):
    """uint8 (3, 64s, 64s) -> uint8 (3,64,64): the exact integer box mean, (sum of the s x s block + (s*s)//2) // (s*s)."""
    s = _hires_scale(s)
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.shape != (3, 64 * s, 64 * s):
        raise ValueError("a source photo at scale %d is uint8 (3,%d,%d), got %s %s" % (s, 64 * s, 64 * s, src.dtype, src.shape))
    total = src.reshape(3, 64, s, 64, s).sum(axis=(2, 4), dtype=np.int64)
    return np.uint8((total + (s * s) // 2) // (s * s))


def edit_field(x, recon_uint8, error, mask):
    """What the photo blend adds to the photo, in tanh units: IM = from_tanh(to_tanh(RECON) + MASK*DELTA + (1-MASK)*ERROR) and
    ERROR = to_tanh(GIM) - to_tanh(RECON) give IM = GIM + 127.5 * MASK*(DELTA - ERROR).  DELTA is the blend's own float32 delta, the
    product is float64 (MASK is the float64 mask photo_blend_host returns), rounded to float32 once.  -> float32 (3,64,64)."""
    DELTA = np.asarray(x, np.float32) - to_tanh(np.float32(np.asarray(recon_uint8)))
    return np.float32(np.asarray(mask, np.float64) * (np.float64(DELTA) - np.float64(np.asarray(error))))


def hires_axis_taps(s, lo, cnt):
    """Bilinear taps of output coordinates Y = lo .. lo+cnt-1 of a 64s-long axis into the 64-long field axis, half-pixel centres,
    in integers: a = 2Y + 1 - s, i0 = floor(a / 2s), k = a - 2s*i0 in [0, 2s), t = float32(k) / float32(2s) (one float32
    division).  -> (clip(i0, 0, 63), clip(i0 + 1, 0, 63), t): the edges are clamped."""
    s = _hires_scale(s)
    Y = np.arange(int(lo), int(lo) + int(cnt), dtype=np.int64)
    a = 2 * Y + 1 - s
    i0 = a // (2 * s)                        # floor division
    k = a - 2 * s * i0
    t = np.float32(k) / np.float32(2 * s)
    return np.clip(i0, 0, 63), np.clip(i0 + 1, 0, 63), t


def hires_render(src, field, kind, s, vx, vy, vw, vh):
    """Window (vx, vy, vw, vh) of the full-resolution picture -> uint8 (3, vh, vw).  float32 throughout, every operation rounded on its
    own (no fma):  per field row  r = A + tx*(B - A)  (A, B = the field at the two column taps);  v = top + ty*(bot - top);
    kind 0 (photo plus edit field)  q = float32(src) + 127.5f*v;   kind 1 (field holds the sample x)  q = 127.5f*(v + 1.0f);
    out = uint8(clip(rint(q), 0, 255)), ties to even.  A zero field returns the source bytes."""
    s = _hires_scale(s)
    S = 64 * s
    vx, vy, vw, vh = int(vx), int(vy), int(vw), int(vh)
    if vw < 1 or vh < 1 or vx < 0 or vy < 0 or vx + vw > S or vy + vh > S:
        raise ValueError("window (%d,%d) + %d x %d outside the %d x %d picture" % (vx, vy, vw, vh, S, S))
    if kind not in (0, 1):
        raise ValueError("kind must be 0 (photo plus field) or 1 (plain sample), got %r" % (kind,))
    F = np.asarray(field, np.float32)
    c0, c1, tx = hires_axis_taps(s, vx, vw)
    r0, r1, ty = hires_axis_taps(s, vy, vh)
    A = F[:, :, c0]
    rows = A + tx * (F[:, :, c1] - A)        # (3,64,vw): a field row's horizontal pass is the same for every output row that taps it
    top = rows[:, r0]
    v = top + ty[None, :, None] * (rows[:, r1] - top)
    if kind == 0:
        q = np.float32(np.asarray(src)[:, vy:vy + vh, vx:vx + vw]) + np.float32(127.5) * v
    else:
        q = np.float32(127.5) * (v + np.float32(1.0))
    assert q.dtype == np.float32
    return np.uint8(np.clip(np.rint(q), 0, 255))


# ---- edge-aware render (ian_sessions_reserve_guide, include/ian.h) -----------------------------------------------------
# Joint bilateral upsampling of the edit field: each of the four bilinear taps is weighted by how close the photo's pixel is to the
# tap's pixel of GIM, the photo's own 64x64 box mean.  These two functions ARE the specification, as hires_* are.
GUIDE_TABLE_LEN = 3 * 255 + 1
GUIDE_FLOOR = np.float32(2.0 ** -24)


def guide_table(sigma):
    """The range weights of the guided render -> float32 (766,): entry d, the sum over the three channels of the absolute byte
    differences, is max(float32(exp(-d^2 / (2 * (3*sigma)^2))), 2^-24) with the exponent in float64; sigma in levels per channel.
    The floor keeps every denominator of hires_render_guided positive and normal."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError("sigma must be a positive number of levels, got %r" % (sigma,))
    d = np.arange(GUIDE_TABLE_LEN, dtype=np.float64)
    return np.maximum(np.float32(np.exp(-(d ** 2) / (2.0 * (3.0 * sigma) ** 2))), GUIDE_FLOOR)


def hires_guide_field(src, gim, field, s, vx, vy, vw, vh, table):
    """The guided sample v of the field over window (vx, vy, vw, vh) -> float32 (3, vh, vw): hires_render_guided's kind 0 up to and
    including the division."""
    s = _hires_scale(s)
    S = 64 * s
    vx, vy, vw, vh = int(vx), int(vy), int(vw), int(vh)
    if vw < 1 or vh < 1 or vx < 0 or vy < 0 or vx + vw > S or vy + vh > S:
        raise ValueError("window (%d,%d) + %d x %d outside the %d x %d picture" % (vx, vy, vw, vh, S, S))
    table = np.asarray(table)
    if table.dtype != np.float32 or table.shape != (GUIDE_TABLE_LEN,):
        raise ValueError("a guide table is float32 (%d,), got %s %s" % (GUIDE_TABLE_LEN, table.dtype, table.shape))
    F = np.asarray(field, np.float32)
    P = np.int32(np.asarray(src)[:, vy:vy + vh, vx:vx + vw])
    G = np.int32(np.asarray(gim))
    c0, c1, tx = hires_axis_taps(s, vx, vw)
    r0, r1, ty = hires_axis_taps(s, vy, vh)
    one = np.float32(1.0)
    den = num = None
    for rr, wy in ((r0, one - ty), (r1, ty)):
        for cc, wx in ((c0, one - tx), (c1, tx)):
            d = np.abs(P - G[:, rr][:, :, cc]).sum(axis=0)                 # (vh, vw), 0..765
            w = (wy[:, None] * wx[None, :]) * table[d]
            t = w[None] * F[:, rr][:, :, cc]
            den, num = (w, t) if den is None else (den + w, num + t)
    v = num / den[None]
    assert v.dtype == np.float32
    return v


def hires_render_guided(src, gim, field, kind, s, vx, vy, vw, vh, table):
    """hires_render with the field's four bilinear taps weighted by the photo (joint bilateral upsampling) -> uint8 (3, vh, vw).
    gim uint8 (3,64,64) is the session's GIM, table = guide_table(sigma).  kind 1 (the field is a sample, there is no photo to guide
    by): exactly hires_render.  kind 0, per output pixel (Y, X), float32 throughout, every operation rounded on its own (no fma):
      (r0, r1, ty), (c0, c1, tx) = hires_axis_taps;  the taps k = 0..3 are (r0,c0), (r0,c1), (r1,c0), (r1,c1);
      s_k = wy*wx, wy in {1.0f - ty, ty}, wx in {1.0f - tx, tx};   d_k = sum_c |int(src[c,Y,X]) - int(gim[c,r_k,c_k])|;
      w_k = s_k * table[d_k]  (the same four weights for the three channels);   den = ((w0 + w1) + w2) + w3;
      num_c = ((w0*f0 + w1*f1) + w2*f2) + w3*f3, f_k = field[c,r_k,c_k];   v = num_c / den  (one division);
      q = float32(src[c,Y,X]) + 127.5f*v;   out = uint8(clip(rint(q), 0, 255)).
    A zero field gives num = 0, v = 0: the source bytes."""
    if kind not in (0, 1):
        raise ValueError("kind must be 0 (photo plus field) or 1 (plain sample), got %r" % (kind,))
    if kind == 1:
        return hires_render(src, field, kind, s, vx, vy, vw, vh)
    v = hires_guide_field(src, gim, field, s, vx, vy, vw, vh, table)
    vx, vy, vw, vh = int(vx), int(vy), int(vw), int(vh)
    q = np.float32(np.asarray(src)[:, vy:vy + vh, vx:vx + vw]) + np.float32(127.5) * v
    assert q.dtype == np.float32
    return np.uint8(np.clip(np.rint(q), 0, 255))


# ---- canvases (ian_sessions_reserve_canvas / ian_canvas_*, include/ian.h) ----------------------------------------------
# A canvas is a whole photo, uint8 (3, H, W); a session is placed on it as a square of 64*s pixels a side at pixel offset (ox, oy), each
# placement with its own scale s.  The reference has no counterpart, so these three functions ARE the specification, as hires_* are:
# float32, every operation rounded on its own, and the device (kernels_session.hip the crop mean, kernels_window.hip the compose)
# matches them bit for bit.
CANVAS_MAX_PLACED = 8
CANVAS_MAX_FEATHER = 16


def _canvas_square(canvas, ox, oy, s):
    s = _hires_scale(s)
    canvas = np.asarray(canvas)
    if canvas.dtype != np.uint8 or canvas.ndim != 3 or canvas.shape[0] != 3:
        raise ValueError("a canvas is uint8 (3,H,W), got %s %s" % (canvas.dtype, canvas.shape))
    if int(ox) != ox or int(oy) != oy:
        raise ValueError("a square's offset is a pair of integers, got (%r,%r)" % (ox, oy))
    ox, oy, S = int(ox), int(oy), 64 * s
    if ox < 0 or oy < 0 or ox + S > canvas.shape[2] or oy + S > canvas.shape[1]:
        raise ValueError("square (%d,%d) + %d outside the %d x %d canvas" % (ox, oy, S, canvas.shape[2], canvas.shape[1]))
    return canvas, ox, oy, s


def canvas_crop_mean(canvas, ox, oy, s):
    """The 64x64 picture a session placed at (ox, oy) with scale s starts from: hires_downsample of canvas[:, oy:oy+64s, ox:ox+64s]."""
    canvas, ox, oy, s = _canvas_square(canvas, ox, oy, s)
    return hires_downsample(np.ascontiguousarray(canvas[:, oy:oy + 64 * s, ox:ox + 64 * s]), s)


def canvas_ramp(s, f, lo, cnt):
    """The feather along one axis of a square of scale s, for square coordinates u = lo .. lo+cnt-1: 1.0f everywhere at f = 0, otherwise
    d = min(u, 64s-1-u) and r = min(1.0f, float32(2d+1) / float32(2*f*s)) (one float32 division).  f is the feather width in field
    pixels, 0..16; r == 1 exactly for f*s <= u <= 64s-1-f*s.  A pixel's weight is ry * rx, one float32 product.  -> float32 (cnt,)"""
    s = _hires_scale(s)
    if int(f) != f or not 0 <= int(f) <= CANVAS_MAX_FEATHER:
        raise ValueError("feather must be an integer in 0..%d, got %r" % (CANVAS_MAX_FEATHER, f))
    f = int(f)
    u = np.arange(int(lo), int(lo) + int(cnt), dtype=np.int64)
    if u.size and (u[0] < 0 or u[-1] > 64 * s - 1):
        raise ValueError("coordinates %d..%d outside the square of %d pixels" % (u[0], u[-1], 64 * s))
    if f == 0:
        return np.ones(u.shape, np.float32)
    d = np.minimum(u, 64 * s - 1 - u)
    return np.minimum(np.float32(1.0), np.float32(2 * d + 1) / np.float32(2 * f * s))


def _canvas_compose(canvas, placed, f, vx, vy, vw, vh, table):
    """The body of canvas_compose (table None; placements of 5 entries) and canvas_compose_guided (placements of 6, GIM last)."""
    canvas = np.asarray(canvas)
    if canvas.dtype != np.uint8 or canvas.ndim != 3 or canvas.shape[0] != 3:
        raise ValueError("a canvas is uint8 (3,H,W), got %s %s" % (canvas.dtype, canvas.shape))
    H, W = canvas.shape[1:]
    vx, vy, vw, vh = int(vx), int(vy), int(vw), int(vh)
    if vw < 1 or vh < 1 or vx < 0 or vy < 0 or vx + vw > W or vy + vh > H:
        raise ValueError("window (%d,%d) + %d x %d outside the %d x %d canvas" % (vx, vy, vw, vh, W, H))
    if len(placed) > CANVAS_MAX_PLACED:
        raise ValueError("a canvas holds at most %d placements, got %d" % (CANVAS_MAX_PLACED, len(placed)))
    acc = np.float32(canvas[:, vy:vy + vh, vx:vx + vw])
    for (ox, oy, s, field, kind, *gim) in placed:
        if len(gim) != (table is not None):
            raise ValueError("a placement is (ox, oy, s, FIELD, kind%s)" % ("" if table is None else ", GIM"))
        _, ox, oy, s = _canvas_square(canvas, ox, oy, s)
        if kind not in (0, 1):
            raise ValueError("kind must be 0 (photo plus field) or 1 (plain sample), got %r" % (kind,))
        S = 64 * s
        x0, x1, y0, y1 = max(vx, ox), min(vx + vw, ox + S), max(vy, oy), min(vy + vh, oy + S)
        if x0 >= x1 or y0 >= y1:
            continue
        F = np.asarray(field, np.float32)
        if table is not None and kind == 0:      # the photo is the stored canvas, never the running acc
            v = hires_guide_field(canvas[:, oy:oy + S, ox:ox + S], gim[0], F, s, x0 - ox, y0 - oy, x1 - x0, y1 - y0, table)
        else:
            c0, c1, tx = hires_axis_taps(s, x0 - ox, x1 - x0)
            r0, r1, ty = hires_axis_taps(s, y0 - oy, y1 - y0)
            A = F[:, :, c0]
            rows = A + tx * (F[:, :, c1] - A)
            top = rows[:, r0]
            v = top + ty[None, :, None] * (rows[:, r1] - top)
        w = canvas_ramp(s, f, y0 - oy, y1 - y0)[:, None] * canvas_ramp(s, f, x0 - ox, x1 - x0)[None, :]
        part = acc[:, y0 - vy:y1 - vy, x0 - vx:x1 - vx]
        if kind == 0:
            new = part + (np.float32(127.5) * v) * w
        else:
            t = np.float32(127.5) * (v + np.float32(1.0))
            new = np.where(w == np.float32(1.0), t, part + (t - part) * w)
        assert new.dtype == np.float32 and w.dtype == np.float32
        acc[:, y0 - vy:y1 - vy, x0 - vx:x1 - vx] = new
    return np.uint8(np.clip(np.rint(acc), 0, 255))


def canvas_compose(canvas, placed, f, vx, vy, vw, vh):
    """Window (vx, vy, vw, vh) of a canvas with its placed sessions' edits on top -> uint8 (3, vh, vw).  placed = [(ox, oy, s, FIELD,
    kind), ...] in ascending session id; FIELD float32 (3,64,64) and kind as ian_session_read gives them.  Per pixel and channel
    acc = float32(canvas byte); then, for every placement whose square covers the pixel, in list order: v = the bilinear sample of
    FIELD at square coordinates (X-ox, Y-oy) with hires_render's expressions in hires_render's order, w = ry * rx (canvas_ramp), and
      kind 0:  acc = acc + (127.5f*v)*w
      kind 1:  t = 127.5f*(v + 1.0f);  acc = t where w == 1.0f, elsewhere acc = acc + (t - acc)*w
    out = uint8(clip(rint(acc), 0, 255)), ties to even.  Zero fields return the canvas bytes; in the core of a lone placement
    (w == 1) the result is hires_render(crop, FIELD, kind, s, ...) byte for byte."""
    return _canvas_compose(canvas, placed, f, vx, vy, vw, vh, None)


def canvas_compose_guided(canvas, placed, f, vx, vy, vw, vh, table):
    """canvas_compose with the edit field guided by the photo (ian_sessions_reserve_edges) -> uint8 (3, vh, vw).
    placed = [(ox, oy, s, FIELD, kind, GIM), ...] in ascending session id, GIM uint8 (3,64,64) as ian_session_read gives it (the box
    mean of the square, canvas_crop_mean); table = guide_table(sigma).  The one change: for a kind 0 placement the sample v at square
    coordinates (X-ox, Y-oy) is hires_guide_field's v, with the STORED canvas byte as the photo's pixel (not the running acc, so
    overlapping placements do not see each other's edits in their range weights); then acc = acc + (127.5f*v)*w as in canvas_compose.
    Kind 1 placements, the feather, the order of the placements and the rounding are canvas_compose's.  Zero fields return the canvas
    bytes; in the core of a lone kind 0 placement (w == 1) the result is hires_render_guided(crop, GIM, FIELD, 0, s, ...) byte for
    byte."""
    table = np.asarray(table)
    if table.dtype != np.float32 or table.shape != (GUIDE_TABLE_LEN,):
        raise ValueError("a guide table is float32 (%d,), got %s %s" % (GUIDE_TABLE_LEN, table.dtype, table.shape))
    return _canvas_compose(canvas, placed, f, vx, vy, vw, vh, table)


# ---- zoomed views (ian_session_zoom / ian_compose_zoom, include/ian.h) ------------------------------------------------
# A view at 1/k is the exact integer box mean of the full-resolution result: the four functions above give the bytes of the source
# window (vx, vy, k*vw, k*vh), rounded to uint8 per pixel, and zoom_box_mean averages whole k x k blocks of them with
# hires_downsample's rounding.  These functions ARE the specification; the device matches them bit for bit without ever writing the
# full-resolution bytes.
ZOOM_MAX = 16


def _zoom(k):
    if int(k) != k or not 1 <= int(k) <= ZOOM_MAX:
        raise ValueError("zoom must be an integer in 1..%d, got %r" % (ZOOM_MAX, k))
    return int(k)


def zoom_box_mean(img_u8, k):
    """uint8 (3, k*vh, k*vw) -> uint8 (3, vh, vw): (sum of the k x k block + (k*k)//2) // (k*k), half rounds up."""
    k = _zoom(k)
    a = np.asarray(img_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[0] != 3 or a.shape[1] % k or a.shape[2] % k or not a.shape[1] or not a.shape[2]:
        raise ValueError("a picture to view at 1/%d is uint8 (3, %d*vh, %d*vw), got %s %s" % (k, k, k, a.dtype, a.shape))
    vh, vw = a.shape[1] // k, a.shape[2] // k
    total = a.reshape(3, vh, k, vw, k).sum(axis=(2, 4), dtype=np.int64)
    return np.uint8((total + (k * k) // 2) // (k * k))


# The pixel formats of a window result (ian_sessions_set_pixels): the id is the index.
PIXEL_FORMATS = ("planar", "rgb", "rgba", "bgra")


def pixel_format_id(fmt):
    """A format's name or id -> its id, 0..3."""
    if isinstance(fmt, str):
        if fmt not in PIXEL_FORMATS:
            raise ValueError("a pixel format is one of %s, got %r" % (", ".join(PIXEL_FORMATS), fmt))
        return PIXEL_FORMATS.index(fmt)
    if isinstance(fmt, (bool, float)) or int(fmt) != fmt or not 0 <= int(fmt) < len(PIXEL_FORMATS):
        raise ValueError("a pixel format is 0..%d or one of %s, got %r" % (len(PIXEL_FORMATS) - 1, ", ".join(PIXEL_FORMATS), fmt))
    return int(fmt)


def window_shape(n, vw, vh, fmt):
    """The shape of n windows of vw x vh under a pixel format: (n,3,vh,vw) planar, (n,vh,vw,3) rgb, (n,vh,vw,4) rgba / bgra."""
    f = pixel_format_id(fmt)
    return (n, 3, vh, vw) if f == 0 else (n, vh, vw, 3 if f == 1 else 4)


def pack_window(planar, fmt):
    """The specification of the packed window formats: planar uint8 (...,3,vh,vw), what every window call writes under format 0 ->
    what it writes under fmt.  planar: the array itself; rgb: (...,vh,vw,3); rgba: (...,vh,vw,4) as R, G, B, 255; bgra: as B, G, R,
    255.  Every colour byte is the planar byte of that pixel and channel."""
    f = pixel_format_id(fmt)
    a = np.asarray(planar)
    if a.dtype != np.uint8 or a.ndim < 3 or a.shape[-3] != 3:
        raise ValueError("planar windows are uint8 (...,3,vh,vw), got %s %s" % (a.dtype, a.shape))
    if f == 0:
        return a
    rgb = np.moveaxis(a, -3, -1)
    if f == 1:
        return np.ascontiguousarray(rgb)
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = rgb if f == 2 else rgb[..., ::-1]
    return out


def zoom_window(w, h, k):
    """The largest (vw, vh) a w x h picture shows whole at 1/k: vw % 4 == 0, k*vw <= w, k*vh <= h."""
    k = _zoom(k)
    return (int(w) // k) & ~3, int(h) // k


def hires_render_zoom(src, field, kind, s, vx, vy, vw, vh, k):
    """hires_render of the source window (vx, vy, k*vw, k*vh) at 1/k -> uint8 (3, vh, vw)."""
    k = _zoom(k)
    return zoom_box_mean(hires_render(src, field, kind, s, vx, vy, k * int(vw), k * int(vh)), k)


def hires_render_guided_zoom(src, gim, field, kind, s, vx, vy, vw, vh, k, table):
    """hires_render_guided of the source window (vx, vy, k*vw, k*vh) at 1/k -> uint8 (3, vh, vw)."""
    k = _zoom(k)
    return zoom_box_mean(hires_render_guided(src, gim, field, kind, s, vx, vy, k * int(vw), k * int(vh), table), k)


def canvas_compose_zoom(canvas, placed, f, vx, vy, vw, vh, k):
    """canvas_compose of the source window (vx, vy, k*vw, k*vh) at 1/k -> uint8 (3, vh, vw)."""
    k = _zoom(k)
    return zoom_box_mean(canvas_compose(canvas, placed, f, vx, vy, k * int(vw), k * int(vh)), k)


def canvas_compose_guided_zoom(canvas, placed, f, vx, vy, vw, vh, k, table):
    """canvas_compose_guided of the source window (vx, vy, k*vw, k*vh) at 1/k -> uint8 (3, vh, vw)."""
    k = _zoom(k)
    return zoom_box_mean(canvas_compose_guided(canvas, placed, f, vx, vy, k * int(vw), k * int(vh), table), k)


# ---- oriented placements (ian_place_oriented, include/ian.h) -----------------------------------------------------------
# A placement as a similarity transform: the square's centre (cx2, cy2) in half pixels of the canvas (pixel X covers [X, X+1), its
# centre is 2X+1), and A = (ax, ay), the canvas displacement per field pixel along the field's x axis in Q16; the field's y axis is
# B = (-ay, ax).  L2 = ax*ax + ay*ay in [2^32, 2^40] is a step of 1..16 canvas pixels, a side of 64..1024.  The geometry is all
# integers (Python ints / int64 here), so these functions ARE the specification and the device matches them bit for bit;
# oriented_placement is the only place a float touches it.
ORIENTED_L2_MIN, ORIENTED_L2_MAX = 1 << 32, 1 << 40


def oriented_placement(cx, cy, side, angle_deg):
    """A centre in canvas pixels, a side in pixels and an angle in degrees -> (cx2, cy2, ax, ay)."""
    a = np.deg2rad(float(angle_deg))
    step = float(side) / 64.0
    return (int(round(2.0 * float(cx))), int(round(2.0 * float(cy))), int(round(step * np.cos(a) * 65536.0)),
            int(round(step * np.sin(a) * 65536.0)))


def _oriented_ints(*v):
    out = []
    for x in v:
        if int(x) != x or not -2 ** 31 <= int(x) < 2 ** 31:
            raise ValueError("an oriented placement is (cx2, cy2, ax, ay), all int32, got %r" % (v,))
        out.append(int(x))
    return out


def oriented_derive(ax, ay):
    """-> (m, bx, by).  m in 0..4 is the smallest with 2^(32+2m) >= L2: the gather takes n = 2^m samples per field pixel per axis.
    (bx, by) = round(A * 2^36 / L2), field pixels per canvas pixel in Q20, by floor division: floor((2*a*2^36 + L2) / (2*L2))."""
    ax, ay = _oriented_ints(ax, ay)
    L2 = ax * ax + ay * ay
    if not ORIENTED_L2_MIN <= L2 <= ORIENTED_L2_MAX:
        raise ValueError("ax*ax + ay*ay = %d outside 2^32..2^40 (a side of 64..1024 pixels)" % L2)
    m = next(k for k in range(5) if (1 << (32 + 2 * k)) >= L2)
    return m, ((ax << 37) + L2) // (2 * L2), ((ay << 37) + L2) // (2 * L2)


def _oriented_sample(c2, m, d):
    return ((c2 << (16 + m)) + d) >> (17 + m)


def oriented_inside(w, h, cx2, cy2, ax, ay):
    """Whether every sample of canvas_crop_mean_oriented lies on a w x h canvas.  The sample coordinates are monotone in (U, V), so
    the four corner samples decide."""
    cx2, cy2, ax, ay = _oriented_ints(cx2, cy2, ax, ay)
    m = oriented_derive(ax, ay)[0]
    e = (64 << m) - 1
    for U in (-e, e):
        for V in (-e, e):
            X, Y = _oriented_sample(cx2, m, U * ax - V * ay), _oriented_sample(cy2, m, U * ay + V * ax)
            if not (0 <= X < int(w) and 0 <= Y < int(h)):
                return False
    return True


def oriented_bbox(cx2, cy2, ax, ay):
    """-> (x0, y0, x1, y1), inclusive pixel bounds that contain every pixel canvas_compose_oriented can change: the square's half
    extent along either axis is 32 * (|ax| + |ay|) / 65536 pixels, rounded up to half pixels, plus one pixel for the rounding of
    (bx, by)."""
    cx2, cy2, ax, ay = _oriented_ints(cx2, cy2, ax, ay)
    h2 = (abs(ax) + abs(ay) + 1023) >> 10
    return ((cx2 - h2) >> 1) - 1, ((cy2 - h2) >> 1) - 1, ((cx2 + h2) >> 1) + 1, ((cy2 + h2) >> 1) + 1


def canvas_crop_mean_oriented(canvas, cx2, cy2, ax, ay):
    """The 64x64 picture a session placed at (cx2, cy2, ax, ay) starts from -> uint8 (3,64,64).  Sub-sample k = 0 .. 64n-1 of an axis
    has U = 2k + 1 - 64n (rows: V); DX = U*ax - V*ay, DY = U*ay + V*ax; the sample is canvas pixel
    X = ((cx2 << (16+m)) + DX) >> (17+m), Y likewise (arithmetic shifts), and GIM = (sum of the n*n bytes + n*n/2) // (n*n)."""
    canvas = np.asarray(canvas)
    if canvas.dtype != np.uint8 or canvas.ndim != 3 or canvas.shape[0] != 3:
        raise ValueError("a canvas is uint8 (3,H,W), got %s %s" % (canvas.dtype, canvas.shape))
    cx2, cy2, ax, ay = _oriented_ints(cx2, cy2, ax, ay)
    m = oriented_derive(ax, ay)[0]
    if not oriented_inside(canvas.shape[2], canvas.shape[1], cx2, cy2, ax, ay):
        raise ValueError("square (%d,%d,%d,%d) samples outside the %d x %d canvas" % (cx2, cy2, ax, ay, canvas.shape[2], canvas.shape[1]))
    n = 1 << m
    U = (2 * np.arange(64 * n, dtype=np.int64) + 1 - 64 * n)[None, :]
    V = U.T
    X = ((cx2 << (16 + m)) + U * ax - V * ay) >> (17 + m)
    Y = ((cy2 << (16 + m)) + U * ay + V * ax) >> (17 + m)
    total = canvas[:, Y, X].reshape(3, 64, n, 64, n).sum(axis=(2, 4), dtype=np.int64)
    return np.uint8((total + (n * n) // 2) // (n * n))


def _oriented_taps(Q):
    a = Q + (1 << 26) - (1 << 20)
    i0 = a >> 21
    t = np.float32(a & ((1 << 21) - 1)) / np.float32(1 << 21)
    return np.clip(i0, 0, 63), np.clip(i0 + 1, 0, 63), t


def _oriented_ramp(Q, f):
    if f == 0:
        return np.ones(Q.shape, np.float32)
    d = np.minimum(Q + (1 << 26), (1 << 26) - Q) >> 5
    return np.minimum(np.float32(1.0), np.float32(d) / np.float32(f << 16))


def canvas_compose_oriented(canvas, placed, f, vx, vy, vw, vh):
    """canvas_compose for oriented placements -> uint8 (3, vh, vw).  placed = [(cx2, cy2, ax, ay, FIELD, kind), ...] in ascending
    session id.  Per pixel (X, Y) and placement: dx = 2X+1-cx2, dy = 2Y+1-cy2, Uq = dx*bx + dy*by (u - 32 in Q21),
    Vq = dy*bx - dx*by; the pixel is inside when -2^26 <= Uq, Vq < 2^26.  Taps along an axis: a = Q + 2^26 - 2^20, i0 = a >> 21,
    t = float32(a & (2^21-1)) / float32(2^21), both taps clamped to 0..63; the sample is hires_render's bilinear expression.  The
    ramp is 1.0f at f == 0, otherwise d = min(Q + 2^26, 2^26 - Q) >> 5 and r = min(1.0f, float32(d) / float32(f << 16));
    w = r(Vq) * r(Uq).  Kinds, order and rounding are canvas_compose's."""
    canvas = np.asarray(canvas)
    if canvas.dtype != np.uint8 or canvas.ndim != 3 or canvas.shape[0] != 3:
        raise ValueError("a canvas is uint8 (3,H,W), got %s %s" % (canvas.dtype, canvas.shape))
    H, W = canvas.shape[1:]
    vx, vy, vw, vh = int(vx), int(vy), int(vw), int(vh)
    if vw < 1 or vh < 1 or vx < 0 or vy < 0 or vx + vw > W or vy + vh > H:
        raise ValueError("window (%d,%d) + %d x %d outside the %d x %d canvas" % (vx, vy, vw, vh, W, H))
    if len(placed) > CANVAS_MAX_PLACED:
        raise ValueError("a canvas holds at most %d placements, got %d" % (CANVAS_MAX_PLACED, len(placed)))
    if int(f) != f or not 0 <= int(f) <= CANVAS_MAX_FEATHER:
        raise ValueError("feather must be an integer in 0..%d, got %r" % (CANVAS_MAX_FEATHER, f))
    f = int(f)
    acc = np.float32(canvas[:, vy:vy + vh, vx:vx + vw])
    Xc = (2 * np.arange(vx, vx + vw, dtype=np.int64) + 1)[None, :]
    Yc = (2 * np.arange(vy, vy + vh, dtype=np.int64) + 1)[:, None]
    for (cx2, cy2, ax, ay, field, kind) in placed:
        cx2, cy2, ax, ay = _oriented_ints(cx2, cy2, ax, ay)
        _, bx, by = oriented_derive(ax, ay)
        if kind not in (0, 1):
            raise ValueError("kind must be 0 (photo plus field) or 1 (plain sample), got %r" % (kind,))
        dx, dy = Xc - cx2, Yc - cy2
        Uq, Vq = dx * bx + dy * by, dy * bx - dx * by
        lim = 1 << 26
        inside = (Uq >= -lim) & (Uq < lim) & (Vq >= -lim) & (Vq < lim)
        if not inside.any():
            continue
        Uq, Vq = np.where(inside, Uq, 0), np.where(inside, Vq, 0)
        F = np.asarray(field, np.float32)
        c0, c1, tx = _oriented_taps(Uq)
        r0, r1, ty = _oriented_taps(Vq)
        top = F[:, r0, c0] + tx * (F[:, r0, c1] - F[:, r0, c0])
        bot = F[:, r1, c0] + tx * (F[:, r1, c1] - F[:, r1, c0])
        v = top + ty * (bot - top)
        w = _oriented_ramp(Vq, f) * _oriented_ramp(Uq, f)
        if kind == 0:
            new = acc + (np.float32(127.5) * v) * w
        else:
            t = np.float32(127.5) * (v + np.float32(1.0))
            new = np.where(w == np.float32(1.0), t, acc + (t - acc) * w)
        assert new.dtype == np.float32 and w.dtype == np.float32
        acc = np.where(inside[None], new, acc)
    return np.uint8(np.clip(np.rint(acc), 0, 255))


def canvas_compose_oriented_zoom(canvas, placed, f, vx, vy, vw, vh, k):
    """canvas_compose_oriented of the source window (vx, vy, k*vw, k*vh) at 1/k -> uint8 (3, vh, vw)."""
    k = _zoom(k)
    return zoom_box_mean(canvas_compose_oriented(canvas, placed, f, vx, vy, k * int(vw), k * int(vh)), k)


# ---- local edits (ian_sessions_reserve_local / ian_session_local, include/ian.h) -------------------------------------
# NPE.py declares USER_MASK "currently not implemented" (NPE.py:58-59, :221), offers gk (NPE.py:167-175) for "changes to MASK ... more
# localized to the brush location" and dampen (NPE.py:184-189) as a commented-out alternative for D (NPE.py:227, :298).  These four
# functions ARE the specification of what the sessions make of them: float64, every operation rounded on its own, and the device
# (kernels_session.hip, npe_blend.h) matches them bit for bit.
LOCAL_SIGMA = 0.3         # NPE.py:170
LOCAL_IM = 64             # NPE.py:171
DAMPEN_THRESH = 0.75      # NPE.py:187


def local_falloff_table(sigma=LOCAL_SIGMA, im=LOCAL_IM):
    """f64[64]: t[d] = exp(-(d**2 / float(im)) / (2 * sigma**2)), the falloff at d pixels from the brush rectangle along one axis;
    t[0] == 1.0.  The host computes it (as it computes the blend's Gaussian); the device only multiplies two of its entries."""
    d = np.arange(64)
    return np.exp(-(d ** 2 / float(im)) / (2 * sigma ** 2))


def _axis_distance(lo, hi):
    """gk's distance of pixel j to the half-open interval [lo, hi): lo - j before it, 0 inside, j - hi + 1 after it."""
    j = np.arange(64)
    return np.where(j < lo, lo - j, np.where(j >= hi, j - hi + 1, 0))


def local_footprint(c1, r1, c2, r2, t):
    """f64[64,64]: F = t[dy][:,None] * t[dx][None,:] (one float64 product per pixel) on gk's distance grids: 1.0 inside the brush
    rectangle, falling off with the distance to it.  gk takes exp of the SUM of the two exponents; the separable form differs from
    it by rounding only.  The rectangle must not be empty (0 <= c1 < c2 <= 64, 0 <= r1 < r2 <= 64)."""
    c1, r1, c2, r2 = int(c1), int(r1), int(c2), int(r2)
    if not (0 <= c1 < c2 <= 64 and 0 <= r1 < r2 <= 64):
        raise ValueError("a footprint needs a non-empty rectangle inside the 64x64 image, got (%d,%d,%d,%d)" % (c1, r1, c2, r2))
    t = np.asarray(t, np.float64)
    return t[_axis_distance(r1, r2)][:, None] * t[_axis_distance(c1, c2)][None, :]


def umask_paint(U, box, t):
    """USER_MASK after a stroke: np.maximum(U, local_footprint(box)).  Exact and idempotent, and the result of several strokes does
    not depend on their order.  An empty rectangle (c2 <= c1 or r2 <= r1) leaves U as it is."""
    c1, r1, c2, r2 = [int(v) for v in box]
    U = np.asarray(U, np.float64)
    if c2 <= c1 or r2 <= r1:
        return U.copy()
    return np.maximum(U, local_footprint(c1, r1, c2, r2, t))


def brush_rect(x, y, d):
    """move_mouse's brush rectangle (NPE.py:148-156) for a point (x, y) that is already in 64-pixel space and the brush-size slider's
    value d -> (c1, r1, c2, r2): brush_width = d//4 + 1 pixels a side, centred on the point and pushed back inside the image.  The //4
    of NPE.py:148 (canvas to image) and of :202 (the rectangle read back from the canvas, exact: its corners are multiples of 4) stay
    with the caller."""
    x, y, d = int(x), int(y), int(d)
    brush_width = (d // 4) + 1
    xmin = max(min(x - brush_width // 2, 64 - brush_width), 0)
    ymin = max(min(y - brush_width // 2, 64 - brush_width), 0)
    return xmin, ymin, xmin + brush_width, ymin + brush_width


# ---- brush tips (ian_sessions_set_tip, ian_session_brush_tip) -------------------------------------------------------
# A tip is a weight image [th][tw]; the library takes the weights as given, and what a brush shape means as a loss is decided here.
def tip_weights(w):
    """A brush shape w [th][tw] (weights >= 0, not all zero) -> the float32 weights of ian_sessions_set_tip, normalised so that they
    sum to 1/3 (times three channels: a weighted MEAN, as the rectangle's 1/N is): float32(w) * (float32(1) / float32(3 * S)), S the
    float64 sum of w.  For w == 1 that is 1.f / (float)(3 * th * tw), the rectangle brush's own factor, bit for bit."""
    w = np.asarray(w)
    if w.ndim != 2 or not 1 <= w.shape[0] <= 64 or not 1 <= w.shape[1] <= 64:
        raise ValueError("a tip has shape (th, tw) with both sides 1..64, got %s" % (w.shape,))
    w64 = w.astype(np.float64)
    if not np.all(np.isfinite(w64)) or np.any(w64 < 0):
        raise ValueError("the weights of a tip are finite and >= 0")
    S = float(w64.sum())
    if not S > 0:
        raise ValueError("a tip that is all zero has no normalisation (pass it with normalise=False for a zero gradient)")
    return (w.astype(np.float32) * (np.float32(1) / np.float32(3 * S))).astype(np.float32)


def tip_rect(x, y, tw, th):
    """The rectangle of a tw x th tip at the mouse position (x, y) in 64-pixel space -> (c1, r1, c2, r2): placed as move_mouse places
    its square (NPE.py:148-156, brush_rect), centred on the point and pushed back inside the image."""
    x, y, tw, th = int(x), int(y), int(tw), int(th)
    if not (1 <= tw <= 64 and 1 <= th <= 64):
        raise ValueError("a tip has both sides 1..64, got %d x %d" % (tw, th))
    xmin = max(min(x - tw // 2, 64 - tw), 0)
    ymin = max(min(y - th // 2, 64 - th), 0)
    return xmin, ymin, xmin + tw, ymin + th


def round_tip(diameter, hardness=0.5):
    """A round brush of `diameter` pixels (1..64) with a soft edge -> float32 (diameter, diameter), un-normalised: weight 1 out to
    hardness * R from the centre, falling smoothly (smoothstep: zero slope at both ends) to 0 at R = diameter / 2; a pixel is taken at
    its centre.  Built in float64.  hardness in [0, 1]; 1 is a hard disc."""
    D, hd = int(diameter), float(hardness)
    if not 1 <= D <= 64:
        raise ValueError("diameter %r outside 1..64" % (diameter,))
    if not 0.0 <= hd <= 1.0:
        raise ValueError("hardness %r outside [0, 1]" % (hardness,))
    R = D / 2.0
    o = np.arange(D, dtype=np.float64) + 0.5 - R         # pixel centres, symmetric about 0
    d2 = o[:, None] ** 2 + o[None, :] ** 2               # the same sum in every one of the square's eight symmetries
    r = np.sqrt(d2)
    r0 = hd * R
    if r0 < R:
        t = np.clip((R - r) / (R - r0), 0.0, 1.0)
        w = t * t * (3.0 - 2.0 * t)
    else:
        w = (r < R).astype(np.float64)
    w[r <= r0] = 1.0
    return w.astype(np.float32)


def tip_seed(xhat, box, wn, rgb=None, mode=1):
    """The loss seed of one tip event, operation by operation what the seed kernels compute (kernels_brush.hip, SEED_TIP) -> float32
    (3,H,W): inside box = (c1, r1, c2, r2), whose size is wn's, mode 1 gives 2.f * (xhat - rgb[co]) * wn[r - r1][c - c1] (float32:
    the difference rounded, then each product) and mode 0 gives wn[r - r1][c - c1]; zero outside.  The three channels share wn."""
    xhat = np.asarray(xhat, np.float32)
    wn = np.asarray(wn, np.float32)
    c1, r1, c2, r2 = [int(v) for v in box]
    if xhat.ndim != 3 or wn.shape != (r2 - r1, c2 - c1):
        raise ValueError("the box (%d,%d,%d,%d) is not the tip's %s" % (c1, r1, c2, r2, wn.shape))
    g = np.zeros_like(xhat)
    if int(mode) == 0:
        g[:, r1:r2, c1:c2] = wn[None]
        return g
    t = np.asarray(rgb, np.float32).reshape(-1, 1, 1)
    d = (xhat[:, r1:r2, c1:c2] - t).astype(np.float32)
    g[:, r1:r2, c1:c2] = ((np.float32(2) * d).astype(np.float32) * wn[None]).astype(np.float32)
    return g


def clone_tip_seed(xhat, box, wn, target):
    """The loss seed of one weighted clone event, operation by operation what the seed kernels compute (kernels_brush.hip,
    SEED_CLONE_TIP) -> float32 (3,H,W): tip_seed's mode 1 with a target image (clone_target of the source) in the place of the colour:
    inside box = (c1, r1, c2, r2), whose size is wn's, 2.f * (xhat - target) * wn[r - r1][c - c1] (float32: the difference rounded,
    then each product); zero outside."""
    xhat = np.asarray(xhat, np.float32)
    wn = np.asarray(wn, np.float32)
    target = np.asarray(target, np.float32)
    c1, r1, c2, r2 = [int(v) for v in box]
    if xhat.ndim != 3 or wn.shape != (r2 - r1, c2 - c1):
        raise ValueError("the box (%d,%d,%d,%d) is not the tip's %s" % (c1, r1, c2, r2, wn.shape))
    if target.shape != xhat.shape:
        raise ValueError("the target %s is not the image's %s" % (target.shape, xhat.shape))
    g = np.zeros_like(xhat)
    d = (xhat[:, r1:r2, c1:c2] - target[:, r1:r2, c1:c2]).astype(np.float32)
    g[:, r1:r2, c1:c2] = ((np.float32(2) * d).astype(np.float32) * wn[None]).astype(np.float32)
    return g


def tip_footprint(wn, c1, r1, t):
    """f64[64,64]: the footprint a tip wn [th][tw] placed at (c1, r1) leaves in the user mask (ian_sessions_set_soft_mask): the
    tip's shape s = float64(wn) / float64(max wn) spread by the falloff table t,
        R[qy, x] = max_qx s[qy, qx] * t[|x - (c1 + qx)|]        F[y, x] = max_qy t[|y - (r1 + qy)|] * R[qy, x]
    one float64 division per tip pixel and one float64 product per term.  All zeros for an all-zero tip.  For an all-ones tip it is
    local_footprint of the rectangle, bit for bit; for any other it is <= that everywhere, and 1.0 where wn has its maximum."""
    wn = np.asarray(wn)
    c1, r1 = int(c1), int(r1)
    if wn.ndim != 2 or not (1 <= wn.shape[0] <= 64 and 1 <= wn.shape[1] <= 64):
        raise ValueError("a tip has shape (th, tw) with both sides 1..64, got %s" % (wn.shape,))
    th, tw = wn.shape
    if not (0 <= c1 and c1 + tw <= 64 and 0 <= r1 and r1 + th <= 64):
        raise ValueError("a %d x %d tip at (%d,%d) leaves the 64x64 image" % (tw, th, c1, r1))
    t = np.asarray(t, np.float64)
    w = wn.astype(np.float64)
    m = float(w.max())
    if not m > 0:
        return np.zeros((64, 64), np.float64)
    s = w / m
    j = np.arange(64)
    tx = t[np.abs(j[None, :] - (c1 + np.arange(tw))[:, None])]       # [qx, x]
    ty = t[np.abs(j[:, None] - (r1 + np.arange(th))[None, :])]       # [y, qy]
    R = (s[:, :, None] * tx[None, :, :]).max(axis=1)                 # [qy, x]
    return (ty[:, :, None] * R[None, :, :]).max(axis=1)              # [y, x]


def umask_paint_tip(U, wn, c1, r1, t):
    """USER_MASK after a tipped paint event under ian_sessions_set_soft_mask: np.maximum(U, tip_footprint(wn, c1, r1, t)).  Exact
    and idempotent like umask_paint, and the result of several points does not depend on their order."""
    return np.maximum(np.asarray(U, np.float64), tip_footprint(wn, c1, r1, t))


def stroke_footprint(U, boxes, t):
    """USER_MASK after a whole stroke (ian_session_stroke): umask_paint for every rectangle of boxes (K,4), in sequence.  np.maximum is
    exact, so the order of the rectangles does not matter and a rectangle given twice adds nothing."""
    U = np.array(U, np.float64)
    for box in np.asarray(boxes).reshape(-1, 4):
        U = umask_paint(U, box, t)
    return U


def clone_target(picture_u8, box, offset=(0, 0)):
    """The target image of one clone event (ian_session_clone) as a stateless call would be given it -> float32 (3,64,64):
    T[:, r, c] = np.asarray(to_tanh(picture[:, r + dr, c + dc]), dtype=np.float32) for (r, c) inside box = (c1, r1, c2, r2), zero
    elsewhere (the loss never reads there); offset = (dc, dr).  picture_u8 is the source session's GIM, IM or RECON, uint8 (3,64,64).
    An empty rectangle gives all zeros; a non-empty one must lie inside the image, and so must its shifted copy."""
    p = np.asarray(picture_u8)
    if p.dtype != np.uint8 or p.shape != (3, 64, 64):
        raise ValueError("a source picture is uint8 (3,64,64), got %s %s" % (p.dtype, p.shape))
    c1, r1, c2, r2 = [int(v) for v in box]
    dc, dr = [int(v) for v in offset]
    T = np.zeros((3, 64, 64), np.float32)
    if c2 <= c1 or r2 <= r1:
        return T
    if c1 < 0 or r1 < 0 or c2 > 64 or r2 > 64:
        raise ValueError("patch (%d,%d,%d,%d) outside the 64x64 image" % (c1, r1, c2, r2))
    if c1 + dc < 0 or c2 + dc > 64 or r1 + dr < 0 or r2 + dr > 64:
        raise ValueError("patch (%d,%d,%d,%d) shifted by (%d,%d) leaves the 64x64 image" % (c1, r1, c2, r2, dc, dr))
    T[:, r1:r2, c1:c2] = np.asarray(to_tanh(p[:, r1 + dr:r2 + dr, c1 + dc:c2 + dc]), dtype=np.float32)   # float64, one rounding: NPE.py:257
    return T


def photo_blend_local(xhat, recon_uint8, error, U=None, half=None, dampen=False, thresh=DAMPEN_THRESH):
    """photo_blend_host with the user mask and / or dampen -> (IM uint8, MASK_L float64, FIELD float32).
      MASK    exactly photo_blend_host's (half = gaussian_half_kernel(...): the same filter through separable_reflect_filter, which
              equals scipy's bit for bit; None: scipy's own with BLEND_SIGMA)
      MASK_L  = MASK * U (U float64 (64,64)), or MASK when U is None
      D       = MASK_L*DELTA + (1-MASK_L)*ERROR
      dampen  (NPE.py:184-189): t32 = to_tanh(float32(RECON)); s = float64(t32) + D; D = where(s > thresh, thresh - float64(t32), D)
      IM      = uint8(from_tanh(to_tanh(RECON) + D))
      FIELD   = float32(MASK_L * (float64(DELTA) - float64(ERROR))) (edit_field with MASK_L); with dampen float32(D - float64(ERROR))"""
    RECON = np.asarray(recon_uint8)
    ERROR = np.asarray(error)
    t32 = to_tanh(np.float32(RECON))
    DELTA = np.asarray(xhat, np.float32) - t32
    m = np.min([np.mean(np.abs(DELTA), axis=0), np.ones((64, 64))], axis=0)
    MASK = gaussian_filter(m, BLEND_SIGMA) if half is None else separable_reflect_filter(m, np.asarray(half, np.float64))
    MASK_L = MASK if U is None else MASK * np.asarray(U, np.float64)
    D = MASK_L * DELTA + (1 - MASK_L) * ERROR
    if dampen:
        s = np.float64(t32) + D
        D = np.where(s > thresh, thresh - np.float64(t32), D)
        FIELD = np.float32(D - np.float64(ERROR))
    else:
        FIELD = np.float32(MASK_L * (np.float64(DELTA) - np.float64(ERROR)))
    with np.errstate(invalid="ignore"):
        IM = np.uint8(from_tanh(to_tanh(RECON) + D))
    return IM, MASK_L, FIELD


# ---- undo history of an edit session (ian_session_mark / ian_session_undo, include/ian.h) -----------------------------
# No arithmetic: the bookkeeping of which saved state is where.  csrc/ian_session_history.h is the same specification in C++; the two
# return the same physical slots for the same operations.
class SessionHistory:
    """One session's history: saved states E[0..len-1], a cursor c (0 <= c <= len; c == len: the live state is not in the list,
    c < len: it is E[c]) in a ring of depth + 1 physical slots, entry k in slot (base + k) % (depth + 1).  Every method returns the
    physical slots to save the live state into / to load it from; what a slot holds is the caller's.
    c == len implies len <= depth, c < len implies len <= depth + 1: at most `depth` steps can be undone, and the slot beyond them
    holds the tip that the first undo saves."""

    def __init__(self, depth):
        depth = int(depth)
        if not 1 <= depth <= 64:
            raise ValueError("depth must be in 1..64, got %d" % depth)
        self.depth = depth
        self.base = self.len = self.cur = 0

    def _slot(self, k):
        return (self.base + k) % (self.depth + 1)

    def _drop_oldest(self):
        self.base = (self.base + 1) % (self.depth + 1)
        self.len -= 1
        self.cur = max(self.cur - 1, 0)

    @property
    def undoable(self):
        return self.cur

    @property
    def redoable(self):
        return self.len - 1 - self.cur if self.cur < self.len else 0

    def mark(self):
        """A stroke begins: the redo tail goes, the oldest entry too when the list is full -> the slot to save the live state into."""
        if self.cur < self.len:
            self.len = self.cur
        if self.len == self.depth:
            self.cur = self.len
            self._drop_oldest()
        slot = self._slot(self.len)
        self.len += 1
        self.cur = self.len
        return slot

    def undo(self, k=1):
        """-> (the slot to save the tip into first, or -1; the slot to load)."""
        k = int(k)
        if not 1 <= k <= self.undoable:
            raise ValueError("%d undo steps asked, %d available" % (k, self.undoable))
        save = -1
        if self.cur == self.len:
            save = self._slot(self.len)
            self.len += 1
        self.cur -= k
        return save, self._slot(self.cur)

    def redo(self, k=1):
        """-> the slot to load."""
        k = int(k)
        if not 1 <= k <= self.redoable:
            raise ValueError("%d redo steps asked, %d available" % (k, self.redoable))
        self.cur += k
        return self._slot(self.cur)

    def edited(self):
        """The latent was written by something other than undo / redo: the redo tail goes, the state the user came back to stays an
        undo target (the oldest entry goes when that makes depth + 1 of them)."""
        if self.cur >= self.len:
            return
        self.len = self.cur + 1
        self.cur = self.len
        if self.len > self.depth:
            self._drop_oldest()

    def clear(self):
        self.base = self.len = self.cur = 0


# ---- saved edit sessions (ian_session_save / ian_session_load): the record, byte for byte, in numpy ---------------------
SESSION_RECORD_MAGIC = 0x534E4149      # "IANS"
SESSION_RECORD_FORMAT = 1
# ian_session_meta (include/ian.h): 64 bytes
SESSION_META_DTYPE = np.dtype([("magic", "<u4"), ("format", "<i4"), ("num_latents", "<i4"), ("scale", "<i4"), ("local", "<i4"),
                               ("depth", "<i4"), ("has_source", "<i4"), ("local_flags", "<i4"), ("hist_len", "<i4"), ("hist_cur", "<i4"),
                               ("body_bytes", "<i8"), ("reserved", "<i4", (4,))])


def session_record_columns(zl, scale=0, local=False, depth=0):
    """The arrays of one record's body, in order: [(name, dtype, shape)].  The 64x64 state always; SOURCE (3, S, S), S = 64 * scale,
    FIELD and FIELD_KIND with a full-resolution reservation; UMASK and LOCAL with the local one; with a history of `depth` the ring
    of depth + 1 saved Z rows and, when local, of as many UMASK rows."""
    zl, scale, depth = int(zl), int(scale), int(depth)
    if zl < 1 or not 0 <= scale <= 16 or not 0 <= depth <= 64:
        raise ValueError("a layout has zl >= 1, scale 0..16, depth 0..64, got %d, %d, %d" % (zl, scale, depth))
    cols = [("GIM", np.uint8, (3, 64, 64)), ("IM", np.uint8, (3, 64, 64)), ("RECON", np.uint8, (3, 64, 64)),
            ("ERROR", np.float32, (3, 64, 64)), ("Z", np.float32, (zl,)), ("MODE", np.int32, (1,))]
    if scale:
        cols += [("SOURCE", np.uint8, (3, 64 * scale, 64 * scale)), ("FIELD", np.float32, (3, 64, 64)), ("FIELD_KIND", np.int32, (1,))]
    if local:
        cols += [("UMASK", np.float64, (64, 64)), ("LOCAL", np.int32, (1,))]
    if depth:
        cols.append(("HIST_Z", np.float32, (depth + 1, zl)))
        if local:
            cols.append(("HIST_UMASK", np.float64, (depth + 1, 64, 64)))
    return cols


def session_record_layout(zl, scale=0, local=False, depth=0):
    """-> ({name: byte offset in the body}, in body order, and body_bytes): every array starts at a multiple of 16 bytes."""
    offsets, at = {}, 0
    for name, dtype, shape in session_record_columns(zl, scale, local, depth):
        offsets[name] = at
        at += -(-int(np.prod(shape)) * np.dtype(dtype).itemsize // 16) * 16
    return offsets, at


def session_meta(zl, scale=0, local=False, depth=0, has_source=0, local_flags=0, hist_len=0, hist_cur=0):
    """One ian_session_meta as a 0-d structured array."""
    m = np.zeros((), SESSION_META_DTYPE)
    m["magic"], m["format"] = SESSION_RECORD_MAGIC, SESSION_RECORD_FORMAT
    m["num_latents"], m["scale"], m["local"], m["depth"] = int(zl), int(scale), int(bool(local)), int(depth)
    m["has_source"], m["local_flags"], m["hist_len"], m["hist_cur"] = int(has_source), int(local_flags), int(hist_len), int(hist_cur)
    m["body_bytes"] = session_record_layout(zl, scale, local, depth)[1]
    return m


def check_session_meta(meta, zl, scale=0, local=False, depth=0):
    """A record's meta against the layout it is to be loaded into -> None, or the name of the first field that is refused
    (csrc/ian_session_record.h, session_record_check, in its order)."""
    g = lambda k: int(meta[k])
    local, depth = int(bool(local)), int(depth)
    if g("magic") != SESSION_RECORD_MAGIC:
        return "magic"
    if g("format") != SESSION_RECORD_FORMAT:
        return "format"
    want = {"num_latents": int(zl), "scale": int(scale), "local": local, "depth": depth,
            "body_bytes": session_record_layout(zl, scale, local, depth)[1]}
    for k in ("num_latents", "scale", "local", "depth", "body_bytes"):
        if g(k) != want[k]:
            return k
    if not 0 <= g("local_flags") <= 3 or (g("local_flags") and not local):
        return "local_flags"
    if g("has_source") not in (0, 1) or (g("has_source") and not scale):
        return "has_source"
    ln, cur = g("hist_len"), g("hist_cur")
    if ln < 0:
        return "hist_len"
    if not 0 <= cur <= ln:
        return "hist_cur"
    if (depth == 0 and ln) or (cur == ln and ln > depth) or ln > depth + 1:
        return "hist_len"
    if any(int(v) for v in np.asarray(meta["reserved"]).reshape(-1)):
        return "reserved"
    return None


def session_record_pack(fields, history_entries, zl, scale=0, local=False, depth=0, hist_cur=None):
    """One session -> (meta, body uint8 (body_bytes,)), the canonical record.  fields: what EditSessions.read returns (a session without
    a full-resolution source has no "SOURCE": those bytes are zero and has_source is 0); history_entries: the history's entries, oldest
    first, each (Z, UMASK) or Z alone in a layout without the local reservation -- entry k goes to slot k, the other slots are zero;
    hist_cur: the cursor, len(history_entries) (the tip) when not given."""
    offsets, body_bytes = session_record_layout(zl, scale, local, depth)
    body = np.zeros(body_bytes, np.uint8)
    entries = [e if isinstance(e, (tuple, list)) else (e, None) for e in history_entries]
    if len(entries) > (depth + 1 if depth else 0):
        raise ValueError("%d history entries for depth %d" % (len(entries), depth))
    for name, dtype, shape in session_record_columns(zl, scale, local, depth):
        if name == "HIST_Z":
            a = np.zeros(shape, dtype)
            for k, e in enumerate(entries):
                a[k] = np.asarray(e[0], dtype).reshape(shape[1:])
        elif name == "HIST_UMASK":
            a = np.zeros(shape, dtype)
            for k, e in enumerate(entries):
                a[k] = np.asarray(e[1], dtype).reshape(shape[1:])
        elif name == "SOURCE" and fields.get("SOURCE") is None:
            continue
        else:
            a = np.asarray(fields[name], dtype).reshape(shape)
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        body[offsets[name]:offsets[name] + raw.size] = raw
    meta = session_meta(zl, scale, local, depth, has_source=int(fields.get("SOURCE") is not None), local_flags=int(fields.get("LOCAL", 0)),
                        hist_len=len(entries), hist_cur=len(entries) if hist_cur is None else int(hist_cur))
    return meta, body


def session_record_unpack(meta, body):
    """The inverse of session_record_pack -> (fields, history_entries): scalars as ints, "SOURCE" only with has_source, entries as
    (Z, UMASK) or Z alone."""
    zl, scale, local, depth = (int(meta[k]) for k in ("num_latents", "scale", "local", "depth"))
    offsets, body_bytes = session_record_layout(zl, scale, local, depth)
    body = np.ascontiguousarray(body, np.uint8).reshape(-1)
    if body.size != body_bytes or int(meta["body_bytes"]) != body_bytes:
        raise ValueError("the body holds %d bytes, the meta says %d, the layout has %d" % (body.size, int(meta["body_bytes"]), body_bytes))
    fields, ring = {}, {}
    for name, dtype, shape in session_record_columns(zl, scale, local, depth):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = body[offsets[name]:offsets[name] + nbytes].copy().view(dtype).reshape(shape)
        if name.startswith("HIST_"):
            ring[name] = a
        elif name == "SOURCE" and not int(meta["has_source"]):
            continue
        else:
            fields[name] = int(a[0]) if shape == (1,) else a
    entries = []
    for k in range(int(meta["hist_len"])):
        entries.append((ring["HIST_Z"][k], ring["HIST_UMASK"][k]) if "HIST_UMASK" in ring else ring["HIST_Z"][k])
    return fields, entries


# ---- fitting the latent to the photo (ian_session_fit): the optimiser and the loss, operation by operation, in numpy ----
FIT_MAX_STEPS = 512
FIT_BETA1, FIT_BETA2, FIT_EPS = np.float32(0.9), np.float32(0.999), np.float32(1e-8)
FIT_ONE_M_BETA1, FIT_ONE_M_BETA2 = np.float32(0.1), np.float32(0.001)   # the literals 0.1f and 0.001f, not 1 - beta
_FIT_CONSTS = []


def fit_adam_consts(steps):
    """(c1, c2), float32 arrays of length steps + 1 (entry 0 unused, zero): Adam's bias corrections c1[t] = float32(1 / (1 - 0.9**t))
    and c2[t] = float32(1 / (1 - 0.999**t)), each computed in float64 and rounded once -- the values the library passes to its kernel."""
    steps = int(steps)
    if not 1 <= steps <= FIT_MAX_STEPS:
        raise ValueError("steps must be in 1..%d, got %d" % (FIT_MAX_STEPS, steps))
    if not _FIT_CONSTS:     # entry t does not depend on steps: the whole table once
        c1, c2 = np.zeros(FIT_MAX_STEPS + 1, np.float32), np.zeros(FIT_MAX_STEPS + 1, np.float32)
        for t in range(1, FIT_MAX_STEPS + 1):
            c1[t] = np.float32(1.0 / (1.0 - 0.9 ** t))
            c2[t] = np.float32(1.0 / (1.0 - 0.999 ** t))
        _FIT_CONSTS.extend((c1, c2))
    return _FIT_CONSTS[0][:steps + 1].copy(), _FIT_CONSTS[1][:steps + 1].copy()


def fit_adam_step(z, g, m, v, t, lr):
    """Adam step t (1-based) of ian_session_fit on float32 arrays of one shape -> (z_new, m_new, v_new).  Every operation is a
    float32 numpy operation rounded on its own, in the order of csrc/ian_fit_step.h:
        m = (0.9f * m) + (0.1f * g);  v = (0.999f * v) + ((0.001f * g) * g);  z - ((lr * (m * c1[t])) / (sqrt(v * c2[t]) + 1e-8f))"""
    z, g, m, v = (np.asarray(a, np.float32) for a in (z, g, m, v))
    t = int(t)
    c1, c2 = fit_adam_consts(t)
    lr = np.float32(lr)
    m = (FIT_BETA1 * m) + (FIT_ONE_M_BETA1 * g)
    v = (FIT_BETA2 * v) + ((FIT_ONE_M_BETA2 * g) * g)
    mh = m * c1[t]
    vh = v * c2[t]
    z_new = z - ((lr * mh) / (np.sqrt(vh) + FIT_EPS))
    assert z_new.dtype == np.float32 and m.dtype == np.float32 and v.dtype == np.float32
    return z_new, m, v


def fit_loss(x, target, box):
    """The API.py:64 loss of one image: the float64 mean of (float64(x) - float64(target))**2 over channels x rows r1:r2 x columns
    c1:c2 of (3,64,64) arrays, box = (c1, r1, c2, r2); 0.0 for an empty rectangle."""
    c1, r1, c2, r2 = (int(b) for b in box)
    a = np.asarray(x, np.float64)[:, r1:r2, c1:c2]
    b = np.asarray(target, np.float64)[:, r1:r2, c1:c2]
    if a.size == 0:
        return 0.0
    return float(np.mean((a - b) ** 2))
