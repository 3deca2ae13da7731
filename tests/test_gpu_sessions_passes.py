"""The brush calls that render in the same submission (brush_view, with and without tips; brush_compose) at a brush_pass below n: the
events run as passes of two and one, the windows follow the last pass.  Two models with the same parameters and one pool each get the
same photos; one side makes the one call, the other brush and then render / compose under the same option.  Every comparison is
np.array_equal, the library against itself across call forms."""
import numpy as np
import pytest

from session_helpers import KEYS64, assert_fields, model_pool, sources

pytestmark = pytest.mark.gpu

CAP = 12
BOXES = np.array([(10, 12, 30, 28), (33, 5, 50, 20), (2, 40, 22, 56)])           # the first and the last: 20 wide, 16 high, as the tips
COLOURS = np.array([(250, 20, 20), (10, 240, 90), (30, 30, 200)])

_cache = {}


def pools():
    """((model A, pool A), (model B, pool B)): full resolution at scale 2, two tips, one 128 x 128 canvas."""
    if "p" not in _cache:
        pair = []
        for _ in range(2):
            m, pool = model_pool("IAN_simple", capacity=CAP)
            pool.reserve_hires(2)
            pool.reserve_tips(2)
            rs = np.random.RandomState(3)
            for t in range(2):
                pool.set_tip(t, rs.uniform(0.1, 1.0, (16, 20)))
            pool.reserve_canvases(1, 128, 128, 4)
            pair.append((m, pool))
        _cache["p"] = pair
    return _cache["p"]


class brush_pass:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        for m, _ in pools():
            m.handle.set_option("brush_pass", self.value)

    def __exit__(self, *exc):
        for m, _ in pools():
            m.handle.set_option("brush_pass", 256)


@pytest.mark.parametrize("tips", [None, [0, -1, 1]])
def test_brush_view_in_passes_is_brush_then_render_and_leaves_no_residency(tips):
    (_, A), (_, B) = pools()
    ids, spare = [1, 7, 4], [0]
    src = sources(4, 2, 23)
    for p in (A, B):
        opened = p.open_hires(ids + spare, src)
    origins, size = np.array([(32, 32), (76, 16), (16, 88)]), (16, 16)           # each window in the middle of its session's rectangle, at scale 2
    with brush_pass(2):
        shown, out = A.brush_view(ids, BOXES, COLOURS, None, 0.5, -1.0, origins, size, tips=tips)
        shown_w = B.brush(ids, BOXES, COLOURS, None, 0.5, -1.0, tips=tips)
        out_w = B.render(ids, origins, size)
    assert out.shape == (3, 3, 16, 16) and np.array_equal(shown, shown_w) and np.array_equal(out, out_w)
    assert all((shown[k] != opened[k]).any() for k in range(3))                  # every event shows, the last pass's too
    assert np.array_equal(out, A.render(ids, origins, size))                     # the windows were taken after the last pass's blend
    assert any((out[k] != src[k][:, y:y + 16, x:x + 16]).any() for k, (x, y) in enumerate(origins))
    for i in ids:
        assert_fields(A.read(i), B.read(i), KEYS64 + ("FIELD", "FIELD_KIND", "SOURCE"), i)
    # The activations on A belong to the last pass alone (session 4 at batch 1).  A call on the same ids that now fits one pass must
    # gather and run the forward, as on a handle whose residency another call has ended for certain.
    B.open_hires(spare, src[3:])
    again, again_w = (p.brush(ids, BOXES, COLOURS, None, 0.5, -1.0, tips=tips) for p in (A, B))
    assert np.array_equal(again, again_w) and not np.array_equal(again, shown)
    for i in ids:
        assert_fields(A.read(i), B.read(i), KEYS64 + ("FIELD", "FIELD_KIND"), i)


def test_brush_compose_in_passes_is_brush_then_compose():
    (_, A), (_, B) = pools()
    ids = [2, 5, 8]                                                              # 2 and 5 placed, their squares overlapping; 8 is not
    rs = np.random.RandomState(17)
    c = np.uint8(rs.randint(0, 256, (3, 128, 128)))
    for p in (A, B):
        p.canvas_put(0, c)
        p.place(ids[:2], 0, [(4, 8), (36, 56)], [1, 1])
        p.open(ids[2:], c[None, :, 60:124, 60:124].copy())
    win = ([0, 0], [(0, 0), (64, 40)], (64, 88))                                 # between them every pixel of both squares
    with brush_pass(2):
        shown, out = A.brush_compose(ids, BOXES, COLOURS, None, 0.5, -1.0, windows=win)
        shown_w = B.brush(ids, BOXES, COLOURS, None, 0.5, -1.0)
        out_w = B.compose(*win)
    assert out.shape == (2, 3, 88, 64) and np.array_equal(shown, shown_w) and np.array_equal(out, out_w)
    assert (out[0] != c[:, :88, :64]).any() or (out[1] != c[:, 40:128, 64:128]).any()   # the windows show an edit
    for i in ids:
        assert_fields(A.read(i), B.read(i), KEYS64 + ("FIELD", "FIELD_KIND"), i)
