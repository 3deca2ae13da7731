"""The edge-aware full-resolution render (ian_sessions_reserve_guide, ian_sessions_guide; EditSessions.reserve_guide / guide).  Every
comparison is np.array_equal against npe_ops.hires_render_guided, whose inputs (SOURCE, GIM, FIELD, FIELD_KIND) are read back from the
pool after a paint event that leaves a non-zero field: the numpy function specifies the arithmetic and the device matches it bit for
bit.  Every test switches the guide off again: the pool is shared."""
import numpy as np
import pytest

from oracle import ian_oracle as O
from session_helpers import assert_fields, model_pool, refused, sources

pytestmark = pytest.mark.gpu

CAP = 16
KEYS = ("Z", "RECON", "ERROR", "IM", "GIM", "MODE", "FIELD", "FIELD_KIND", "SOURCE")

_cache = {}


def pool():
    if not _cache:
        _cache["mp"] = model_pool("IAN_simple", capacity=CAP)
    return _cache["mp"]


def table_of(sigma):
    from neural_photo_editor_amd import npe_ops as N
    return N.guide_table(sigma)


def painted(s, ids, seed, sample=()):
    """A pool at scale s whose sessions `ids` hold photos and, after one paint event, non-zero edit fields (kind 0); the sessions of
    `sample` are in sample mode (their FIELD is x, kind 1).  -> (model, pool, {id: what read() gives})"""
    m, sh = pool()
    sh.reserve_guide()
    sh.reserve_hires(s)
    sh.open_hires(ids, sources(len(ids), s, seed))
    if sample:
        sh.sample(list(sample), O.make_latents(len(sample), seed=seed))
    boxes = np.array([(10 + 3 * k, 12 + 2 * k, 34 + 3 * k, 40 + 2 * k) for k in range(len(ids))])
    sh.paint(ids, boxes, np.array([(250, 20, 30), (10, 240, 90), (40, 60, 250), (200, 200, 10)][:len(ids)]), weight=0.5)
    got = {i: sh.read(i) for i in ids}
    for i in ids:
        assert got[i]["FIELD"].any() and got[i]["FIELD_KIND"] == (1 if i in sample else 0), i
    return m, sh, got


def reference(got, s, win, table):
    from neural_photo_editor_amd import npe_ops as N
    return N.hires_render_guided(got["SOURCE"], got["GIM"], got["FIELD"], int(got["FIELD_KIND"]), s, *win, table)


def windows(S):
    """(x, y, vw, vh): vw = 4, vh = 1 at the four corners (clamped taps); vh = 9 from an odd y (more than two bands, the last one
    short); an interior window of several uchar4 per lane."""
    return [(0, 0, 4, 1), (S - 4, 0, 4, 1), (0, S - 1, 4, 1), (S - 4, S - 1, 4, 1), (8, 37, 24, 9),
            ((S - 48) // 8 * 4, (S - 50) // 2, 48, 50)]


# ---- 1. the render -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 16])
def test_windows_of_three_sessions_match_the_specification(s):
    ids = [9, 2, 14]
    _, sh, got = painted(s, ids, 10 * s)
    table = table_of(4.0)
    sh.reserve_guide(table=table)
    try:
        edited = False
        for win in windows(64 * s):
            out = sh.render(ids, win[:2], win[2:])
            assert out.shape == (3, 3, win[3], win[2]) and out.dtype == np.uint8
            for k, i in enumerate(ids):
                assert np.array_equal(out[k], reference(got[i], s, win, table)), (s, i, win)
                edited |= bool((out[k] != got[i]["SOURCE"][:, win[1]:win[1] + win[3], win[0]:win[0] + win[2]]).any())
        assert edited                                                        # some window shows the edit
    finally:
        sh.reserve_guide()
        if s == 16:
            sh.reserve_hires(0)


def test_the_whole_picture_two_tiles_and_mixed_kinds_in_one_call():
    from neural_photo_editor_amd import npe_ops as N
    s, S = 3, 192
    ids = [3, 11, 6]
    _, sh, got = painted(s, ids, 77, sample=(6,))
    table = table_of(8.0)
    sh.reserve_guide(table=table)
    try:
        whole = sh.render(ids, (0, 0), S)                                     # a photo-mode and a sample-mode session in one call
        for k, i in enumerate(ids):
            assert np.array_equal(whole[k], reference(got[i], s, (0, 0, S, S), table)), i
        assert np.array_equal(whole[2], N.hires_render(got[6]["SOURCE"], got[6]["FIELD"], 1, s, 0, 0, S, S))   # kind 1: the plain render
        assert (whole[0] != N.hires_render(got[3]["SOURCE"], got[3]["FIELD"], 0, s, 0, 0, S, S)).any()        # kind 0: not the plain one
        tiles = sh.render([3, 3], [(0, 0), (96, 0)], (96, S))                 # two tiles of one session
        assert np.array_equal(tiles[0], whole[0][:, :, :96]) and np.array_equal(tiles[1], whole[0][:, :, 96:])
    finally:
        sh.reserve_guide()


def test_brush_view_is_brush_then_render():
    s = 3
    A, B = [1, 7], [8, 4]
    m, sh = pool()
    sh.reserve_guide()
    sh.reserve_hires(s)
    src = sources(2, s, 13)
    sh.open_hires(A, src)
    sh.open_hires(B, src)
    table = table_of(4.0)
    sh.reserve_guide(table=table)
    try:
        boxes, colours = np.array([(10, 12, 30, 28), (33, 5, 50, 20)]), np.array([(250, 20, 20), (10, 240, 90)])
        origins, size = np.array([(40, 36), (96, 100)]), (88, 57)
        shown, out = sh.brush_view(A, boxes, colours, None, 0.5, -1.0, origins, size)
        shown_w = sh.paint(B, boxes, colours, weight=0.5)
        out_w = sh.render(B, origins, size)
        assert np.array_equal(shown, shown_w) and out.shape == (2, 3, 57, 88) and np.array_equal(out, out_w)
        for k, (a, b) in enumerate(zip(A, B)):
            ga = sh.read(a)
            assert_fields(ga, sh.read(b), KEYS)
            assert np.array_equal(out[k], reference(ga, s, (*origins[k], *size), table))
        assert (out != src[:, :, 36:36 + 57, 40:40 + 88]).any()
    finally:
        sh.reserve_guide()


def test_commit_renders_the_guided_picture_into_the_source():
    s, S = 2, 128
    ids = [12, 5]
    _, sh, got = painted(s, ids, 21)
    table = table_of(4.0)
    sh.reserve_guide(table=table)
    try:
        before = sh.render(ids, (0, 0), S)
        for k, i in enumerate(ids):
            assert np.array_equal(before[k], reference(got[i], s, (0, 0, S, S), table))
            assert (before[k] != got[i]["SOURCE"]).any()
        shown = sh.commit(ids)
        for k, i in enumerate(ids):
            after = sh.read(i)
            assert np.array_equal(after["SOURCE"], before[k]), i             # in place: every lane stored what the render gives
            assert np.array_equal(after["GIM"], got[i]["IM"]) and np.array_equal(after["IM"], got[i]["IM"]) and np.array_equal(shown[k], got[i]["IM"])
            assert not after["FIELD"].any() and after["FIELD_KIND"] == 0
        assert np.array_equal(sh.render(ids, (0, 0), S), before)
    finally:
        sh.reserve_guide()


# ---- 2. the reservation -------------------------------------------------------------------------------------------------------------
def test_replacing_the_table_and_switching_the_guide_off():
    from neural_photo_editor_amd import npe_ops as N
    s = 3
    ids = [0, 1, 2]
    win = (40, 37, 64, 50)
    _, sh, got = painted(s, ids, 5)
    assert sh.guide() is None
    plain = sh.render(ids, win[:2], win[2:])
    try:
        outs = {}
        for sigma in (4.0, 16.0):                                            # the second call replaces the table
            sh.reserve_guide(sigma)
            t = sh.guide()
            assert t.dtype == np.float32 and np.array_equal(t, table_of(sigma))
            outs[sigma] = sh.render(ids, win[:2], win[2:])
            for k, i in enumerate(ids):
                assert np.array_equal(outs[sigma][k], reference(got[i], s, win, t)), (sigma, i)
        assert (outs[4.0] != outs[16.0]).any() and (outs[4.0] != plain).any()
        custom = np.linspace(1.0, 0.25, 766).astype(np.float32)             # any positive table, not only a Gaussian
        sh.reserve_guide(table=custom)
        assert np.array_equal(sh.guide(), custom)
        assert np.array_equal(sh.render([1], win[:2], win[2:])[0], reference(got[1], s, win, custom))
    finally:
        sh.reserve_guide()
    assert sh.guide() is None
    off = sh.render(ids, win[:2], win[2:])
    assert np.array_equal(off, plain)
    for k, i in enumerate(ids):
        assert np.array_equal(off[k], N.hires_render(got[i]["SOURCE"], got[i]["FIELD"], 0, s, *win))
        assert_fields(sh.read(i), got[i], KEYS)                               # a render, guided or not, changes no session


def test_refusals_return_their_code_and_change_nothing():
    s = 2
    ids = [0, 1]
    win = (8, 5, 64, 40)
    m, sh, got = painted(s, ids, 55)
    h = m.handle
    table = table_of(4.0)
    sh.reserve_guide(table=table)
    try:
        before = sh.render(ids, win[:2], win[2:])
        bad_zero, bad_nan, bad_neg, bad_inf = (table.copy() for _ in range(4))
        bad_zero[700], bad_nan[0], bad_neg[765], bad_inf[3] = 0.0, np.nan, -1.0, np.inf
        refused(lambda: h.sessions_reserve_guide(np.ones(5, np.float32)), "count 5", -7)
        refused(lambda: h.sessions_reserve_guide(np.ones(767, np.float32)), "count 767", -7)
        refused(lambda: h.sessions_reserve_guide(bad_zero), r"table\[700\]", -7)
        refused(lambda: h.sessions_reserve_guide(bad_nan), r"table\[0\]", -7)
        refused(lambda: h.sessions_reserve_guide(bad_neg), r"table\[765\]", -7)
        refused(lambda: h.sessions_reserve_guide(bad_inf), r"table\[3\]", -7)
        refused(lambda: h._check(h.lib.ian_sessions_reserve_guide(h._h, None, 766)), "null table", -7)
        refused(lambda: h.sessions_reserve_canvas(1, 128, 128, 0), "a guide is reserved", -6)           # canvases after a guide
        assert sh.canvases == 0
        assert np.array_equal(sh.guide(), table) and np.array_equal(sh.render(ids, win[:2], win[2:]), before)
        for i in ids:
            assert_fields(sh.read(i), got[i], KEYS)
        sh.reserve_guide()
        sh.reserve_canvases(1, 128, 128, 0)                                    # a guide after canvases
        try:
            refused(lambda: h.sessions_reserve_guide(table), "canvases are reserved", -6)
            assert sh.guide() is None
        finally:
            sh.reserve_canvases(0)
        plain = sh.render(ids, win[:2], win[2:])
        assert (plain != before).any()                                        # the refused call did not switch the guide on
        sh.reserve_hires(0)                                                   # no full-resolution reservation
        refused(lambda: h.sessions_reserve_guide(table), "no full-resolution reservation", -6)
        refused(lambda: h.sessions_reserve_guide(None), "no full-resolution reservation", -6)
        refused(lambda: h.sessions_guide(), "no full-resolution reservation", -6)
        sh.reserve_hires(s)                                                   # and a reservation freed with its group does not come back
        assert sh.guide() is None
    finally:
        sh.reserve_guide()


def test_hires_zero_frees_the_guide_and_a_new_scale_keeps_it():
    m, sh = pool()
    sh.reserve_guide()
    sh.reserve_hires(2)
    table = table_of(16.0)
    sh.reserve_guide(table=table)
    try:
        sh.reserve_hires(3)                                                   # the table does not depend on the scale
        assert np.array_equal(sh.guide(), table)
        ids = [4]
        sh.open_hires(ids, sources(1, 3, 8))
        sh.paint(ids, (10, 10, 40, 40), (250, 20, 30), weight=0.5)
        got = sh.read(4)
        assert np.array_equal(sh.render(ids, (0, 0), (64, 9))[0], reference(got, 3, (0, 0, 64, 9), table))
        sh.reserve_hires(0)
        assert sh.guide() is None and not sh.guided
        sh.reserve_hires(3)
        assert sh.guide() is None
    finally:
        sh.reserve_guide()


def test_save_and_load_round_trip_with_a_guide_reserved():
    s = 2
    ids, other = [3, 8], [10, 1]
    win = (0, 0, 128, 128)
    _, sh, got = painted(s, ids, 91)
    table = table_of(4.0)
    sh.reserve_guide(table=table)
    try:
        info = sh.record_info()
        before = sh.render(ids, win[:2], win[2:])
        rec = sh.save(ids)
        sh.load(other, rec)
        assert sh.record_info() == info and np.array_equal(sh.guide(), table)  # the guide is the pool's, not the records'
        after = sh.render(other, win[:2], win[2:])
        assert np.array_equal(after, before)
        for k, (a, b) in enumerate(zip(ids, other)):
            assert_fields(sh.read(b), got[a], KEYS)
            assert np.array_equal(after[k], reference(got[a], s, win, table))
        sh.reserve_guide()
        layout_off = sh.record_info()
        assert layout_off == info                                              # and the layout does not know it either
    finally:
        sh.reserve_guide()
