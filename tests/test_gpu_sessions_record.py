"""Saving and loading whole edit sessions (ian_session_record_info, ian_session_save, ian_session_load; EditSessions.save / load).
Every comparison is exact, bytes against bytes: a record is the pool's rows rearranged (npe_ops.session_record_pack is the
specification), and a loaded session must go on exactly as the saved one would have.  Two handles with the same weights: pool A
does the work, pool B is the other handle a session moves to, and the pool that never saw a load."""
import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from oracle import ian_oracle as O
import session_helpers as H
from session_helpers import assert_fields, model_pool, refused
from session_record_helpers import Tracker, expected_record

pytestmark = pytest.mark.gpu

CAP = 8
SCALE, DEPTH = 2, 3
X = [5, 1, 6]                       # a: full-resolution source, local + dampen, a wrapped ring, the cursor mid-list; b: plain; c: sample mode
Y = [0, 7, 3]
BOXES = np.array([(0, 0, 4, 4), (23, 30, 40, 47), (60, 60, 64, 64), (30, 35, 47, 52), (5, 9, 16, 20)])
COLOURS = np.array([(250, 20, 20), (10, 240, 90), (30, 30, 200), (200, 200, 10), (90, 10, 160)])

_cache = {}


def reserve(pool, scale=SCALE, local=True, depth=DEPTH):
    """The pool's three reservations, in the order the library wants them (the history goes first and comes last)."""
    pool.reserve_history(0)
    pool.reserve_hires(scale)
    pool.reserve_local(local)
    pool.reserve_history(depth)


def pools():
    if "ab" not in _cache:
        _cache["ab"] = model_pool("IAN_simple", capacity=CAP) + model_pool("IAN_simple", capacity=CAP)
        reserve(_cache["ab"][1])
        reserve(_cache["ab"][3])
    return _cache["ab"]


def fields(pool, ids):
    return [pool.read(i) for i in ids]


def same(got, want, tag):
    assert len(got) == len(want), tag
    for g, w in zip(got, want):
        assert set(g) == set(w), (tag, sorted(g), sorted(w))
        assert_fields(g, w, tuple(w), tag)


def counters(pool, ids):
    return [(h["depth"], h["undo"], h["redo"]) for h in (pool.history(i) for i in ids)]


def part_one(pool, ids):
    """The three sessions of the issue -> the tracker that knows what their rings hold."""
    a, b, c = ids
    tr = Tracker(pool, ids)
    pool.open_hires([a], H.sources(1, SCALE, 3))
    pool.open([b, c], H.sources(2, 1, 4))
    pool.set_local(ids, flags=[3, 0, 0])                                 # an open keeps the flags an earlier test left
    pool.sample([c], O.make_latents(1, seed=7))
    for k in range(5):                                                   # depth 3: the ring wraps, its base moves off slot 0
        tr.mark([a])
        pool.paint([a], BOXES[k], COLOURS[k], weight=0.5)
        tr.edited([a])
    tr.undo([a])                                                         # the tip is saved behind the list, the cursor is mid-list
    pool.scroll([b], BOXES[1], [1.0], weight=0.3)
    pool.paint([c], BOXES[2], COLOURS[2], weight=0.5)
    assert tr.H[a].base != 0 and (tr.H[a].len, tr.H[a].cur) == (4, 2)
    return tr


def part_two(pool, ids):
    """Editing goes on -> everything it shows and leaves behind."""
    a = ids[0]
    log = [pool.paint(ids, BOXES[:3], COLOURS[:3], weight=0.5), pool.undo([a], 2), pool.redo([a], 1),
           pool.paint(ids, BOXES[2:5], COLOURS[2:5], weight=0.5), pool.render([a], (8, 12), (64, 40))]
    pool.mark(ids)
    log.append(pool.paint(ids, BOXES[1:4], COLOURS[1:4], weight=0.5))
    return log, fields(pool, ids), counters(pool, ids)


def baseline():
    """part one and part two on pool A without a save between them."""
    if "base" not in _cache:
        _, sa, _, _ = pools()
        part_one(sa, X)
        _cache["base"] = part_two(sa, X)
    return _cache["base"]


def same_run(got, tag):
    log, f, c = got
    wlog, wf, wc = baseline()
    assert len(log) == len(wlog)
    for k, (g, w) in enumerate(zip(log, wlog)):
        assert g.shape == w.shape and np.array_equal(g, w), (tag, "shown / window", k)
    same(f, wf, tag)
    assert c == wc, tag


# ---- 1. the record equals the specification ----------------------------------------------------------------------------------------
def test_record_equals_the_spec():
    _, sa, _, _ = pools()
    tr = part_one(sa, X)
    before = fields(sa, X)
    rec = sa.save(X)
    same(fields(sa, X), before, "a save changes no session")
    offsets, body_bytes = N.session_record_layout(100, SCALE, True, DEPTH)
    assert rec.body.shape == (3, body_bytes) and rec.meta.shape == (3,)
    for k, sid in enumerate(X):
        meta, body = expected_record(sa, tr, sid)
        for name in N.SESSION_META_DTYPE.names:
            assert np.array_equal(rec.meta[k][name], meta[name]), (sid, name, rec.meta[k][name], meta[name])
        names = list(offsets)
        for j, name in enumerate(names):                                 # array by array, so that a failure names it
            lo, hi = offsets[name], offsets[names[j + 1]] if j + 1 < len(names) else body_bytes
            assert np.array_equal(rec.body[k, lo:hi], body[lo:hi]), (sid, name)
    a, b, c = (rec.meta[k] for k in range(3))
    assert (int(a["has_source"]), int(a["local_flags"]), int(a["hist_len"]), int(a["hist_cur"])) == (1, 3, 4, 2)
    assert (int(b["has_source"]), int(b["local_flags"]), int(b["hist_len"]), int(b["hist_cur"])) == (0, 0, 0, 0)
    assert (int(c["has_source"]), int(c["local_flags"]), int(c["hist_len"]), int(c["hist_cur"])) == (0, 0, 0, 0)
    fa, ea = N.session_record_unpack(rec.meta[0], rec.body[0])
    fc, _ = N.session_record_unpack(rec.meta[2], rec.body[2])
    assert len(ea) == 4 and fa["MODE"] == 0 and fc["MODE"] == 1 and fa["UMASK"].any() and "SOURCE" not in fc
    info = sa.record_info()
    assert info == {"num_latents": 100, "scale": SCALE, "local": 1, "depth": DEPTH, "body_bytes": body_bytes, "offsets": list(offsets.values())}


# ---- 2. resuming equals never having left ------------------------------------------------------------------------------------------
def test_resuming_on_another_handle_equals_never_having_left():
    _, sa, _, sb = pools()
    part_one(sa, X)
    rec = sa.save(X)
    sb.load(Y, rec)
    assert counters(sb, Y) == counters(sa, X)
    same(fields(sb, Y), fields(sa, X), "loaded")
    same_run(part_two(sb, Y), "second handle")


def test_resuming_after_the_ids_were_used_for_something_else_equals_never_having_left():
    _, sa, _, _ = pools()
    part_one(sa, X)
    rec = api.SessionRecords.frombytes(sa.save(X).tobytes())             # through the file form
    sa.open(X, H.sources(3, 1, 9))                                       # other photos, other flags, other histories
    sa.set_local(X, flags=[1, 2, 3])
    for k in range(2):
        sa.mark(X)
        sa.paint(X, BOXES[k], COLOURS[k], weight=0.5)
    assert counters(sa, X) == [(DEPTH, 2, 0)] * 3
    sa.load(X, rec)
    same_run(part_two(sa, X), "loaded back")


# ---- 3. canonical form -------------------------------------------------------------------------------------------------------------
def test_records_are_canonical():
    _, sa, _, _ = pools()
    part_one(sa, X)
    rec = sa.save(X)
    sa.load(Y, rec)                                                      # the rings of Y start at slot 0, those of X did not
    again = sa.save(Y)
    assert again.meta.tobytes() == rec.meta.tobytes()
    assert np.array_equal(again.body, rec.body)
    twice = sa.save(X)
    assert twice.meta.tobytes() == rec.meta.tobytes() and np.array_equal(twice.body, rec.body)


# ---- 4. neighbours -----------------------------------------------------------------------------------------------------------------
def test_a_load_leaves_the_other_sessions_alone():
    _, sa, _, sb = pools()
    everyone, others = [1, 2, 3, 4, 5, 6], [1, 3, 4, 6]
    ph = H.sources(6, 1, 21)
    for s in (sa, sb):
        s.open(everyone, ph)
        s.set_local(everyone, flags=[3, 1, 0, 2, 1, 3])
        s.mark(everyone)
        s.paint(everyone, BOXES[0], COLOURS[0], weight=0.5)
    before = fields(sa, others)
    sa.load([2, 5], sa.save([1, 3]))
    same(fields(sa, others), before, "after the load")
    same(fields(sa, others), fields(sb, others), "the pool that never loaded")
    same(fields(sa, [2, 5]), fields(sa, [1, 3]), "the targets")
    assert np.array_equal(sa.undo(others), sb.undo(others))
    same(fields(sa, others), fields(sb, others), "after an undo")
    assert counters(sa, others) == counters(sb, others) == [(DEPTH, 0, 1)] * 4


# ---- 5. passes and pointers --------------------------------------------------------------------------------------------------------
def test_staging_passes_and_device_bodies_give_the_same_bytes():
    import torch
    ma, sa, _, _ = pools()
    part_one(sa, X)
    rec = sa.save(X)
    bb = rec.body.shape[1]
    try:
        ma.handle.set_option("session_stage_bytes", bb)                  # one record per pass: three passes
        small = sa.save(X)
        assert small.meta.tobytes() == rec.meta.tobytes() and np.array_equal(small.body, rec.body)
        sa.load(Y, rec)
        assert np.array_equal(sa.save(Y).body, rec.body)
        ma.handle.set_option("session_stage_bytes", 1)                   # less than a record is still one record per pass
        assert np.array_equal(sa.save(X).body, rec.body)
    finally:
        ma.handle.set_option("session_stage_bytes", 64 << 20)
    dev = sa.save(X, device=True)
    assert dev.on_device and dev.body.is_cuda and dev.meta.tobytes() == rec.meta.tobytes()
    torch.cuda.synchronize()
    assert np.array_equal(dev.body.cpu().numpy(), rec.body)
    sa.open(Y, H.sources(3, 1, 33))                                      # something else in the targets first
    sa.load(Y, dev)
    torch.cuda.synchronize()
    same(fields(sa, Y), fields(sa, X), "loaded from device memory")
    assert counters(sa, Y) == counters(sa, X)
    assert np.array_equal(sa.save(Y).body, rec.body)


# ---- 6. residency ------------------------------------------------------------------------------------------------------------------
def test_a_save_keeps_and_a_load_ends_the_residency_of_brush():
    _, sa, _, sb = pools()
    a = [4]
    ph = H.sources(1, 1, 41)
    for s in (sa, sb):
        s.open(a, ph)
    rec0 = sa.save(a)
    first = sa.paint(a, BOXES[1], COLOURS[1], weight=0.5)
    assert np.array_equal(sb.paint(a, BOXES[1], COLOURS[1], weight=0.5), first)
    mid = sa.save(a)                                                     # A saves between two brushes of the same session, B does not
    assert np.array_equal(sa.paint(a, BOXES[3], COLOURS[3], weight=0.5), sb.paint(a, BOXES[3], COLOURS[3], weight=0.5))
    same(fields(sa, a), fields(sb, a), "save between two brushes")
    assert not np.array_equal(N.session_record_unpack(mid.meta[0], mid.body[0])[0]["Z"], sa.read(4)["Z"])
    # a load over a session whose forward is resident: the next brush starts from the record's latent
    assert not np.array_equal(N.session_record_unpack(rec0.meta[0], rec0.body[0])[0]["Z"], sa.read(4)["Z"])
    sa.load(a, rec0)
    sb.open([2], H.sources(1, 1, 42))                                    # B: a freshly loaded session, another one's forward resident
    sb.paint([2], BOXES[0], COLOURS[0], weight=0.5)
    sb.load(a, rec0)
    assert np.array_equal(sa.paint(a, BOXES[1], COLOURS[1], weight=0.5), first)
    assert np.array_equal(sb.paint(a, BOXES[1], COLOURS[1], weight=0.5), first)
    same(fields(sa, a), fields(sb, a), "brush after a load")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_change_nothing():
    import torch
    ma, sa, mb, sb = pools()
    ha, hb = ma.handle, mb.handle
    sa.reserve(1)                                                        # ids 1..7 come back unopened
    sa.reserve(CAP)
    part_one(sa, X)
    rec = sa.save(X)
    bb = rec.body.shape[1]
    T = [2, 4, 7]                                                        # the targets of the refused loads: never opened
    before, count = fields(sa, X), counters(sa, X)
    i32 = lambda v: np.asarray(v, np.int32)
    meta3, body3 = np.zeros(3, N.SESSION_META_DTYPE), np.full((3, bb), 7, np.uint8)

    def unchanged(tag):
        same(fields(sa, X), before, tag)
        assert counters(sa, X) == count, tag
        assert np.all(body3 == 7) and not meta3.tobytes().strip(b"\0"), tag
        for t in T:
            assert t not in sa._opened
            refused(lambda: ha.session_read(t, "Z"), "session %d has not been opened" % t, -7)

    def tamper(i, **kw):
        m = rec.meta.copy()
        for k, v in kw.items():
            m[i][k] = v
        return m

    def other_layout(scale=SCALE, local=True, depth=DEPTH):
        """Three records from pool B in another layout."""
        reserve(sb, scale, local, depth)
        sb.open(Y, H.sources(3, 1, 51))
        return sb.save(Y)

    save = lambda ids, n=None: lambda: ha.session_save(i32(ids), meta3, body3)
    load = lambda ids, meta=rec.meta, body=rec.body: lambda: ha.session_load(i32(ids), meta, body)
    bad = [
        ("n = 0", save([])), ("n = 257", lambda: ha.session_save(np.arange(257, dtype=np.int32), meta3, body3)),
        ("item 1: session %d outside the pool" % CAP, save([5, CAP])), ("item 0: session -1 outside the pool", save([-1])),
        ("item 2: session 5 already appears as item 0", save([5, 1, 5])), ("item 1: session 2 has not been opened", save([5, 2])),
        ("body .* is not 16-byte aligned", lambda: ha.session_save(i32(X), meta3, body3.reshape(-1)[4:])),
        ("must be a host array", lambda: ha.session_save(torch.tensor(X, dtype=torch.int32, device="cuda"), meta3, body3)),
        ("meta must be a host array", lambda: ha.session_save(i32(X[:1]), torch.zeros(64, dtype=torch.uint8, device="cuda"), body3)),
        ("n = 0", load([])), ("item 1: session %d outside the pool" % CAP, load([2, CAP, 4])),
        ("item 2: session 2 already appears as item 0", load([2, 4, 2])),
        ("body .* is not 16-byte aligned", lambda: ha.session_load(i32([2]), rec.meta, np.concatenate([body3[0], body3[0]])[8:])),
        ("meta must be a host array", lambda: ha.session_load(i32([2]), torch.zeros(64, dtype=torch.uint8, device="cuda"), rec.body)),
        ("item 1: magic = 0 ", load(T, tamper(1, magic=0))),
        (r"item 0: format = 2 \(this pool: 1\)", load(T, tamper(0, format=2))),
        (r"item 2: body_bytes = %d \(this pool: %d\)" % (bb - 16, bb), load(T, tamper(2, body_bytes=bb - 16))),
        (r"item 1: num_latents = 99 \(this pool: 100\)", load(T, tamper(1, num_latents=99))),
        ("item 0: local_flags = 4 ", load(T, tamper(0, local_flags=4))),
        ("item 0: has_source = 2 ", load(T, tamper(0, has_source=2))),
        ("item 0: hist_cur = 5 ", load(T, tamper(0, hist_cur=5))),                 # the cursor behind the entries
        ("item 0: hist_len = 4 .*cursor at the tip", load(T, tamper(0, hist_cur=4))),   # four entries need a cursor before the tip
        ("item 0: hist_len = 5 ", load(T, tamper(0, hist_len=5))),
        ("item 1: hist_cur = -1 ", load(T, tamper(1, hist_cur=-1))),
        ("item 2: reserved = 1 ", load(T, tamper(2, reserved=[0, 0, 1, 0]))),
    ]
    for needle, call in bad:
        refused(call, needle, -7)
        unchanged(needle)
    try:
        for kw, needle in (({"scale": 4}, r"item 0: scale = 4 \(this pool: 2\)"), ({"scale": 0}, r"item 0: scale = 0 \(this pool: 2\)"),
                           ({"depth": 5}, r"item 0: depth = 5 \(this pool: 3\)"), ({"depth": 0}, r"item 0: depth = 0 \(this pool: 3\)"),
                           ({"local": False}, r"item 0: local = 0 \(this pool: 1\)")):
            other = other_layout(**kw)
            assert other.body.shape[1] != bb
            refused(load(T, other.meta, other.body), needle, -7)
            unchanged(needle)
            with pytest.raises(ValueError):                              # and the Python surface refuses before the library
                sa.load(T, other)
            unchanged("python: " + needle)
        # a source needs a scale, flags need the local reservation: pool B without either
        plain = other_layout(scale=0, local=False, depth=0)
        m = plain.meta.copy()
        m[1]["has_source"] = 1
        refused(lambda: hb.session_load(i32(Y), m, plain.body), "item 1: has_source = 1 .*scale 0", -7)
        m = plain.meta.copy()
        m[2]["local_flags"] = 1
        refused(lambda: hb.session_load(i32(Y), m, plain.body), "item 2: local_flags = 1 .*without the local reservation", -7)
        m = plain.meta.copy()
        m[0]["hist_len"] = 1
        refused(lambda: hb.session_load(i32(Y), m, plain.body), "item 0: hist_len = 1 .*without a history", -7)
        sb.load(Y, plain)                                                # what was refused was the meta, not the pool
        # -6: no pool
        sb.close()
        refused(lambda: hb.session_save(i32([0]), meta3, body3), "no session pool", -6)
        refused(lambda: hb.session_load(i32([0]), plain.meta, plain.body), "no session pool", -6)
        refused(lambda: hb.session_record_info(), "no session pool", -6)
        unchanged("-6")
    finally:
        sb.reserve(CAP)
        reserve(sb)
    # the pool still works, and so does the one that was rebuilt
    sa.load(Y, rec)
    same(fields(sa, Y), before, "a load after the refusals")
    sb.load(Y, rec)
    same(fields(sb, Y), before, "the rebuilt pool")
