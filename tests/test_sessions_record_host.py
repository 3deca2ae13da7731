"""CPU tests of saved edit sessions (ian_session_record_info, ian_session_save, ian_session_load; EditSessions.save / load): the
record layout of npe_ops against sums written out by hand, pack / unpack as inverses and the canonical zeros, the C++ header
csrc/ian_session_record.h (compiled into a stand-alone program under AddressSanitizer and UBSan) against npe_ops.check_session_meta,
the header / export list agreement, the packer and EditSessions over a stub (every validation before any library call), and the file
form of SessionRecords."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import api, npe_ops as N
from neural_photo_editor_amd import lib as L
from session_helpers import HEADER, ROOT, header_code, run_c, stub_sessions
from session_record_helpers import META_FIELDS, random_session

NEW_EXPORTS = ("ian_session_record_info", "ian_session_save", "ian_session_load")
CSRC = os.path.join(ROOT, "neural_photo_editor_amd", "csrc")
LAYOUTS = [(100, 0, 0, 0), (100, 2, 1, 3), (100, 16, 1, 64), (7, 1, 0, 1), (100, 0, 1, 0), (100, 0, 0, 16), (5, 3, 1, 2)]
IMG = 3 * 64 * 64


def pad(b):
    return (b + 15) // 16 * 16


def by_hand(zl, scale, local, depth):
    """[(name, bytes)] of a body, every size written out: the table of include/ian.h and DESIGN.md 4.6."""
    cols = [("GIM", 12288), ("IM", 12288), ("RECON", 12288), ("ERROR", 49152), ("Z", 4 * zl), ("MODE", 4)]
    if scale:
        cols += [("SOURCE", 3 * (64 * scale) ** 2), ("FIELD", 49152), ("FIELD_KIND", 4)]
    if local:
        cols += [("UMASK", 32768), ("LOCAL", 4)]
    if depth:
        cols += [("HIST_Z", (depth + 1) * 4 * zl)]
        if local:
            cols += [("HIST_UMASK", (depth + 1) * 32768)]
    return cols


# ---- 1. the layout -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout_offsets_are_aligned_ordered_and_sum_up(layout):
    offsets, body_bytes = N.session_record_layout(*layout)
    want = by_hand(*layout)
    assert list(offsets) == [name for name, _ in want]                  # table order
    at = 0
    for name, nbytes in want:
        assert offsets[name] == at and at % 16 == 0, name
        at += pad(nbytes)
    assert body_bytes == at and body_bytes % 16 == 0
    assert len(offsets) <= L.SESSION_RECORD_MAX_COLUMNS
    assert int(N.session_meta(*layout)["body_bytes"]) == body_bytes


def test_layout_sizes_by_hand():
    assert N.session_record_layout(100, 0, 0, 0)[1] == 3 * 12288 + 49152 + 400 + 16 == 86432
    assert N.session_record_layout(7, 1, 0, 1)[1] == 3 * 12288 + 49152 + 32 + 16 + 12288 + 49152 + 16 + 64
    # include/ian.h: depth 16 and 100 latents with the local reservation are 563 856 bytes of rings
    base = N.session_record_layout(100, 0, 1, 0)[1]
    assert N.session_record_layout(100, 0, 1, 16)[1] - base == 563856
    assert N.SESSION_META_DTYPE.itemsize == 64 == ctypes.sizeof(L.SessionMeta)
    for name in N.SESSION_META_DTYPE.names:
        assert N.SESSION_META_DTYPE.fields[name][1] == getattr(L.SessionMeta, name).offset, name
    for bad in ((0, 0, 0, 0), (100, 17, 0, 0), (100, 0, 0, 65), (100, -1, 0, 0)):
        with pytest.raises(ValueError):
            N.session_record_layout(*bad)


# ---- 2. pack and unpack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [(100, 0, 0, 0), (100, 2, 1, 3), (7, 1, 0, 1), (5, 3, 1, 2), (100, 0, 0, 16)])
def test_pack_then_unpack_is_the_identity_and_the_unwritten_parts_are_zero(layout):
    zl, scale, local, depth = layout
    rs = np.random.RandomState(sum(layout))
    offsets, body_bytes = N.session_record_layout(*layout)
    sizes = dict(by_hand(*layout))
    for case in range(4):
        nent = min(case, depth + 1) if depth else 0
        with_source = bool(scale) and case % 2 == 0
        fields, entries = random_session(rs, zl, scale, local, nent, with_source)
        cur = nent if nent <= depth else nent - 1                       # depth + 1 entries: the cursor is not at the tip
        meta, body = N.session_record_pack(fields, entries, zl, scale, local, depth, hist_cur=cur)
        assert body.dtype == np.uint8 and body.shape == (body_bytes,)
        assert N.check_session_meta(meta, *layout) is None
        assert (int(meta["has_source"]), int(meta["hist_len"]), int(meta["hist_cur"])) == (int(with_source), nent, cur)
        assert int(meta["local_flags"]) == (fields["LOCAL"] if local else 0)
        f2, e2 = N.session_record_unpack(meta, body)
        assert set(f2) == set(fields) and len(e2) == nent
        for k in fields:
            assert np.array_equal(f2[k], fields[k]) and np.asarray(f2[k]).dtype == np.asarray(fields[k]).dtype, k
        for a, b in zip(e2, entries):
            if local:
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            else:
                assert np.array_equal(a, b)
        meta2, body2 = N.session_record_pack(f2, e2, zl, scale, local, depth, hist_cur=cur)
        assert meta2.tobytes() == meta.tobytes() and np.array_equal(body2, body)
        # canonical zeros: the padding, the slots that are no entries, a source that is not there
        for name, nbytes in sizes.items():
            assert not body[offsets[name] + nbytes:offsets[name] + pad(nbytes)].any(), name
        if depth:
            slot = 4 * zl
            assert not body[offsets["HIST_Z"] + nent * slot:offsets["HIST_Z"] + (depth + 1) * slot].any()
            assert nent == 0 or body[offsets["HIST_Z"]:offsets["HIST_Z"] + nent * slot].any()
            if local:
                assert not body[offsets["HIST_UMASK"] + nent * 32768:offsets["HIST_UMASK"] + (depth + 1) * 32768].any()
        if scale and not with_source:
            assert not body[offsets["SOURCE"]:offsets["SOURCE"] + sizes["SOURCE"]].any()
    with pytest.raises(ValueError):
        N.session_record_pack(fields, [fields["Z"]] * (depth + 2), zl, scale, local, depth)
    with pytest.raises(ValueError):
        N.session_record_unpack(meta, body[:-16])


# ---- 3. the C++ header against the model -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def record_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("record") / "session_record"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "session_record_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def scripted_metas(layout, seed, count=700):
    """Metas for a pool of `layout`: the valid ones of every history state, and for each a copy with one or two fields replaced by a
    value from a small set around the valid range (so that replacements are often still valid)."""
    zl, scale, local, depth = layout
    rs = random.Random(seed)
    bb = N.session_record_layout(*layout)[1]
    pool = {"magic": [N.SESSION_RECORD_MAGIC, 0, N.SESSION_RECORD_MAGIC + 1, 0x52414E49, 2 ** 32 - 1],
            "format": [1, 0, 2, -1], "num_latents": [zl, zl + 1, 0, 100, 7], "scale": [scale, 0, 1, 2, 16, -1], "local": [local, 0, 1, 2],
            "depth": [depth, 0, 1, 3, 64, depth + 1], "has_source": [0, 1, 2, -1], "local_flags": [0, 1, 2, 3, 4, -1],
            "hist_len": [0, 1, depth, depth + 1, depth + 2, -1, 65, 66], "hist_cur": [0, 1, depth, depth + 1, depth + 2, -1],
            "body_bytes": [bb, bb + 16, bb - 16, 0, 2 ** 40], "reserved": [0, 0, 1, -1]}
    out = []
    for _ in range(count):
        ln = rs.randint(0, depth + 1) if depth else 0
        cur = rs.randint(0, ln) if ln <= depth else rs.randint(0, ln - 1)
        m = N.session_meta(zl, scale, local, depth, has_source=rs.randint(0, 1) if scale else 0, local_flags=rs.randint(0, 3) if local else 0,
                           hist_len=ln, hist_cur=cur)
        assert N.check_session_meta(m, *layout) is None
        for _ in range(rs.choice((0, 1, 1, 1, 2))):
            k = rs.choice(sorted(pool))
            if k == "reserved":
                m["reserved"][rs.randint(0, 3)] = rs.choice(pool[k])
            else:
                m[k] = rs.choice(pool[k])
        out.append(m)
    return out


def meta_line(m):
    return "m " + " ".join(str(int(m[k])) for k in META_FIELDS) + " " + " ".join(str(int(v)) for v in m["reserved"]) + "\n"


def test_cpp_header_equals_the_model(record_program):
    refused = {}
    total = 0
    for li, layout in enumerate(LAYOUTS):
        metas = scripted_metas(layout, 300 + li)
        pads = [0, 1, 4, 15, 16, 17, 28, 400, 12288, 2 ** 31 + 5]
        rings = [(b, d, k) for d in (1, 3, 64) for b in (0, 1, d) for k in (0, 1, d)]
        text = "%d %d %d %d %d\n" % (layout + (N.session_record_layout(*layout)[1],))
        text += "".join("p %d\n" % b for b in pads) + "".join("r %d %d %d\n" % r for r in rings) + "".join(meta_line(m) for m in metas)
        r = subprocess.run([record_program], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        got = r.stdout.split("\n")[:-1]
        assert len(got) == len(pads) + len(rings) + len(metas)
        assert got[:len(pads)] == [str(pad(b)) for b in pads]
        assert got[len(pads):len(pads) + len(rings)] == [str((b + k) % (d + 1)) for b, d, k in rings]
        for m, g in zip(metas, got[len(pads) + len(rings):]):
            want = N.check_session_meta(m, *layout)
            assert g == (want or "ok"), (layout, meta_line(m), g, want)
            refused[g] = refused.get(g, 0) + 1
        total += len(metas)
    assert total >= 4000
    for field in META_FIELDS + ("reserved", "ok"):                      # every refusal field, and acceptance, were reached
        assert refused.get(field, 0) >= 5, (field, refused)


def test_the_cursor_rules_by_hand():
    ok = lambda depth, ln, cur, **kw: N.check_session_meta(N.session_meta(100, 0, kw.get("local", 0), depth, hist_len=ln, hist_cur=cur,
                                                                          local_flags=kw.get("flags", 0)), 100, 0, kw.get("local", 0), depth)
    assert ok(3, 0, 0) is None and ok(3, 3, 3) is None and ok(3, 4, 3) is None and ok(3, 4, 0) is None
    assert ok(3, 4, 4) == "hist_len"                                     # at the tip at most `depth` entries
    assert ok(3, 5, 2) == "hist_len"                                     # never more than depth + 1
    assert ok(3, 2, 3) == "hist_cur" and ok(3, 2, -1) == "hist_cur" and ok(3, -1, 0) == "hist_len"
    assert ok(0, 1, 0) == "hist_len" and ok(0, 0, 0) is None             # no history, no entries
    assert ok(0, 0, 0, flags=1) == "local_flags" and ok(0, 0, 0, flags=1, local=1) is None
    m = N.session_meta(100, 0, 0, 0, has_source=1)
    assert N.check_session_meta(m, 100, 0, 0, 0) == "has_source"
    m = N.session_meta(100, 2, 0, 0, has_source=1)
    assert N.check_session_meta(m, 100, 2, 0, 0) is None and N.check_session_meta(m, 100, 4, 0, 0) == "scale"


# ---- 4. header and loader ----------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99_with_the_new_declarations(tmp_path):
    """The program defines the three functions itself: a definition that disagreed with the header's declaration would not compile."""
    lines = run_c(tmp_path, [
        '#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"',
        'int ian_session_record_info(ian_handle* h, ian_session_meta* m, int64_t* o, int32_t* n) { (void)h; (void)o; m->body_bytes = 86432; *n = 6; return 0; }',
        'int ian_session_save(ian_handle* h, int32_t n, const int32_t* i, ian_session_meta* m, void* b, void* s) {',
        '  (void)h; (void)i; (void)b; (void)s; m[0].magic = IAN_SESSION_RECORD_MAGIC; return n; }',
        'int ian_session_load(ian_handle* h, int32_t n, const int32_t* i, const ian_session_meta* m, const void* b, void* s) {',
        '  (void)h; (void)i; (void)b; (void)s; return n + (int)m[0].format; }',
        'int main(void) {',
        '  ian_session_meta m = {0};',
        '  int32_t n = 0;',
        '  ian_session_record_info(0, &m, 0, &n);',
        '  m.format = IAN_SESSION_RECORD_FORMAT;',
        '  printf("%d %d %d %d %d\\n", (int)sizeof(ian_session_meta), (int)offsetof(ian_session_meta, body_bytes), (int)n,',
        '         ian_session_save(0, 3, 0, &m, 0, 0), ian_session_load(0, 2, 0, &m, 0, 0));',
        '  printf("%u %d %d\\n", (unsigned)m.magic, (int)m.body_bytes, IAN_SESSION_RECORD_MAX_COLUMNS);',
        '  return 0;', '}'])
    assert lines == ["64 40 6 3 3", "%d 86432 %d" % (N.SESSION_RECORD_MAGIC, L.SESSION_RECORD_MAX_COLUMNS)]


def test_header_and_export_list_agree_on_the_new_names():
    code = header_code()
    declared = set(re.findall(r"\b(ian_[a-z_0-9]+)\s*\(", code))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS, name
    lib = L.load_library()
    protos = {name: argt for _, name, argt in L.parse_header_prototypes(HEADER)}
    for name in NEW_EXPORTS:
        fn = getattr(lib, name)                        # exported by the built library
        assert fn.restype is ctypes.c_int32
        assert len(fn.argtypes) == len(protos[name]), name
    assert protos["ian_session_save"] == ["ptr", "int32_t", "ptr", "ptr", "ptr", "ptr"]
    assert protos["ian_session_load"] == protos["ian_session_save"]
    assert protos["ian_session_record_info"] == ["ptr"] * 4
    fields = re.search(r"typedef struct ian_session_meta \{(.*?)\} ian_session_meta;", code, flags=re.S).group(1)
    names = re.findall(r"\b(\w+)(?:\[4\])?;", fields)
    assert tuple(names) == N.SESSION_META_DTYPE.names == tuple(f[0] for f in L.SessionMeta._fields_)


# ---- 5. the packer and EditSessions over a stub ------------------------------------------------------------------------------------
def record_stub(scale=2, local=True, depth=3, **kw):
    s, h = stub_sessions(args=True, scale=scale, reserve=local, **kw)
    if depth:
        s.reserve_history(depth)
    h.calls.clear()
    return s, h


def records_for(layout, n, seed=0, sources=None):
    zl, scale, local, depth = layout
    rs = np.random.RandomState(seed)
    metas, bodies = [], []
    for i in range(n):
        with_source = bool(scale) and (sources is None or i in sources)
        f, e = random_session(rs, zl, scale, local, min(i, depth), with_source)
        m, b = N.session_record_pack(f, e, zl, scale, local, depth)
        metas.append(m)
        bodies.append(b)
    return api.SessionRecords(np.stack(metas), np.stack(bodies))


def test_valid_calls_reach_the_library_with_the_packed_arrays():
    s, h = record_stub()
    bb = N.session_record_layout(100, 2, 1, 3)[1]
    rec = s.save([2, 0, 3])
    (name, (ids, meta, body)), = h.calls
    assert name == "session_save" and ids.dtype == np.int32 and list(ids) == [2, 0, 3]
    assert meta is rec.meta and meta.dtype == N.SESSION_META_DTYPE and meta.shape == (3,) and meta.flags.c_contiguous
    assert body is rec.body and body.dtype == np.uint8 and body.shape == (3, bb) and body.ctypes.data % 16 == 0
    h.calls.clear()
    rec = records_for((100, 2, 1, 3), 2, sources={1})
    s.load([5, 1], rec)                                # 5 was not opened: a load opens it
    (name, (ids, meta, body)), = h.calls
    assert name == "session_load" and ids.dtype == np.int32 and list(ids) == [5, 1]
    assert meta.tobytes() == rec.meta.tobytes() and np.array_equal(body, rec.body) and body.ctypes.data % 16 == 0 and body.flags.c_contiguous
    assert {5, 1} <= s._opened and 1 in s._sourced and 5 not in s._sourced
    h.calls.clear()
    odd = np.empty(2 * bb + 1, np.uint8)[1:].reshape(2, bb)               # a body that is not 16-byte aligned is copied, not refused
    odd[...] = rec.body
    s.load([6, 7], api.SessionRecords(rec.meta, odd))
    assert h.calls[0][1][2].ctypes.data % 16 == 0 and np.array_equal(h.calls[0][1][2], rec.body)
    # the packer alone
    ids, meta, body = api.pack_session_records([4], rec[1], 100, 2, True, 3, capacity=8)
    assert list(ids) == [4] and len(meta) == 1 and body.shape == (1, bb) and int(meta[0]["has_source"]) == 1
    # a plain pool
    s, h = record_stub(scale=0, local=False, depth=0)
    rec = records_for((100, 0, 0, 0), 1)
    assert rec.body.shape == (1, 86432)
    s.load([7], rec)
    assert h.calls[-1][0] == "session_load"


def tampered(rec, i, **kw):
    meta = rec.meta.copy()
    for k, v in kw.items():
        meta[i][k] = v
    return api.SessionRecords(meta, rec.body)


@pytest.mark.parametrize("call", [
    lambda s, r: s.save([0, 1, 0]),                                          # an id given twice
    lambda s, r: s.save([0, 8]),                                             # outside the capacity
    lambda s, r: s.save([-1]),
    lambda s, r: s.save([4]),                                                # not opened
    lambda s, r: s.save([]),
    lambda s, r: s.save(list(range(257))),
    lambda s, r: s.save([0.5]),
    lambda s, r: s.load([0, 0], r),
    lambda s, r: s.load([0, 8], r),
    lambda s, r: s.load([0], r),                                             # two records for one id
    lambda s, r: s.load([0, 1, 2], r),
    lambda s, r: s.load([0, 1], (r.meta, r.body)),                           # not SessionRecords
    lambda s, r: s.load([0, 1], api.SessionRecords(r.meta, r.body[:, :-16])),    # wrong body shape
    lambda s, r: s.load([0, 1], api.SessionRecords(r.meta, np.concatenate([r.body, r.body], 1))),
    lambda s, r: s.load([0, 1], records_for((100, 4, 1, 3), 2)),             # another scale
    lambda s, r: s.load([0, 1], records_for((100, 2, 1, 4), 2)),             # another depth
    lambda s, r: s.load([0, 1], records_for((100, 2, 0, 3), 2)),             # local off
    lambda s, r: s.load([0, 1], records_for((7, 2, 1, 3), 2)),               # another latent size
    lambda s, r: s.load([0, 1], tampered(r, 1, hist_cur=2)),                 # a cursor behind the entries (record 1 has one)
    lambda s, r: s.load([0, 1], tampered(r, 1, hist_len=5, hist_cur=1)),
    lambda s, r: s.load([0, 1], tampered(r, 0, local_flags=4)),
    lambda s, r: s.load([0, 1], tampered(r, 0, magic=0)),
    lambda s, r: s.load([0, 1], tampered(r, 0, format=2)),
    lambda s, r: s.load([0, 1], tampered(r, 0, body_bytes=16)),
])
def test_invalid_input_raises_before_any_library_call(call):
    s, h = record_stub()
    rec = records_for((100, 2, 1, 3), 2)
    opened = set(s._opened)
    with pytest.raises(ValueError):
        call(s, rec)
    assert h.calls == [] and s._opened == opened


def test_session_records_refuse_what_is_no_record():
    rec = records_for((100, 0, 0, 0), 2)
    with pytest.raises(ValueError):
        api.SessionRecords(rec.meta, rec.body[:1])
    with pytest.raises(ValueError):
        api.SessionRecords(np.zeros(2, np.int32), rec.body)
    with pytest.raises(ValueError):
        api.SessionRecords(rec.meta, rec.body.reshape(-1))


# ---- 6. the file form --------------------------------------------------------------------------------------------------------------
def test_tobytes_frombytes_round_trip():
    rec = records_for((100, 2, 1, 3), 3, seed=5, sources={0, 2})
    data = rec.tobytes()
    bb = rec.body.shape[1]
    assert len(data) == 16 + 3 * (64 + bb) and data[:4] == b"IANR"
    assert list(np.frombuffer(data, "<i4", 3, 4)) == [1, 3, bb]
    back = api.SessionRecords.frombytes(data)
    assert back.meta.tobytes() == rec.meta.tobytes() and np.array_equal(back.body, rec.body)
    assert back.body.ctypes.data % 16 == 0 and back.body.flags.writeable and back.tobytes() == data
    one = api.SessionRecords.frombytes(rec[1].tobytes())
    assert len(one) == 1 and np.array_equal(one.body[0], rec.body[1]) and int(one.meta[0]["hist_len"]) == 1
    f, e = N.session_record_unpack(back.meta[2], back.body[2])            # and what is in the file is the session
    assert "SOURCE" in f and len(e) == 2
    for bad in (b"", data[:15], b"JUNK" + data[4:], data[:-1], data + b"\0", data[:4] + np.array([2], "<i4").tobytes() + data[8:]):
        with pytest.raises(ValueError):
            api.SessionRecords.frombytes(bad)
