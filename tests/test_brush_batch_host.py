"""The batched brush's host side without a GPU: the argument packer of IAN.imgrad_batch / IAN.brush_step_batch and the
ctypes mirrors of ian_brush_item / ian_photo_batch_args against the C header."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from neural_photo_editor_amd import lib as L
from neural_photo_editor_amd.api import BATCH_MAX, pack_brush_items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float_boxes_are_truncated_like_imgrad():
    items = pack_brush_items([[1.7, 2.2, 30.9, 40.0], [0.0, 0.0, 64.0, 64.0]], n_rgb=2)
    assert [(it.c1, it.r1, it.c2, it.r2) for it in items] == [(1, 2, 30, 40), (0, 0, 64, 64)]
    assert [it.gscale for it in items] == [1 + (30 - 1), 65.0]


def test_coef_and_gscale_are_formed_as_brush_step_forms_them():
    boxes = np.array([[0, 0, 4, 4], [10, 3, 17, 9], [5, 5, 5, 9]])
    weight = np.array([0.05, 0.3, 0.07])
    sign = np.array([-1.0, 1.0, -1.0])
    items = pack_brush_items(boxes, None, None, weight, sign)
    for it, b, w, s in zip(items, boxes, weight, sign):
        assert np.float32(it.coef).tobytes() == np.float32(s * w).tobytes()
        assert it.gscale == np.float32(1 + (b[2] - b[0]))
    scalar = pack_brush_items(boxes, None, None, 0.05, -1.0)
    assert all(np.float32(it.coef).tobytes() == np.float32(-1.0 * 0.05).tobytes() for it in scalar)


def test_modes_default_from_rgb():
    boxes = np.tile([0, 0, 8, 8], (3, 1))
    assert [it.mode for it in pack_brush_items(boxes, n_rgb=3)] == [1, 1, 1]
    assert [it.mode for it in pack_brush_items(boxes, n_rgb=None)] == [0, 0, 0]
    assert [it.mode for it in pack_brush_items(boxes, n_rgb=3, modes=[0, 1, 0])] == [0, 1, 0]


@pytest.mark.parametrize("kwargs", [
    dict(boxes=np.zeros((3, 3))),                                      # not (n,4)
    dict(boxes=np.zeros(4)),                                           # not 2-D
    dict(boxes=np.zeros((0, 4))),                                      # n = 0
    dict(boxes=np.zeros((BATCH_MAX + 1, 4))),                          # n = 257
    dict(boxes=np.zeros((3, 4)), n_rgb=2),                             # RGB batch of another size
    dict(boxes=np.zeros((3, 4)), modes=[0, 1]),                        # modes of another length
    dict(boxes=np.zeros((3, 4)), modes=[0, 2, 0]),                     # unknown mode
    dict(boxes=np.zeros((3, 4)), n_rgb=None, modes=[0, 1, 0]),         # mode 1 without RGB
    dict(boxes=np.zeros((3, 4)), weight=np.ones(2)),                   # weight of another length
    dict(boxes=np.zeros((3, 4)), sign=np.ones((3, 1))),                # sign of another shape
])
def test_malformed_arguments_raise_before_the_library(kwargs):
    with pytest.raises(ValueError):
        pack_brush_items(**kwargs)


def test_model_methods_validate_before_the_library():
    """The batched methods of the host class raise on malformed input without touching the handle (a stand-in object here)."""
    from neural_photo_editor_amd.api import IAN

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("the library was called")

    m = IAN.__new__(IAN)
    m._zdim, m._h = 100, NoLib()
    z = np.zeros((2, 100), np.float32)
    with pytest.raises(ValueError):
        m.imgrad_batch(np.zeros((2, 4)), z, None, modes=[1, 0])
    with pytest.raises(ValueError):
        m.imgrad_batch(np.zeros((3, 4)), z)                            # 3 boxes, 2 latents
    with pytest.raises(ValueError):
        m.brush_step_batch(np.zeros((2, 4)), np.zeros((2, 99), np.float32))
    with pytest.raises(ValueError):
        m.brush_step_batch(np.zeros((2, 4)), z, photo=(np.zeros((3, 64, 64), np.uint8), np.zeros((3, 64, 64), np.float32)))


def test_struct_mirrors_match_the_header(tmp_path):
    assert ctypes.sizeof(L.BrushItem) == 28
    assert L.BrushItem.coef.offset == 20 and L.BrushItem.gscale.offset == 24
    assert "ian_grad_batch" in L.EXPORTS and "ian_brush_step_batch" in L.EXPORTS
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    mirrors = {"ian_brush_item": L.BrushItem, "ian_photo_batch_args": L.PhotoBatchArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ian.h"', 'int main(void) {']
    for cname, cls in mirrors.items():
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    for line in filter(None, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")):
        cname, field, val = line.split()
        cls = mirrors[cname]
        assert (ctypes.sizeof(cls) if field == "size" else getattr(cls, field).offset) == int(val), (cname, field)
