"""The print kernels of K13, K16 and K17 at every byte phase of the text's address, on texts that more than one workgroup
prints: K13 and K16 cut the text into 32 KiB windows aligned to 16 bytes of its address, so two workgroups meet at a window edge
that moves with the phase; K17 prints a workgroup per 256 polygons, so 257 lines are two ranges that meet inside a 16-byte
chunk.  Through the `_dev` entries on torch tensors, the text inside a guarded buffer, byte for byte against the restatements
(tests/yolo_seg_ref.py, coco_ref.py, yolo_obb_ref.py).  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import coco_ref
import test_gpu_coco as k16
import test_gpu_yolo_obb as k17
import test_gpu_yolo_seg as k13
import yolo_obb_ref
import yolo_seg_ref

pytestmark = pytest.mark.gpu

WINDOW = 32 * 1024               # K13_WINDOW and K16_WINDOW
PHASES = range(16, 32)           # the text's offset in a 512-byte aligned buffer: every phase, and 16 guard bytes or more before it
K13_BYTES = 37568                # 64 rows of 4 lines of 2 + 8 * 18 bytes and the 3 "\n" between them
K16_POLYS, K16_BYTES = 142, 32884   # the fewest of these polygons (in twos per row) whose objects pass 32 KiB
K17_BYTES = 19274                # one row of 257 lines of 2 + 72 bytes and the 256 "\n" between them


def _polygons(seed, n_polys, n_pts):
    """n_polys polygons of n_pts vertices, all inside a 640 x 480 image"""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(8, 632, n_polys * n_pts), rng.uniform(8, 472, n_polys * n_pts)], 1).reshape(-1)
    return xy, np.arange(0, n_polys * n_pts + 1, n_pts, dtype=np.int32)


def _rows(n_rows, per_row, first_cid):
    return (np.arange(0, n_rows * per_row + 1, per_row, dtype=np.int32), np.full(n_rows, 640.0), np.full(n_rows, 480.0),
            (first_cid + np.arange(n_rows) % 50).astype(np.int32))       # two-digit class ids


@functools.lru_cache(maxsize=None)
def seg_case():
    xy, pt_off = _polygons(13, 64 * 4, 8)
    row_off, W, H, cid = _rows(64, 4, 10)
    t = (xy, pt_off, row_off, None, W, H, cid)
    return t, yolo_seg_ref.seg_arrays(*t)


@functools.lru_cache(maxsize=None)
def coco_case():
    xy, pt_off = _polygons(16, K16_POLYS, 8)
    row_off, W, H, _ = _rows(K16_POLYS // 2, 2, 10)
    t = (xy, pt_off, row_off, (1 + np.arange(K16_POLYS) % 7).astype(np.int32), W, H, np.zeros(len(W), np.uint8))
    return t, coco_ref.coco_arrays(*t, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def obb_case():
    xy, pt_off = _polygons(17, 257, 5)
    row_off, W, H, cid = _rows(1, 257, 10)
    t = (xy, pt_off, row_off, None, W, H, cid)
    return t, yolo_obb_ref.obb_arrays(*t)


@pytest.mark.parametrize("offset", PHASES)
def test_k13_at_every_phase(native, offset):
    t, want = seg_case()
    assert len(want[3]) == K13_BYTES > WINDOW            # two windows at every phase
    got = k13.check_dev(*t, offset=offset)
    assert all(np.array_equal(got[k], want[k]) for k in range(3)) and got[3] == want[3]


@pytest.mark.parametrize("offset", PHASES)
def test_k16_at_every_phase(native, offset):
    t, want = coco_case()
    assert len(want[3]) == K16_BYTES > WINDOW
    k16.same(k16.run_dev(t, offset=offset), want)


@pytest.mark.parametrize("offset", PHASES)
def test_k17_at_every_phase(native, offset):
    t, want = obb_case()
    assert int((want[2] <= 1).sum()) == 257 and len(want[3]) == K17_BYTES       # 257 written polygons: two polygon tiles
    k17.same(k17.check_dev(*t, offset=offset), want)
