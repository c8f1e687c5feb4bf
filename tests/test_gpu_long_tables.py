"""The six steps that share the polygon-table path (csrc/poly_table.h, k13_poly.h, k13_scan.h) on the long sparse table of
tests/long_tables.py: scans of more than one part over rows, polygons, tiles and items, 256-polygon blocks inside one row and
behind a long run of equal row_off entries, print windows that touch more rows than are staged (K13, K17) and hold thousands of
empty tiles (K20).  tests/test_long_tables_cpu.py asserts that the table has those shapes.  Every step through its own module's
checker: both C-ABI entries against the step's reference, exactly.  Needs a real MI355X."""
import numpy as np
import pytest

import long_tables as LT
from test_gpu_coco import check as k16_check
from test_gpu_polygon_audit import run_dev as k14_dev, same as k14_same
from test_gpu_polygon_raster import both as k21_both
from test_gpu_tile_labels import both as k20_both
from test_gpu_yolo_obb import check as k17_check
from test_gpu_yolo_seg import check as k13_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sel", [False, True])
def test_k13(native, sel):
    want = LT.k13_want(sel)
    got = k13_check(native, *LT.k13_table(sel))
    assert got[3] == want[3] and np.array_equal(got[0], want[0]) and len(want[3]) > 3 * 32768


def test_k17(native):
    want = LT.k17_want()
    got = k17_check(native, *LT.k13_table())                                  # with and without corners, and the _dev entry
    assert got[3] == want[3] and np.array_equal(got[2], want[2]) and got[5].shape == (len(want[2]), 8)


def test_k14(native):
    table, want = LT.k14_table(), LT.k14_want()
    k14_same(native.audit_polygons(*table), want)
    k14_same(k14_dev(table), want)
    assert want[3][:, 0].sum() == (table[3] >= 0).sum()


@pytest.mark.parametrize("flags", [1, 0])
def test_k16(native, flags):
    want = k16_check(native, LT.k16_table(), flags=flags, want=LT.k16_want(flags))
    assert want[2].sum() == (want[0] <= 1).sum() > 1000


@pytest.mark.parametrize("mode, max_tiles_per_row", [(0, 4096), (1, 4096), (0, 6)])
def test_k20(native, mode, max_tiles_per_row):
    want = k20_both(native, LT.k20_table(), LT.k20_params(mode, max_tiles_per_row), want=LT.k20_want(mode, max_tiles_per_row))
    assert (3 in want[0]) == (max_tiles_per_row == 6) and len(want[2]) > 4096 and len(want[-1]) > 8 * 8192


@pytest.mark.parametrize("max_pixels", [1 << 20, 12])
def test_k21(native, max_pixels):
    want = k21_both(native, LT.k21_table(), background=9, max_pixels=max_pixels, want=LT.k21_want(max_pixels))
    assert (3 in want[0]) == (max_pixels == 12) and len(want[-1]) > 10000
