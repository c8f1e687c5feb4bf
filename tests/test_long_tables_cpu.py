"""The long sparse table of tests/long_tables.py has the shapes tests/test_gpu_long_tables.py relies on: stated here on the
references' outputs, so that a change of the generator that loses one of them fails without a GPU.  The constants are the
kernels' (csrc/k13_seg.hip, k13_poly.h users, k16_coco.hip, k20_tile.hip)."""
import numpy as np

import long_tables as LT
from deal_yolo_daya_amd.core import processor as P

SCAN_TILE = 2048                 # K13_SCAN_TILE: values per part of k13_scan_inclusive
POLY_BLOCK = 256                 # polygons per workgroup of the lane-per-polygon kernels (poly_tile_rows)
K13_WINDOW, K13_ROWS_LDS = 32 * 1024, 1024
K16_WINDOW = 32 * 1024
K20_WINDOW, K20_PRINT_BLOCK = 8 * 1024, 64


def test_rows_and_polygons():
    xy, pt_off, row_off, W, H = LT.long_sparse()
    n, nb = len(W), len(pt_off) - 1
    count = np.diff(row_off)
    assert len(row_off) == n + 1 and row_off[0] == 0 and row_off[-1] == nb and len(xy) == 2 * pt_off[-1]
    assert n > 2 * SCAN_TILE and nb > SCAN_TILE                               # more than one part in every scan over rows or polygons
    big = int(np.argmax(count))
    assert count[big] > 2 * POLY_BLOCK
    blocks = np.arange(0, nb, POLY_BLOCK)                                      # a block of polygons wholly inside that row
    assert ((blocks >= row_off[big]) & (blocks + POLY_BLOCK <= row_off[big + 1])).any()
    assert count[0] == 0 and count[-1] > 0 and (count[n - 1 - 1500:n - 1] == 0).all()
    before = np.searchsorted(row_off, blocks, side="right") - 1               # the row of every block's first polygon
    run = np.asarray([(row_off[:r + 1] == row_off[r]).sum() for r in before])
    assert run.max() >= 500                                                    # a block that starts after hundreds of equal entries
    assert set(np.diff(pt_off).tolist()) == set(LT.LENGTHS)
    st = LT.size_status(W, H)
    assert np.array_equal(st, P._audit_sizes(W, H, n)[0]) and set(st.tolist()) == {0, 1, 2}
    for lo, hi in ((0, 1000), (1000, 2000), (2000, 4000), (4000, n)):          # rows of no size and of a fractional size in every region
        assert (W[lo:hi] == 0).any() and (W[lo:hi] != np.floor(W[lo:hi])).any() and np.isnan(H[lo:hi]).any()
    assert LT.long_sparse() is LT.long_sparse()


def _rows_of_windows(text_off, window, phase):
    """(first row, last row) of every print window, as k13_tile_rows_kernel finds them"""
    total, n = int(text_off[-1]), len(text_off) - 1
    out = []
    for t in range(-(-(total + phase) // window)):
        lo, hi = max(t * window - phase, 0), min((t + 1) * window - phase, total)
        ra = min(np.searchsorted(text_off, lo, side="right") - 1, n - 1)
        rb = min(np.searchsorted(text_off, hi - 1, side="right") - 1, n - 1)
        out.append((int(ra), int(rb)))
    return out


def test_k13_and_k17_windows_touch_more_rows_than_are_staged():
    text_off, flag, action, text = LT.k13_want()
    assert len(text) > 3 * K13_WINDOW and len(set(action.tolist())) >= 3 and set(flag.tolist()) == {0, 1, 2}
    starts = text_off[:-1]
    inside = [int(((starts >= b) & (starts < b + K13_WINDOW - 16)).sum()) for b in range(0, len(text), K13_WINDOW)]
    assert max(inside) > K13_ROWS_LDS + 16
    for phase in range(16):                                                    # the unstaged branch at every phase of the buffer
        assert max(rb - ra + 2 for ra, rb in _rows_of_windows(text_off, K13_WINDOW, phase)) > K13_ROWS_LDS, phase
    assert len(LT.k13_want(True)[3]) > 3 * K13_WINDOW and len(set(LT.k13_want(True)[2].tolist())) >= 3
    assert (255 in LT.k13_want(True)[2]) and (255 not in LT.k13_want(False)[2])
    want = LT.k17_want()
    assert len(want[3]) > 3 * K13_WINDOW and len(set(want[2].tolist())) >= 3


def test_k14_and_k16():
    cat = LT.k14_want()[0]
    assert len(set(cat.tolist())) >= 3 and 255 in cat
    for flags in (1, 0):
        action, area, kept, text = LT.k16_want(flags)
        assert len(set(action.tolist())) >= 3
    assert len(LT.k16_want(1)[3]) > 3 * K16_WINDOW


def test_k20_tiles():
    for mode in (0, 1):
        status, tile_off, lines, text_off, action = LT.k20_want(mode)[:5]
        assert len(lines) > 2 * SCAN_TILE and tile_off[-1] == len(lines) and len(set(action.tolist())) >= 3
        assert set(status.tolist()) == {0, 1, 2}
        full = np.flatnonzero(lines > 0)
        gap = np.diff(full) - 1                                                # tiles without text between two tiles with text
        at = text_off[full[1:]] % K20_WINDOW                                   # where the text goes on after the gap
        one_window = (at > 0) & (at < K20_WINDOW - 15)                         # not a window's first byte at any phase of the buffer
        assert (gap[one_window] > K20_PRINT_BLOCK).any()
    status = LT.k20_want(0, 6)[0]
    assert set(status.tolist()) == {0, 1, 2, 3} and len(LT.k20_want(0, 6)[2]) > 2 * SCAN_TILE


def test_k21_rows_and_pixels():
    status, pix_off, action, covered, owned, pixels = LT.k21_want()
    assert set(status.tolist()) == {0, 1, 2} and {0, 5} <= set(action.tolist()) and len(set(action.tolist())) >= 3
    assert (covered > owned).any() and len(pixels) == pix_off[-1] > 100000
    assert {9} < set(pixels.tolist())                                          # the background and painted values
    status = LT.k21_want(12)[0]
    assert set(status.tolist()) == {0, 1, 2, 3}
    painted = np.flatnonzero(status == 0)
    assert ((status == 3)[painted[0]:painted[-1]]).any()                       # too_large between painted rows
