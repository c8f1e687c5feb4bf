"""K21 (label masks, csrc/k21_raster.hip) through both C-ABI entries and export_masks_csv, against the restatement in
tests/polygon_raster_ref.py.  Exact: every output array and every pixel, with guard values round the outputs.  Needs a real
MI355X."""
import ctypes as C
import json
import math

import numpy as np
import pandas as pd
import pytest

import polygon_raster_ref as R
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu

NAMES = ("row_status", "pix_off", "action", "covered", "owned", "pixels")


def table(rows):
    """rows = [(W, H, [(val, [(x, y)])])] -> (xy, pt_off, row_off, val, width, height)"""
    xy, pt_off, row_off, val, W, H = [], [0], [0], [], [], []
    for w, h, polys in rows:
        for v, pts in polys:
            xy += [c for p in pts for c in p]
            pt_off.append(pt_off[-1] + len(pts))
            val.append(v)
        row_off.append(len(val))
        W.append(w)
        H.append(h)
    return (np.asarray(xy, np.float64), np.asarray(pt_off, np.int32), np.asarray(row_off, np.int32), np.asarray(val, np.int32),
            np.asarray(W, np.float64), np.asarray(H, np.float64))


def random_rows(rng, n_rows, max_polys=8, max_pts=45, max_size=96, values=(1, 2, 200)):
    rows = []
    for _ in range(n_rows):
        w, h = int(rng.integers(1, max_size + 1)), int(rng.integers(1, max_size + 1))
        wide = rng.random() < 0.2                                         # about one row in five reaches outside the image
        polys = []
        for _ in range(int(rng.integers(0, max_polys + 1))):
            m = int(rng.integers(1, max_pts + 1)) if rng.random() < 0.3 else int(rng.integers(2, 9))
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            r = rng.choice([4.0, 20.0, 90.0])
            pts = np.stack([cx + rng.uniform(-r, r, m), cy + rng.uniform(-r, r, m)], axis=1)
            if not wide:
                pts = np.clip(pts, 0, [w, h])
            kind = rng.random()
            if kind < 0.3:
                pts = np.round(pts)                                       # vertices on pixel corners, repeated vertices
            elif kind < 0.5:
                pts = np.round(pts) + 0.5                                 # vertices on pixel centres
            if rng.random() < 0.03:
                pts[rng.integers(0, m), rng.integers(0, 2)] = rng.choice([np.nan, np.inf, 2.0 ** 43])
            v = -1 if rng.random() < 0.1 else int(rng.choice(values))
            polys.append((v, [tuple(p) for p in pts.tolist()]))
        if rng.random() < 0.08:
            w = rng.choice([0.0, w + 0.5, math.nan, -3.0, 5000.0])        # rows that are not rasterised
        rows.append((w, h, polys))
    return rows


def same(got, want, names=NAMES):
    for g, w, what in zip(got, want, names):
        assert np.asarray(g).dtype == np.asarray(w).dtype and np.array_equal(g, w), what


def run_dev(t, background=0, max_pixels=1 << 26, phase=0, measure_only=False, pix_cap=None, hz=None):
    """the _dev entry on torch tensors: outputs at odd offsets inside guarded buffers, the pixels at `phase` bytes past a 16-byte
    boundary -> (the six outputs, return code, *out_total).  hz: the harness of tests/stream_contract.py (its decoys in the
    table's order), armed anew for both calls; without one the calls go to torch's current stream"""
    import torch
    from deal_yolo_daya_amd import _native
    from stream_contract import PLAIN

    hz = hz or PLAIN
    xy, pt_off, row_off, val, W, H = t
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    n, nb, npnt = len(W), len(val), len(xy) // 2
    d_xy = torch.zeros(len(xy) + 4, dtype=torch.float64, device=dev)
    d_xy[2:2 + len(xy)] = up(xy)
    d_pt, d_row, d_val, d_w, d_h = up(pt_off), up(row_off), up(val), up(W), up(H)
    g8, g64 = 0xA5, -7
    status = torch.full((n + 2,), g8, dtype=torch.uint8, device=dev)
    act = torch.full((nb + 2,), g8, dtype=torch.uint8, device=dev)
    pix_off = torch.full((n + 3,), g64, dtype=torch.int64, device=dev)
    cov, own = (torch.full((nb + 2,), g64, dtype=torch.int64, device=dev) for _ in range(2))
    L = _native.lib()
    total = C.c_int64(-1)
    hz.arm([d_xy[2:2 + len(xy)], d_pt, d_row, d_val, d_w, d_h])
    hz.watch(status, act, pix_off, cov, own)

    def call(pix_ptr, cap):
        return hz.call(L.dyd_rasterize_polygons_dev, d_xy.data_ptr() + 16, d_pt.data_ptr(), d_row.data_ptr(), d_val.data_ptr(),
                       d_w.data_ptr(), d_h.data_ptr(), n, nb, npnt, background, max_pixels, status.data_ptr() + 1,
                       pix_off.data_ptr() + 8, act.data_ptr() + 1, cov.data_ptr() + 8, own.data_ptr() + 8,
                       pix_ptr, cap, C.byref(total))

    rc = call(None, 0)
    assert rc == 0, L.dyd_last_error()
    torch.cuda.synchronize()
    assert (cov == g64).all() and (own == g64).all(), "measure mode touched the counters"
    size = total.value
    pixels = np.zeros(0, np.uint8)
    if not measure_only:
        cap = size if pix_cap is None else pix_cap
        buf = torch.full((64 + 16 + size + 64,), 0x7e, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        at = 64 + phase
        hz.watch(buf)
        rc = call(buf.data_ptr() + at, cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        if rc == 0:
            pixels = out[at:at + size].copy()
            assert (out[:at] == 0x7e).all() and (out[at + size:] == 0x7e).all(), "write outside the pixels"
        else:
            assert (out == 0x7e).all()
    hz.restore()
    arrays = []
    for a, fill in ((status, g8), (pix_off, g64), (act, g8), (cov, g64), (own, g64)):
        a = a.cpu().numpy()
        assert a[0] == fill and a[-1] == fill, "write outside the outputs"
        arrays.append(a[1:len(a) - 1])
    return (*arrays, pixels), rc, total.value


def both(native, t, background=0, max_pixels=1 << 26, want=None):
    want = R.raster_arrays(*t, background, max_pixels) if want is None else want
    same(native.rasterize_polygons(*t, background, max_pixels), want)
    got, rc, total = run_dev(t, background, max_pixels)
    assert rc == 0 and total == len(want[-1])
    same(got, want)
    return want


def option(native, strip=0, crossings=0):
    native.check(native.lib().dyd_set_option(b"k21_strip", strip), "opt")
    native.check(native.lib().dyd_set_option(b"k21_crossings", crossings), "opt")


@pytest.fixture(autouse=True)
def default_options(native):
    yield
    option(native)


def blob(rng, cx, cy, r, m):
    a = np.sort(rng.uniform(0, 2 * math.pi, m))
    rad = rng.uniform(0.4 * r, r, m)
    return [(cx + rr * math.cos(t), cy + rr * math.sin(t)) for t, rr in zip(a.tolist(), rad.tolist())]


# ----------------------------------------------------------------------------------------------- shapes
def test_widths_and_heights(native):
    rng = np.random.default_rng(3)
    rows = []
    for w in (1, 7, 63, 64, 65, 130):
        for h in (1, 5):
            rows.append((w, h, [(5, blob(rng, w / 2, h / 2, max(w, h) / 2 + 1, 7)), (9, [(0.0, 0.0), (w - 0.25, h / 2)]),
                                (6, blob(rng, w * 0.7, h * 0.4, w / 3 + 1, 5))]))
    want = both(native, table(rows), background=77)
    assert want[0].tolist() == [0] * 12 and (want[3] > 0).sum() >= 24 and set(np.unique(want[-1]).tolist()) >= {5, 6, 9}


def test_every_alignment_of_the_pixel_pointer(native):
    rng = np.random.default_rng(4)
    t = table([(9, 3, [(3, blob(rng, 4, 1.5, 4, 6)), (8, [(5.0, 0.0), (9.0, 2.0)])]), (9, 3, [(4, [(0.0, 0.0), (4.0, 3.0)])])])
    want = R.raster_arrays(*t, 1)
    for phase in range(16):
        got, rc, total = run_dev(t, 1, phase=phase)
        assert rc == 0 and total == 54, phase
        same(got, want)


@pytest.mark.parametrize("w", [64, 65, 200])
def test_strips(native, w):
    option(native, strip=64)
    rng = np.random.default_rng(w)
    polys = [(1, blob(rng, w / 2, 6, w / 2, 11)),                               # crosses every strip
             (2, [(w - 4.0, 5.0), (float(w), 9.0)]),                               # the last columns
             (3, [(66.0, 1.0), (90.0, 11.0)]), (4, [(-5.0, 3.0), (w + 5.0, 4.2)])]    # only in the second strip; past both ends
    want = both(native, table([(w, 12, polys), (3, 2, [(9, [(0.0, 0.0), (3.0, 2.0)])])]))
    assert (want[4][[0, 1, 3]] > 0).all() and (want[4][2] > 0) == (w > 66)


def test_a_full_crossing_list_is_applied_and_emptied(native):
    option(native, crossings=8)
    comb = [(0.0, 0.0)]
    for k in range(40):                                                        # 40 teeth: 80 crossings on a scanline
        comb += [(3.0 * k + 0.5, 10.0), (3.0 * k + 1.5, 1.0), (3.0 * k + 2.5, 10.0)]
    comb.append((125.0, 0.0))
    rng = np.random.default_rng(6)
    want = both(native, table([(125, 12, [(1, comb), (2, blob(rng, 60, 6, 30, 9))])]))
    assert want[3][0] > 300
    option(native, crossings=1)
    both(native, table([(125, 12, [(1, comb)])]))


@pytest.mark.parametrize("m", [2, 3, 64, 65, 300])
def test_edge_chunks(native, m):
    rng = np.random.default_rng(m)
    pts = [(3.0, 2.0), (50.0, 41.0)] if m == 2 else blob(rng, 30, 25, 28, m)
    want = both(native, table([(61, 50, [(1, pts), (2, blob(rng, 30, 25, 10, 5))])]))
    assert want[3][0] > 50


def test_ownership(native):
    nested = [(1, [(2.0, 2.0), (30.0, 30.0)]), (2, [(6.0, 6.0), (26.0, 26.0)]), (3, [(10.0, 10.0), (20.0, 20.0)])]
    partly = [(4, [(0.0, 34.0), (20.0, 44.0)]), (4, [(12.0, 38.0), (32.0, 47.0)])]   # the same val: ownership stays by polygon
    want = both(native, table([(33, 48, nested + partly), (33, 48, nested[::-1] + partly[::-1])]))
    assert want[3].tolist() == [784, 400, 100, 200, 180] + [100, 400, 784, 180, 200]
    assert want[4].tolist() == [384, 300, 100, 152, 180] + [0, 0, 784, 132, 200]


def test_unselected_empty_and_bad(native):
    box = [(1.0, 1.0), (4.0, 4.0)]
    t = table([(6, 5, [(-1, box), (-5, box)])])                                # all unselected: the mask is background
    want = both(native, t, background=9)
    assert want[2].tolist() == [255, 255] and (want[-1] == 9).all() and len(want[-1]) == 30
    t = table([(6, 5, []), (4, 4, [(1, box)]), (3, 3, [])])                    # rows with no polygons
    want = both(native, t, background=2)
    assert want[1].tolist() == [0, 30, 46, 55] and (want[-1][:30] == 2).all()
    none = (np.zeros(0), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    want = both(native, none)                                                  # n_rows == 0
    assert want[1].tolist() == [0] and len(want[-1]) == 0
    want = both(native, table([(5, 4, []), (2, 2, [])]), background=255)       # n_polys == 0
    assert (want[-1] == 255).all() and len(want[-1]) == 24
    bad = table([(8, 8, [(1, [(1.0, 1.0), (math.nan, 3.0), (5.0, 5.0)]), (2, [(3.0, 3.0)]), (3, []), (4, [(0.0, 0.0), (2.0 ** 43, 4.0)]),
                         (5, [(-2.0 ** 42, -2.0 ** 42), (2.0 ** 42, -2.0 ** 42), (2.0 ** 42, 2.0 ** 42), (-2.0 ** 42, 2.0 ** 42)]), (6, [(0.0, 0.0), (math.inf, 1.0)])])])
    want = both(native, bad)
    assert want[2].tolist() == [2, 3, 3, 2, 0, 2] and want[3].tolist() == [0, 0, 0, 0, 64, 0]


def test_row_status_between_painted_rows(native):
    box = [(1, [(0.0, 0.0), (3.0, 3.0)])]
    t = table([(4, 4, box), (0, 4, box), (4.5, 4, box), (4, 4, box), (6, 3, box), (5, 4, box), (17, 1, box), (1, 17, box), (2, 8, box)])
    want = both(native, t, max_pixels=16)
    assert want[0].tolist() == [0, 1, 2, 0, 3, 3, 3, 3, 0] and want[1].tolist() == [0, 16, 16, 16, 32, 32, 32, 32, 32, 48]
    assert want[2].tolist() == [0, 5, 5, 0, 5, 5, 5, 5, 0]


def test_measure_only_and_a_pixel_cap_that_is_too_small(native):
    t = table(random_rows(np.random.default_rng(8), 12))
    want = R.raster_arrays(*t)
    assert len(want[-1]) > 1000
    got, rc, total = run_dev(t, measure_only=True)                             # run_dev checks the counters' guards
    assert rc == 0 and total == len(want[-1])
    same(got[:3], want[:3], NAMES[:3])
    assert (got[3] == -7).all() and (got[4] == -7).all()
    got, rc, total = run_dev(t, pix_cap=len(want[-1]) - 1)
    assert rc == -5 and total == len(want[-1])                                 # DYD_ERR_RANGE with the exact size
    assert b"too small" in native.lib().dyd_last_error()
    same(got[:3], want[:3], NAMES[:3])
    assert (got[3] == -7).all() and (got[4] == -7).all()                       # no counter written


@pytest.mark.parametrize("bad", [dict(background=-1), dict(background=256), dict(max_pixels=0), dict(max_pixels=2 ** 30 + 1), dict(val=256)])
def test_invalid_arguments_are_the_argument_error(native, bad):
    xy, pt_off, row_off, val, W, H = table([(20, 10, [(bad.get("val", 1), [(5.0, 2.0), (15.0, 8.0)])])])
    kw = dict(background=0, max_pixels=1 << 20)
    kw.update({k: v for k, v in bad.items() if k != "val"})
    out = [np.zeros(8, d) for d in (np.uint8, np.int64, np.uint8, np.int64, np.int64)]
    pixels, total = C.c_void_p(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    L = native.lib()
    rc = L.dyd_rasterize_polygons(p(xy), p(pt_off), p(row_off), p(val), p(W), p(H), 1, kw["background"], kw["max_pixels"],
                                  *[p(a) for a in out], C.byref(pixels), C.byref(total))
    assert rc == -1 and b"invalid argument" in L.dyd_last_error() and not pixels.value
    if "val" not in bad:
        rc = L.dyd_rasterize_polygons_dev(None, None, None, None, None, None, 0, 0, 0, kw["background"], kw["max_pixels"],
                                          *[None] * 6, 0, C.byref(total), None)
        assert rc == -1
    assert L.dyd_rasterize_polygons_dev(None, None, None, None, None, None, -1, 0, 0, 0, 16, *[None] * 6, 0, C.byref(total), None) == -1
    assert L.dyd_rasterize_polygons_dev(None, None, None, None, None, None, 1, 0, 0, 0, 16, *[None] * 6, 0, C.byref(total), None) == -1


# ----------------------------------------------------------------------------------------------- random tables
def test_random_table(native):
    rng = np.random.default_rng(1)
    t = table(random_rows(rng, 200))
    want = both(native, t, background=255, max_pixels=96 * 96)
    assert {0, 2, 3, 5, 255} <= set(want[2].tolist()) and {0, 1, 2, 3} <= set(want[0].tolist())
    assert (want[3] > want[4]).any() and ((want[3] > 0) & (want[4] == 0)).any() and len(want[-1]) > 200000
    option(native, strip=17, crossings=3)                                      # the same table over narrow strips and a short list
    same(native.rasterize_polygons(*t, 255, 96 * 96), want)


# ----------------------------------------------------------------------------------------------- the compiled limits
# All at the default options: strips of 1,024 columns (K21_STRIP), a list of 256 crossings (K21_CROSSINGS), 2^20 paint workgroups
# (K21_MAX_GRID).  tests/test_polygon_raster_cpu.py runs the first two tables through the mapping's transliteration.
STRIP, CROSSINGS, MAX_GRID = 1024, 256, 1 << 20


def full_strip_rows(widths=(1023, 1024, 1025, 2049)):
    """rows of height 3: a blob across the whole width, a box on the last three columns, a box across the first strip's end"""
    rng = np.random.default_rng(12)
    return [(w, 3, [(1, blob(rng, w / 2, 1.5, w / 2, 9)), (2, [(w - 3.0, 0.0), (float(w), 3.0)]), (3, [(1020.0, 1.0), (1030.0, 3.0)])])
            for w in widths]


def full_list_rows(n_teeth=150):
    """a comb of n_teeth teeth: 3 * n_teeth + 2 vertices, 2 * n_teeth crossings on the scanlines 1 to 9, and a blob on top"""
    comb = [(0.0, 0.0)]
    for k in range(n_teeth):
        comb += [(3.0 * k + 0.5, 10.0), (3.0 * k + 1.5, 1.0), (3.0 * k + 2.5, 10.0)]
    w = 3 * n_teeth + 5
    comb.append((float(w), 0.0))
    return [(w, 12, [(1, comb), (2, blob(np.random.default_rng(13), w / 2, 6, 100, 9))])]


def test_default_strip_widths(native):
    want = both(native, table(full_strip_rows()), background=5)
    assert (want[3] > 0).all() and (want[4] < want[3]).any() and len(want[-1]) == 3 * (1023 + 1024 + 1025 + 2049)
    for w in (STRIP, STRIP + 1):                             # a full strip, and a second strip of one pixel, at every phase
        t = table(full_strip_rows((w,)))
        want = R.raster_arrays(*t, 5)
        assert (want[3] > 0).all()
        for phase in range(16):
            got, rc, total = run_dev(t, 5, phase=phase)
            assert rc == 0 and total == 3 * w, phase
            same(got, want)


def test_more_crossings_than_the_default_list_holds(native):
    rows = full_list_rows()
    assert len(rows[0][2][0][1]) == 452 and rows[0][0] == 455
    want = both(native, table(rows))
    assert want[3][0] > 3000 and want[4][0] < want[3][0] and 2 * 150 > CROSSINGS


def test_more_items_than_paint_workgroups(native):
    H = 2 ** 20 - 3
    rng = np.random.default_rng(14)
    t = table([(1, H, [(1, [(0.0, 10.0), (1.0, H - 10.0)]), (2, [(0.0, 100.0), (1.0, 500000.25), (0.2, 900000.0)])]),
               (70, 40, [(3, blob(rng, 35, 20, 30, 9)), (4, [(60.0, 2.0), (70.0, 39.0)])])])
    n_items = sum(int(h) * -(-int(w) // STRIP) for w, h in zip(t[4], t[5]))
    assert n_items == MAX_GRID + 37                          # workgroups 0 to 36 take a scanline of each row
    want = both(native, t, background=7, max_pixels=1 << 26)
    assert set(np.unique(want[-1]).tolist()) == {1, 2, 3, 4, 7} and len(want[-1]) == H + 2800
    assert want[3][0] == 2 ** 20 - 23 and want[4][0] < want[3][0]


def test_no_row_is_rasterised(native):
    box, tri = [(1.0, 1.0), (4.0, 4.0)], [(0.0, 0.0), (3.0, 1.0), (2.0, 4.0)]
    polys = [(1, box), (-1, box), (2, tri)]
    t = table([(0, 5, polys), (4.5, 4, polys), (5000, 5000, polys)])
    want = both(native, t, background=3, max_pixels=1 << 20)
    assert want[0].tolist() == [1, 2, 3] and want[1].tolist() == [0, 0, 0, 0] and len(want[-1]) == 0
    assert want[2].tolist() == [5, 255, 5] * 3 and not want[3].any() and not want[4].any()
    got = native.rasterize_polygons(*t, 3, 1 << 20)
    assert not got[3].any() and not got[4].any() and len(got[5]) == 0
    got, rc, total = run_dev(t, 3, 1 << 20, pix_cap=0)       # a pixel pointer that is not NULL and no room behind it
    assert rc == 0 and total == 0
    same(got, want)


BIG = 2.0 ** 40
SKEWED = [[(-BIG, -BIG + 1), (BIG + 3, BIG), (7.0, 2 * BIG)], [(-2 * BIG + 5, 3.0), (2 * BIG, -BIG + 11), (BIG + 1, 4 * BIG)],
          [(-4 * BIG, 2 * BIG + 7), (4 * BIG - 9, -2 * BIG), (13.0, -4 * BIG + 1)], [(BIG + 20, -BIG), (-BIG, BIG + 45), (-2 * BIG - 3, -2 * BIG)],
          [(-BIG, -3 * BIG), (3 * BIG + 1, BIG + 17), (-BIG - 30, BIG)], [(2 * BIG, 2 * BIG + 1), (-2 * BIG + 60, -2 * BIG), (4 * BIG, -BIG + 25)]]


def test_large_skewed_polygons(native):
    """vertices of 2^40 to 2^42 whose edges cross a 50 x 50 image at a slant: xs is a rounded quotient on every scanline"""
    polys = [(k + 1, tri) for k, tri in enumerate(SKEWED)] + [(9, blob(np.random.default_rng(15), 25, 25, 20, 9))]
    want = both(native, table([(50, 50, polys)]))
    cov = want[3][:len(SKEWED)]
    assert ((cov > 0) & (cov < 2500)).sum() >= 2 and (cov == 2500).any() and want[3][-1] > 0
    for k, tri in enumerate(SKEWED):                         # and each alone, where nothing hides it
        both(native, table([(50, 50, [(k + 1, tri)])]))


# ----------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("mode, order", [("semantic", "annotation"), ("semantic", "large_first"), ("instance", "annotation"),
                                         ("instance", "large_first")])
def test_export_masks_csv_end_to_end(native, tmp_path, mode, order):
    from PIL import Image

    rng = np.random.default_rng(21)
    names = ["a", "b", "c"]
    cells, rows = [], random_rows(rng, 30, max_polys=5, max_pts=12, max_size=60, values=(0, 1, 2))
    for _, _, polys in rows:
        cells.append(json.dumps({"objects": [{"name": names[max(v, 0)], "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}
                                             for v, pts in polys if all(map(math.isfinite, sum(pts, ())))]}))
    df = pd.DataFrame({"source": [f"im{k}.jpg" for k in range(30)], P.ANNOTATION_COL: cells,
                       "width": [r[0] for r in rows], "height": [r[1] for r in rows]})
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    res = P.export_masks_csv(src, tmp_path / "ds", mode=mode, order=order, classes=names, batch_pixels=20000,
                             problems_csv=tmp_path / "p.csv")
    back = pd.read_csv(src, encoding="utf-8-sig")

    from helpers import OracleBackend
    ref_be = type("RefBackend", (OracleBackend,), {"rasterize_polygons": staticmethod(R.raster_arrays)})()
    want = P.polygon_masks(back[P.ANNOTATION_COL], back["width"], back["height"], mode=mode, order=order, classes=names,
                           backend=ref_be, sources=back["source"].to_numpy())
    assert {k: res[k] for k in want.totals if k != "python_cells"} == {k: v for k, v in want.totals.items() if k != "python_cells"}
    written = 0
    for i, m in enumerate(want.masks):
        path = tmp_path / "ds" / "masks" / "train" / f"{P._safe_image_stem(f'im{i}.jpg', i)}.png"
        assert path.exists() == (m is not None)
        if m is not None:
            with Image.open(path) as im:
                assert np.array_equal(np.asarray(im), m), i
            written += 1
    assert written > 20 and res["mask_files"] == written and res["painted"] > 20
    manifest = pd.read_csv(tmp_path / "ds" / "masks_train.csv", encoding="utf-8-sig", keep_default_na=False)
    assert manifest["status"].tolist() == want.rows["status"].tolist()
    for c in ("polygons", "painted", "hidden", "empty"):
        assert manifest[c].tolist() == want.rows[c].tolist(), c
    classes = pd.read_csv(tmp_path / "ds" / "mask_classes.csv", encoding="utf-8-sig")
    assert classes.drop(columns="share").values.tolist() == want.per_class.drop(columns="share").values.tolist()
    assert np.allclose(classes["share"].to_numpy(), want.per_class["share"].to_numpy(), rtol=1e-12, atol=0)
    problems = pd.read_csv(tmp_path / "p.csv", encoding="utf-8-sig")
    bad = want.polygons[want.polygons["result"].isin(("hidden", "empty", "bad_coords", "too_few_points"))]
    assert problems[["row", "object", "result"]].values.tolist() == bad[["row", "object", "result"]].values.tolist()
