"""K23 (COCO run-length masks, csrc/k23_rle.hip) through both C-ABI entries and export_coco_csv(segmentation="rle"), against
the restatement in tests/polygon_rle_ref.py and against K21 on the device.  Exact: every output array, run and byte, with guard
values round the outputs of the device entry and the outputs at odd offsets.  Needs a real MI355X."""
import ctypes as C
import json
import math

import numpy as np
import pandas as pd
import pytest

import long_tables as LT
import polygon_raster_ref as K21
import polygon_rle_ref as R
from test_gpu_polygon_raster import blob, random_rows, table
from deal_yolo_daya_amd.core import processor as P
from deal_yolo_daya_amd.core import utils as U

pytestmark = pytest.mark.gpu

NAMES = ("row_status", "action", "area", "bbox", "run_off", "runs", "text_off", "text")
RANGE, INVALID = -5, -1


def same(got, want, names=NAMES):
    for g, w, what in zip(got, want, names):
        if isinstance(w, bytes):
            assert bytes(g) == w, what
        else:
            assert np.asarray(g).dtype == np.asarray(w).dtype and np.array_equal(g, w), what


def run_dev(t, max_pixels=1 << 26, upto="text", runs_cap=None, text_cap=None, phase=1):
    """the _dev entry on torch tensors, as a caller uses it: measure (no runs), then runs without text, then everything.  Outputs
    sit at odd offsets inside guarded buffers, the text `phase` bytes past a 16-byte boundary.  upto: "measure" | "runs" | "text"
    -> (the eight outputs as far as they were asked for, return code of the last call, run total, text total)"""
    import torch
    from deal_yolo_daya_amd import _native

    xy, pt_off, row_off, sel, W, H = t
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    n, nb, npnt = len(W), len(sel), len(xy) // 2
    d_xy = torch.zeros(len(xy) + 4, dtype=torch.float64, device=dev)
    d_xy[2:2 + len(xy)] = up(xy)
    d_pt, d_row, d_sel, d_w, d_h = up(pt_off), up(row_off), up(sel), up(W), up(H)
    g8, g32, g64 = 0xA5, -9, -7
    status = torch.full((n + 2,), g8, dtype=torch.uint8, device=dev)
    act = torch.full((nb + 2,), g8, dtype=torch.uint8, device=dev)
    area = torch.full((nb + 2,), g64, dtype=torch.int64, device=dev)
    bbox = torch.full((4 * nb + 2,), g32, dtype=torch.int32, device=dev)
    run_off, text_off = (torch.full((nb + 3,), g64, dtype=torch.int64, device=dev) for _ in range(2))
    L = _native.lib()
    n_runs, n_text = C.c_int64(-1), C.c_int64(-1)
    torch.cuda.synchronize()                 # the entry takes no stream: the inputs are complete before it is called

    def call(runs_ptr, r_cap, text_ptr, t_cap, with_text_off=True):
        return L.dyd_polygon_rle_dev(d_xy.data_ptr() + 16, d_pt.data_ptr(), d_row.data_ptr(), d_sel.data_ptr(), d_w.data_ptr(),
                                     d_h.data_ptr(), n, nb, npnt, max_pixels, status.data_ptr() + 1, act.data_ptr() + 1,
                                     area.data_ptr() + 8, bbox.data_ptr() + 4, run_off.data_ptr() + 8, runs_ptr, r_cap,
                                     text_off.data_ptr() + 8 if with_text_off else None, text_ptr, t_cap, C.byref(n_runs),
                                     C.byref(n_text))

    def outputs():
        arrays = []
        for a, fill in ((status, g8), (act, g8), (area, g64), (bbox, g32), (run_off, g64), (text_off, g64)):
            a = a.cpu().numpy()
            assert a[0] == fill and a[-1] == fill, "write outside the outputs"
            arrays.append(a[1:len(a) - 1])
        arrays[3] = arrays[3].reshape(-1, 4)
        return arrays

    rc = call(None, 0, None, 0, with_text_off=False)                     # the blocking entry: nothing to wait for afterwards
    assert rc == 0, L.dyd_last_error()
    st, ac, ar, bb, ro, to = outputs()
    assert (to == g64).all() and n_text.value == 0, "measure mode touched the text offsets"
    total_runs = n_runs.value
    assert total_runs == ro[-1]
    if upto == "measure":
        return (st, ac, ar, bb, ro), rc, total_runs, 0
    cap = total_runs if runs_cap is None else runs_cap
    guard32 = 0x7e7e7e7e
    rbuf = torch.full((16 + total_runs + 16,), guard32, dtype=torch.int32, device=dev)
    rat = 5                                                               # 4-byte aligned, not 8
    rc = call(rbuf.data_ptr() + 4 * rat, cap, None, 0)
    out = rbuf.cpu().numpy()
    if rc != 0:
        assert (out == guard32).all(), "runs written although the buffer was too small"
        st, ac, ar, bb, ro, to = outputs()
        assert (to == g64).all()
        return (st, ac, ar, bb, ro), rc, n_runs.value, n_text.value
    assert (out[:rat] == guard32).all() and (out[rat + total_runs:] == guard32).all(), "write outside the runs"
    runs = out[rat:rat + total_runs].view(np.uint32).copy()
    st, ac, ar, bb, ro, to = outputs()
    total_text = n_text.value
    assert total_text == to[-1] and n_runs.value == total_runs
    if upto == "runs":
        return (st, ac, ar, bb, ro, runs, to), rc, total_runs, total_text
    cap = total_text if text_cap is None else text_cap
    tbuf = torch.full((64 + 16 + total_text + 64,), 0x7e, dtype=torch.uint8, device=dev)
    assert tbuf.data_ptr() % 16 == 0
    at = 64 + phase
    rbuf.fill_(guard32)
    rc = call(rbuf.data_ptr() + 4 * rat, total_runs, tbuf.data_ptr() + at, cap)
    out = tbuf.cpu().numpy()
    if rc != 0:
        assert (out == 0x7e).all(), "text written although the buffer was too small"
        return (st, ac, ar, bb, ro, runs, to), rc, n_runs.value, n_text.value
    assert (out[:at] == 0x7e).all() and (out[at + total_text:] == 0x7e).all(), "write outside the text"
    text = out[at:at + total_text].tobytes()
    again = rbuf.cpu().numpy()
    assert np.array_equal(again[rat:rat + total_runs].view(np.uint32), runs) and (again[:rat] == guard32).all()
    st, ac, ar, bb, ro, to = outputs()
    return (st, ac, ar, bb, ro, runs, to, text), rc, n_runs.value, n_text.value


def both(native, t, max_pixels=1 << 26, want=None, phase=1):
    want = R.rle_arrays(*t, max_pixels) if want is None else want
    same(native.polygon_rle(*t, max_pixels), want)
    got, rc, n_runs, n_text = run_dev(t, max_pixels, phase=phase)
    assert rc == 0 and n_runs == len(want[5]) and n_text == len(want[7])
    same(got, want)
    return want


def runs_of(want, p):
    return want[5][want[4][p]:want[4][p + 1]].tolist()


def option(native, strip=0, crossings=0, grid=0, band=0):
    for key, v in ((b"k23_strip", strip), (b"k23_crossings", crossings), (b"k23_grid", grid), (b"k23_band", band)):
        native.check(native.lib().dyd_set_option(key, v), "opt")


@pytest.fixture(autouse=True)
def default_options(native):
    yield
    option(native)


# ----------------------------------------------------------------------------------------------- column continuation
def test_column_continuation_by_hand(native):
    t = table([(4, 3, [(0, [(1.0, 0.0), (3.0, 3.0)]), (0, [(0.0, 0.0), (4.0, 3.0)]), (0, [(9.0, 9.0), (12.0, 12.0)]),
                       (0, [(1.0, 0.0), (3.0, 2.0)]), (0, [(1.0, 1.0), (3.0, 3.0)])])])
    want = both(native, t)
    assert [runs_of(want, p) for p in range(5)] == [[3, 6, 3], [0, 12], [12], [3, 2, 1, 2, 4], [4, 2, 1, 2, 3]]
    assert want[2].tolist() == [6, 12, 0, 4, 4] and want[3].tolist()[:3] == [[1, 0, 2, 3], [0, 0, 4, 3], [0, 0, 0, 0]]


@pytest.mark.parametrize("strip, band", [(0, 0), (64, 0), (17, 0), (64, 1), (17, 2)])     # 0: the default, 1,024 columns by 64 lines
@pytest.mark.parametrize("w", [64, 65, 130])
def test_full_height_columns_across_lanes_and_strips(native, strip, band, w):
    option(native, strip=strip, band=band)
    h = 3.0
    boxes = [[(62.0, 0.0), (66.0, h)], [(0.0, 0.0), (float(w), h)], [(63.0, 0.0), (64.0, h)], [(w - 1.0, 0.0), (float(w), h)],
             [(16.0, 0.0), (18.0, h)], [(33.0, 0.0), (35.0, h)], [(-4.0, -4.0), (w + 4.0, 9.0)], [(200.0, 0.0), (210.0, h)]]
    rng = np.random.default_rng(w)
    polys = [(0, b) for b in boxes] + [(0, blob(rng, w / 2, 1.5, w / 2, 9)), (0, [(60.0, 0.0), (70.0, 3.0), (62.0, 3.0), (68.0, 0.0)])]
    want = both(native, table([(w, 3, polys)]))
    assert runs_of(want, 1) == [0, 3 * w] and runs_of(want, 6) == [0, 3 * w] and runs_of(want, 7) == [3 * w]
    assert runs_of(want, 2) == ([189, 3, 3 * w - 192] if w > 64 else [189, 3])
    assert runs_of(want, 0) == ([186, 3 * min(4, w - 62), 3 * w - 186 - 3 * min(4, w - 62)] if w > 66 else [186, 3 * (w - 62)])


def test_default_strip_widths(native):
    """strips of 1,024 columns (K23_STRIP): 16 words per lane, the last strip of one column, full-height columns over 1023 | 1024"""
    rng = np.random.default_rng(12)
    rows = [(w, 3, [(0, blob(rng, w / 2, 1.5, w / 2, 9)), (0, [(w - 3.0, 0.0), (float(w), 3.0)]), (0, [(1020.0, 0.0), (1030.0, 3.0)]),
                    (0, [(0.0, 0.0), (float(w), 3.0)]), (0, [(1.0, 1.0), (w - 1.0, 2.0)])]) for w in (1023, 1024, 1025, 2049)]
    want = both(native, table(rows))
    assert (want[2] > 0).all() and [runs_of(want, 5 * k + 3) for k in range(4)] == [[0, 3 * w] for w in (1023, 1024, 1025, 2049)]
    assert runs_of(want, 12) == [3060, 15] and runs_of(want, 17) == [3060, 30, 3057] and len(runs_of(want, 19)) == 2 * 2047 + 1


def test_default_band_heights(native):
    """bands of 64 lines (K23_BAND): reaches of 63, 64, 65 and 200 lines, transitions on the first and last line of a band"""
    rng = np.random.default_rng(13)
    rows = []
    for h in (63, 64, 65, 200):
        rows.append((9, h, [(0, blob(rng, 4.5, h / 2, h / 2, 9)), (0, [(2.0, 0.0), (7.0, float(h))]), (0, [(1.0, 63.0), (8.0, 65.0)]),
                            (0, [(0.0, 64.0), (9.0, 128.0)]), (0, [(3.0, 1.0), (4.0, h - 1.0)])]))
    want = both(native, table(rows))
    assert runs_of(want, 16) == [2 * 200, 5 * 200, 2 * 200] and runs_of(want, 18)[:3] == [64, 64, 136] and want[2][17] == 14


# ----------------------------------------------------------------------------------------------- edges and the list
@pytest.mark.parametrize("m", [2, 3, 64, 65, 300])
def test_edge_chunks(native, m):
    rng = np.random.default_rng(m)
    pts = [(3.0, 2.0), (50.0, 41.0)] if m == 2 else blob(rng, 30, 25, 28, m)
    want = both(native, table([(61, 50, [(0, pts), (3, blob(rng, 30, 25, 10, 5))])]))
    assert want[2][0] > 50 and len(runs_of(want, 0)) > 20


@pytest.mark.parametrize("crossings", [1, 3, 8])
def test_a_full_crossing_list_is_applied_and_emptied(native, crossings):
    option(native, crossings=crossings)
    comb = [(0.0, 0.0)]
    for k in range(40):                                                        # 40 teeth: 80 crossings on a scanline
        comb += [(3.0 * k + 0.5, 10.0), (3.0 * k + 1.5, 1.0), (3.0 * k + 2.5, 10.0)]
    comb.append((125.0, 0.0))
    want = both(native, table([(125, 12, [(0, comb), (0, blob(np.random.default_rng(6), 60, 6, 30, 9))])]))
    assert want[2][0] > 300 and len(runs_of(want, 0)) > 100


# ----------------------------------------------------------------------------------------------- polygon shapes
def test_polygon_shapes(native):
    bow = [(2.0, 2.0), (20.0, 18.0), (2.0, 18.0), (20.0, 2.0)]
    left, right = [(3.0, 1.0), (11.3, 2.0), (9.7, 15.0), (2.0, 12.0)], [(11.3, 2.0), (19.0, 4.0), (18.0, 16.0), (9.7, 15.0)]
    quad = [(3.0, 1.0), (11.3, 2.0), (19.0, 4.0), (18.0, 16.0), (9.7, 15.0), (2.0, 12.0)]
    partly = [(-6.5, 4.0), (9.0, -3.0), (30.0, 10.0), (12.0, 31.0)]
    outside = [[(-9.0, -9.0), (-1.0, -1.0)], [(25.0, 3.0), (40.0, 9.0)], [(3.0, 21.0), (9.0, 30.0)], [(-30.0, 5.0), (-2.0, 8.0)]]
    t = table([(22, 20, [(0, bow), (0, left), (0, right), (0, quad), (0, partly)] + [(0, o) for o in outside]),
               (1, 9, [(0, [(0.0, 2.0), (1.0, 5.0)]), (0, [(-3.0, -3.0), (5.0, 20.0)]), (0, [(0.2, 0.0), (0.4, 9.0)])]),
               (9, 1, [(0, [(2.0, 0.0), (5.0, 1.0)]), (0, [(-3.0, -3.0), (15.0, 20.0)]), (0, [(0.0, 0.2), (9.0, 0.4)])])])
    want = both(native, t)
    masks = [R.decode(runs_of(want, p), 22, 20) for p in range(5)]
    assert np.array_equal(masks[0], K21.cover(bow, 22, 20)) and 0 < masks[0].sum() < 16 * 18 // 2 + 20       # even-odd: two triangles
    assert want[2][1] + want[2][2] == want[2][3] and not (masks[1] & masks[2]).any() and np.array_equal(masks[1] | masks[2], masks[3])
    assert 0 < want[2][4] < 22 * 20 and want[3][4].tolist()[:2] == [0, 0] and not want[2][5:9].any()
    assert [runs_of(want, p) for p in range(5, 9)] == [[440]] * 4
    assert [runs_of(want, p) for p in range(9, 12)] == [[2, 3, 4], [0, 9], [9]]
    assert [runs_of(want, p) for p in range(12, 15)] == [[2, 3, 4], [0, 9], [9]]


def test_a_large_image(native):
    side = 32768
    box = [(side - 3.0, 100.0), (float(side), 102.0)]
    want = both(native, table([(side, side, [(0, box), (-1, box), (0, [(5.0, 5.0), (6.0, 6.0)])])]), max_pixels=1 << 30)
    runs = runs_of(want, 0)
    assert runs == [(side - 3) * side + 100, 2, side - 2, 2, side - 2, 2, side - 102] and sum(runs) == 1 << 30
    text = want[7][want[6][0]:want[6][1]]
    assert R.dec(text) == runs and len(R.enc(runs[:1])) == 7 and runs[6] - runs[4] < 0        # a 7-byte code and a negative delta
    assert want[2].tolist() == [6, 0, 1] and want[3][0].tolist() == [side - 3, 100, 3, 2] and want[1].tolist() == [0, 255, 0]
    assert runs_of(want, 2) == [5 * side + 5, 1, (1 << 30) - 5 * side - 6]


# ----------------------------------------------------------------------------------------------- statuses and actions
def test_statuses_and_actions_between_encoded_ones(native):
    box, tri = [(0.0, 0.0), (3.0, 3.0)], [(0.0, 0.0), (3.0, 1.0), (2.0, 4.0)]
    polys = [(0, box), (-1, box), (2, [(1.0, 1.0), (math.nan, 3.0), (5.0, 5.0)]), (3, [(3.0, 3.0)]), (4, []), (0, tri),
             (1, [(0.0, 0.0), (2.0 ** 43, 4.0)]), (7, tri)]
    t = table([(4, 4, polys), (0, 4, polys), (4.5, 4, polys), (4, 4, polys), (6, 3, polys), (17, 1, polys), (2, 8, polys)])
    want = both(native, t, max_pixels=16)
    assert want[0].tolist() == [0, 1, 2, 0, 3, 3, 0]
    assert want[1].tolist() == [0, 255, 2, 3, 3, 0, 2, 0] + [5, 255, 5, 5, 5, 5, 5, 5] * 2 + [0, 255, 2, 3, 3, 0, 2, 0] + \
        [5, 255, 5, 5, 5, 5, 5, 5] * 2 + [0, 255, 2, 3, 3, 0, 2, 0]
    assert np.diff(want[4]).tolist()[8:24] == [0] * 16 and want[2][0] == 9 and not want[2][8:24].any()
    none = (np.zeros(0), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    want = both(native, none)                                                  # n_rows == 0
    assert want[4].tolist() == [0] and want[6].tolist() == [0] and want[7] == b""
    want = both(native, table([(5, 4, []), (2, 2, [])]))                      # n_polys == 0
    assert want[0].tolist() == [0, 0] and len(want[5]) == 0
    want = both(native, table([(5, 4, [(-1, box), (-3, tri)])]))             # nothing selected: no runs, no text
    assert want[1].tolist() == [255, 255] and len(want[5]) == 0 and want[7] == b""


# ----------------------------------------------------------------------------------------------- scans and grids
def test_more_than_one_part_in_every_scan(native):
    """2,400 polygons (K13_SCAN_TILE is 2,048): the scans over polygons, items, runs all have more than one part"""
    rng = np.random.default_rng(9)
    rows = []
    for r in range(300):
        w, h = int(rng.integers(3, 30)), int(rng.integers(2, 12))
        polys = []
        for k in range(8):
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            m = int(rng.integers(2, 7))
            pts = np.stack([cx + rng.uniform(-6, 6, m), cy + rng.uniform(-4, 4, m)], axis=1)
            if (r + k) % 3 == 0:
                pts = np.round(pts)
            polys.append((-1 if (r + k) % 11 == 0 else k, [tuple(p) for p in pts.tolist()]))
        rows.append((w, h, polys))
    want = both(native, table(rows))
    assert len(want[1]) == 2400 and (want[1] == 0).sum() > 2048 and len(want[5]) > 3 * 2048 and len(want[7]) > len(want[5])


def test_the_long_sparse_table(native):
    xy, pt_off, row_off, W, H = LT.long_sparse(0, 2502)
    t = (xy, pt_off, row_off, LT.k21_val(len(pt_off) - 1), W, H)
    want = both(native, t, max_pixels=1 << 20)
    assert np.diff(row_off).max() == 700 and {0, 1, 2} <= set(want[0].tolist()) and {0, 5, 255} <= set(want[1].tolist())
    k21 = K21.raster_arrays(*t, 9, 1 << 20)
    assert np.array_equal(want[2], k21[3]) and np.array_equal(want[1], k21[2])


def test_more_items_than_workgroups(native):
    option(native, strip=17, grid=3, band=7)
    rng = np.random.default_rng(10)
    polys = [(0, blob(rng, 50, 20, 45, 9)), (0, [(0.0, 0.0), (100.0, 40.0)]), (0, blob(rng, 80, 10, 15, 6)), (0, [(3.0, 3.0), (5.0, 9.0)])]
    want = both(native, table([(100, 40, polys), (30, 30, polys)]))
    assert (want[2][:4] > 0).all() and runs_of(want, 1) == [0, 4000] and runs_of(want, 5) == [0, 900]   # 90 items and more on 3 workgroups


# ----------------------------------------------------------------------------------------------- measure and caps
def test_measure_only_and_buffers_one_too_small(native):
    t = table(random_rows(np.random.default_rng(8), 12, values=(0, 1, 2)))
    want = R.rle_arrays(*t)
    assert len(want[5]) > 100 and len(want[7]) > len(want[5])
    got, rc, n_runs, _ = run_dev(t, upto="measure")                            # run_dev checks that the text offsets stay untouched
    assert rc == 0 and n_runs == len(want[5])
    same(got, want[:5], NAMES[:5])
    got, rc, n_runs, n_text = run_dev(t, upto="runs")
    assert rc == 0 and n_text == len(want[7])
    same(got, want[:7], NAMES[:7])
    got, rc, n_runs, _ = run_dev(t, runs_cap=len(want[5]) - 1)                 # run_dev checks that no run was written
    assert rc == RANGE and n_runs == len(want[5]) and b"too small" in native.lib().dyd_last_error()
    same(got, want[:5], NAMES[:5])
    got, rc, n_runs, n_text = run_dev(t, text_cap=len(want[7]) - 1)            # ... and no byte of the text
    assert rc == RANGE and n_text == len(want[7]) and n_runs == len(want[5]) and b"too small" in native.lib().dyd_last_error()
    same(got, want[:7], NAMES[:7])
    for phase in (0, 2, 3, 15):
        got, rc, _, _ = run_dev(t, phase=phase)
        assert rc == 0
        same(got, want)


@pytest.mark.parametrize("max_pixels", [0, -1, 2 ** 30 + 1])
def test_invalid_arguments_are_the_argument_error(native, max_pixels):
    xy, pt_off, row_off, sel, W, H = table([(20, 10, [(1, [(5.0, 2.0), (15.0, 8.0)])])])
    out = [np.zeros(8, d) for d in (np.uint8, np.uint8, np.int64, np.int32, np.int64, np.int64)]
    runs, n_runs, text, total = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    L = native.lib()
    rc = L.dyd_polygon_rle(p(xy), p(pt_off), p(row_off), p(sel), p(W), p(H), 1, max_pixels, *[p(a) for a in out], C.byref(runs),
                           C.byref(n_runs), C.byref(text), C.byref(total))
    assert rc == INVALID and b"invalid argument" in L.dyd_last_error() and not runs.value and not text.value
    rc = L.dyd_polygon_rle_dev(None, None, None, None, None, None, 0, 0, 0, max_pixels, *[None] * 6, 0, None, None, 0, C.byref(n_runs),
                               C.byref(total))
    assert rc == INVALID
    assert L.dyd_polygon_rle_dev(None, None, None, None, None, None, -1, 0, 0, 16, *[None] * 6, 0, None, None, 0, C.byref(n_runs),
                                 C.byref(total)) == INVALID
    assert L.dyd_polygon_rle_dev(None, None, None, None, None, None, 1, 0, 0, 16, *[None] * 6, 0, None, None, 0, C.byref(n_runs),
                                 C.byref(total)) == INVALID


# ----------------------------------------------------------------------------------------------- against K21 on the device
def test_against_k21_on_the_device(native):
    rng = np.random.default_rng(1)
    t = table(random_rows(rng, 120))
    want = both(native, t, max_pixels=96 * 96)
    assert {0, 2, 3, 5, 255} <= set(want[1].tolist()) and {0, 1, 2, 3} <= set(want[0].tolist()) and len(want[5]) > 5000
    k21 = native.rasterize_polygons(*t, 255, 96 * 96)
    assert np.array_equal(want[2], k21[3]) and np.array_equal(want[1], k21[2]) and np.array_equal(want[0], k21[0])
    option(native, strip=17, crossings=3, band=5)                              # the same table over narrow strips, low bands, a short list
    same(native.polygon_rle(*t, 96 * 96), want)
    option(native, band=1)
    same(native.polygon_rle(*t, 96 * 96), want)
    option(native)
    single = table([(w, h, polys[:1]) for w, h, polys in random_rows(rng, 60, max_size=70) if polys and polys[0][0] >= 0])
    got = native.polygon_rle(*single)
    status, pix_off, action, covered, _, pixels = native.rasterize_polygons(*single, 255)
    checked = 0
    for p in np.flatnonzero(got[1] == 0).tolist():                             # one polygon per row: p is the row
        w, h = int(single[4][p]), int(single[5][p])
        mask = pixels[pix_off[p]:pix_off[p + 1]].reshape(h, w) != 255
        assert np.array_equal(U.rle_to_mask(got[7][got[6][p]:got[6][p + 1]], [h, w]), mask), p
        assert np.array_equal(U.rle_to_mask(got[5][got[4][p]:got[4][p + 1]], [h, w]), mask) and got[2][p] == covered[p] == mask.sum()
        checked += 1
    assert checked > 20


# ----------------------------------------------------------------------------------------------- end to end
def test_export_coco_csv_end_to_end(native, tmp_path):
    rng = np.random.default_rng(21)
    names = ["a", "b", "c"]
    cells, rows = [], random_rows(rng, 40, max_polys=5, max_pts=12, max_size=60, values=(0, 1, 2))
    for _, _, polys in rows:
        cells.append(json.dumps({"objects": [{"name": names[max(v, 0)], "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}
                                             for v, pts in polys if all(map(math.isfinite, sum(pts, ())))]}))
    df = pd.DataFrame({"source": [f"im{k}.jpg" for k in range(40)], P.ANNOTATION_COL: cells,
                       "width": [r[0] for r in rows], "height": [r[1] for r in rows]})
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    res = P.export_coco_csv(src, tmp_path / "coco.json", segmentation="rle", iscrowd=1, classes=names, skipped_csv=tmp_path / "s.csv")
    back = pd.read_csv(src, encoding="utf-8-sig")

    from helpers import OracleBackend
    ref_be = type("RefBackend", (OracleBackend,), {"polygon_rle": staticmethod(R.rle_arrays)})()
    ref = P.export_coco_frame(back, tmp_path / "ref.json", segmentation="rle", iscrowd=1, classes=names, skipped_csv=tmp_path / "r.csv",
                              backend=ref_be)
    assert open(res["output"], "rb").read() == open(ref["output"], "rb").read()
    assert open(tmp_path / "s.csv", "rb").read() == open(tmp_path / "r.csv", "rb").read()
    doc = json.load(open(res["output"], encoding="utf-8"))
    assert res["annotations"] == len(doc["annotations"]) > 40 and res["clipped"] == 0 and res["images"] == len(doc["images"])
    sizes = {im["id"]: (im["height"], im["width"]) for im in doc["images"]}
    want = P.polygon_rle(back[P.ANNOTATION_COL], back["width"], back["height"], classes=names, backend=ref_be)
    printed = [k for k, c in enumerate(want.counts) if c is not None and want.polygons["area"][k] > 0]
    assert len(printed) == len(doc["annotations"])
    for a, k in zip(doc["annotations"], printed):
        seg = a["segmentation"]
        assert tuple(seg["size"]) == sizes[a["image_id"]] and seg["counts"].encode() == want.counts[k] and a["iscrowd"] == 1
        assert U.rle_to_mask(seg["counts"], seg["size"]).sum() == a["area"] == want.polygons["area"][k]
        assert a["bbox"] == want.polygons[["x", "y", "w", "h"]].to_numpy()[k].tolist()
    got = P.polygon_rle(back[P.ANNOTATION_COL], back["width"], back["height"], classes=names)      # the step itself on the device
    assert got.counts == want.counts and got.sizes == want.sizes and got.polygons.equals(want.polygons) and got.totals == want.totals
