"""K17 (YOLO oriented-box label lines, csrc/k17_obb.hip) through both C-ABI entries and yolo_obb_label_texts, against the
restatement in tests/yolo_obb_ref.py.  Byte-exact: text, offsets, flags, actions and `clamped`; the corners with ==, so a signed
zero is not a difference.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import yolo_obb_ref as R
from test_gpu_yolo_seg import random_table
from test_yolo_obb_cpu import WORKED, integer_polygons
from test_yolo_seg_cpu import cell, ob
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu


def same(got, want):
    """(text_off, flag, action, text, clamped, corners) of an entry against the restatement's"""
    for k in (0, 1, 2, 4):
        assert np.array_equal(got[k], want[k]), k
    assert got[3] == want[3]
    assert got[5].shape == want[5].shape and np.array_equal(got[5], want[5], equal_nan=True)


def check(native, xy, pt_off, row_off, sel, W, H, cid):
    want = R.obb_arrays(xy, pt_off, row_off, sel, W, H, cid)
    got = native.yolo_obb_lines(xy, pt_off, row_off, sel, W, H, cid, corners=True)
    same(got, want)
    short = native.yolo_obb_lines(xy, pt_off, row_off, sel, W, H, cid)
    assert len(short) == 5 and short[3] == want[3] and np.array_equal(short[4], want[4])
    same(check_dev(xy, pt_off, row_off, sel, W, H, cid), want)
    return got


def check_dev(xy, pt_off, row_off, sel, W, H, cid, offset=3, hz=None):
    """the _dev entry on torch tensors: measure only, too small a buffer, then print into a buffer at an odd address.
    hz: the harness of tests/stream_contract.py (its decoys in the order xy, pt_off, row_off, sel, W, H, cid), armed anew for
    every one of the calls; without one the calls go to torch's current stream as they always did"""
    import torch
    from deal_yolo_daya_amd import _native
    from stream_contract import PLAIN

    hz = hz or PLAIN
    dev = torch.device("cuda", 0)
    L = _native.lib()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    n, nb, npnt = len(row_off) - 1, int(row_off[-1]), int(pt_off[-1])
    d_xy, d_pt, d_row = t(xy if len(xy) else np.zeros(2), np.float64), t(pt_off, np.int32), t(row_off, np.int32)
    d_sel = t(sel, np.uint8) if sel is not None else None
    d_w, d_h, d_cid = t(W, np.float64), t(H, np.float64), t(cid, np.int32)
    toff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    flag = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    act = torch.zeros(max(nb, 1), dtype=torch.uint8, device=dev)
    clamped = torch.full((max(nb, 1),), 7, dtype=torch.uint8, device=dev)
    corners = torch.full((max(nb, 1), 8), float("nan"), dtype=torch.float64, device=dev)
    total = C.c_int64()
    args = (d_xy.data_ptr(), d_pt.data_ptr(), d_row.data_ptr(), d_sel.data_ptr() if d_sel is not None else None, d_w.data_ptr(),
            d_h.data_ptr(), d_cid.data_ptr(), n, nb, npnt, toff.data_ptr(), flag.data_ptr(), act.data_ptr(), clamped.data_ptr())
    hz.arm([d_xy, d_pt, d_row, d_sel, d_w, d_h, d_cid])
    hz.watch(toff, flag, act, clamped, corners)
    _native.check(hz.call(L.dyd_yolo_obb_lines_dev, *args, None, None, 0, C.byref(total)), "measure")     # no corners, no text
    T = total.value
    if T:
        small = torch.empty(T - 1 if T > 1 else 1, dtype=torch.uint8, device=dev)
        rc = hz.call(L.dyd_yolo_obb_lines_dev, *args, corners.data_ptr(), small.data_ptr(), T - 1, C.byref(total))
        assert rc != 0 and total.value == T                                    # DYD_ERR_RANGE with the needed size
    buf = torch.full((T + offset + 32,), 0xAB, dtype=torch.uint8, device=dev)
    hz.watch(buf)
    _native.check(hz.call(L.dyd_yolo_obb_lines_dev, *args, corners.data_ptr(), buf.data_ptr() + offset, T, C.byref(total)), "print")
    hz.restore()
    b = buf.cpu().numpy()
    assert (b[:offset] == 0xAB).all() and (b[offset + T:] == 0xAB).all()      # nothing written outside the text
    return (toff.cpu().numpy(), flag.cpu().numpy()[:n], act.cpu().numpy()[:nb], b[offset:offset + T].tobytes(),
            clamped.cpu().numpy()[:nb], corners.cpu().numpy()[:nb])


def small_table(rng, n_polys, n_rows):
    """n_polys polygons of 2..7 points spread over n_rows rows, rows of no polygon among them"""
    cuts = np.sort(rng.integers(0, n_polys + 1, n_rows - 1))
    cuts[::3] = cuts[0]                                                       # runs of empty rows
    row_off = np.concatenate([[0], np.sort(cuts), [n_polys]]).astype(np.int32)
    npts = rng.integers(2, 8, n_polys)
    pt_off = np.concatenate([[0], np.cumsum(npts)]).astype(np.int32)
    xy = rng.uniform(-40, 680, (int(pt_off[-1]), 2)).reshape(-1)
    return xy, pt_off, row_off, None, np.full(n_rows, 640.0), np.full(n_rows, 480.0), rng.integers(0, 1200, n_rows).astype(np.int32)


@pytest.mark.parametrize("n_polys", [0, 1, 255, 256, 257])
def test_tile_edges(native, n_polys):
    got = check(native, *small_table(np.random.default_rng(n_polys), n_polys, 9))
    assert len(got[2]) == n_polys


def test_no_rows(native):
    got = native.yolo_obb_lines(np.zeros(0), np.zeros(1, np.int32), np.zeros(1, np.int32), None, np.zeros(0), np.zeros(0),
                                np.zeros(0, np.int32), corners=True)
    assert got[3] == b"" and len(got[1]) == 0 and got[5].shape == (0, 8)
    same(check_dev(np.zeros(0), np.zeros(1, np.int32), np.zeros(1, np.int32), None, np.zeros(0), np.zeros(0), np.zeros(0, np.int32)),
         R.obb_arrays(np.zeros(0), [0], [0], None, [], [], []))


@pytest.mark.parametrize("seed,with_sel,special", [(1, True, True), (2, False, False)])
def test_random_tables(native, seed, with_sel, special):
    rng = np.random.default_rng(seed)
    got = check(native, *random_table(rng, 600, max_polys=6, special=special, with_sel=with_sel))
    assert set(np.unique(got[2]).tolist()) >= {0, 1, 3, 4} and got[4].any()


def test_integer_coordinates(native):
    polys = [p for p, size in integer_polygons() if size == 5.0][:400] + [p for p, size in integer_polygons() if size == 1024.0][:200]
    pt_off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    xy = np.asarray([v for p in polys for q in p for v in q], np.float64)
    row_off = np.arange(0, len(polys) + 1, 3, dtype=np.int32)
    n = len(row_off) - 1
    got = check(native, xy, pt_off, row_off, None, np.full(n, 1024.0), np.full(n, 1024.0), np.arange(n, dtype=np.int32))
    assert (got[2] == 6).any() and (got[2] == 0).sum() > 400


def test_long_walk(native):
    # 300 points on a circle: every point is a hull vertex, so the walk takes 300 steps of 300 points and ends at the step cap
    # or at the start; a second one crosses every edge of the image
    a = np.linspace(0, 2 * np.pi, 300, endpoint=False)
    inside = np.stack([320 + 200 * np.cos(a), 240 + 200 * np.sin(a)], 1).reshape(-1)
    across = np.stack([320 + 400 * np.cos(a), 240 + 300 * np.sin(a)], 1).reshape(-1)
    got = check(native, np.concatenate([inside, across]), np.asarray([0, 300, 600], np.int32), np.asarray([0, 2], np.int32), None,
                np.asarray([640.0]), np.asarray([480.0]), np.asarray([12], np.int32))
    assert got[2].tolist() == [0, 1]


def test_worked_answers_through_label_texts(native):
    cells = [cell(ob("a", pts)) for pts, *_ in WORKED]
    stats = {}
    texts, reasons = P.yolo_obb_label_texts(cells, ["a"] * len(cells), [w[3] for w in WORKED], [w[1] for w in WORKED],
                                            [w[2] for w in WORKED], native, stats)
    assert texts == [w[4] for w in WORKED]
    assert reasons == [None if w[4] else P.REASON_NO_VALID_BOX for w in WORKED]
    assert stats["flat"] == 1 and stats["clamped"] == 1 and stats["written"] == 5 and stats["device_rows"] == len(WORKED)
