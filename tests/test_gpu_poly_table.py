"""The host path the polygon steps share (csrc/poly_table.h, the text hand-back of dyd_common.h), at its smallest shapes: degenerate
tables through K13, K14, K17, K20 and K21, malformed tables through the host-pointer entries of K13, K14, K16, K17, K19, K20 and
K21, and the malloc'ed text of K7, K13 and K16.  K16's degenerate tables are in test_gpu_coco.py.  Needs a real MI355X."""
import ctypes as CT

import numpy as np
import pytest

import coco_ref
import polygon_audit_ref
import polygon_raster_ref
import polygon_simplify_ref
import tile_labels_ref
import yolo_obb_ref
import yolo_seg_ref
from test_gpu_polygon_audit import run_dev as k14_dev, same as k14_same
from test_gpu_polygon_raster import both as k21_both
from test_gpu_polygon_simplify import same as k19_same
from test_gpu_tile_labels import both as k20_both
from test_gpu_yolo_obb import check as k17_check
from test_gpu_yolo_seg import check as k13_check

pytestmark = pytest.mark.gpu

I32, U8 = np.int32, np.uint8


def _degenerate():
    """(xy, pt_off, row_off, n_rows) of: no rows; four rows without a polygon; three polygons without a point (xy is NULL at the
    host-pointer entry); 40 five-point polygons with empty rows at both ends"""
    z = np.zeros(0)
    yield z, np.zeros(1, I32), np.zeros(1, I32)
    yield z, np.zeros(1, I32), np.zeros(5, I32)
    yield z, np.zeros(4, I32), np.asarray([0, 1, 1, 3], I32)
    pts = np.random.default_rng(8).uniform(-50, 700, (40, 5, 2))
    yield pts.reshape(-1), np.arange(0, 201, 5, dtype=I32), np.r_[0, 0, np.arange(0, 40, 4)[1:], 40, 40].astype(I32)


def test_degenerate_tables_k13(native):
    for xy, pt_off, row_off in _degenerate():
        n, nb = len(row_off) - 1, len(pt_off) - 1
        for sel in (None, (np.arange(nb) % 3 != 0).astype(U8)):
            off, flag, action, text = k13_check(native, xy, pt_off, row_off, sel, np.full(n, 640.0), np.full(n, 480.0),
                                                np.arange(n, dtype=I32))
            assert len(off) == n + 1 and len(flag) == n and len(action) == nb and off[-1] == len(text)
            if len(xy) == 0:
                assert text == b"" and (flag == 1).all() and set(action.tolist()) <= {3, 255}
            else:
                assert text.count(b"\n") + (flag == 0).sum() == (action <= 1).sum() > 10 and flag[0] == flag[-1] == 1


def test_degenerate_tables_k14(native):
    for xy, pt_off, row_off in _degenerate():
        n, nb = len(row_off) - 1, len(pt_off) - 1
        for nc in (0, 3) if nb == 0 else (3,):
            table = (xy, pt_off, row_off, (np.arange(nb) % (nc + 1) - 1).astype(I32), np.full(n, 640.0), np.full(n, 480.0),
                     np.zeros(n, U8), nc)
            want = polygon_audit_ref.audit_arrays(*table)
            k14_same(native.audit_polygons(*table), want)
            k14_same(k14_dev(table), want)
            assert want[3][:, 0].sum() == (table[3] >= 0).sum()
            if len(xy) == 0:
                assert set(want[0].tolist()) <= {3, 255}
            else:
                assert (want[0] <= 1).sum() > 20


def test_degenerate_tables_k17(native):
    for xy, pt_off, row_off in _degenerate():
        n, nb = len(row_off) - 1, len(pt_off) - 1
        for sel in (None, (np.arange(nb) % 3 != 0).astype(U8)):
            off, flag, action, text, clamped, corners = k17_check(native, xy, pt_off, row_off, sel, np.full(n, 640.0), np.full(n, 480.0),
                                                                  np.arange(n, dtype=I32))
            assert len(off) == n + 1 and len(flag) == n and len(action) == len(clamped) == nb and off[-1] == len(text)
            assert corners.shape == (nb, 8) and np.array_equal(np.isnan(corners).any(axis=1), action > 1)
            if len(xy) == 0:
                assert text == b"" and (flag == 1).all() and set(action.tolist()) <= {3, 255}
            else:
                assert text.count(b"\n") + (flag == 0).sum() == (action <= 1).sum() > 10 and flag[0] == flag[-1] == 1


K20_PARAMS = (256, 256, 200, 200, 0.1, 0, 4096)      # 3 x 3 tiles on a 640 x 480 row


def test_degenerate_tables_k20(native):
    for xy, pt_off, row_off in _degenerate():
        n, nb = len(row_off) - 1, len(pt_off) - 1
        for mode in (0, 1):
            t = (xy, pt_off, row_off, (np.arange(nb) % 3 - 1).astype(I32), np.full(n, 640.0), np.full(n, 480.0))
            status, tile_off, lines, text_off, action, written, cut, dropped, text = k20_both(native, t, K20_PARAMS[:5] + (mode, 4096))
            assert len(status) == n and tile_off.tolist() == list(range(0, 9 * n + 1, 9)) and len(lines) == 9 * n
            assert len(text_off) == 9 * n + 1 and text_off[-1] == len(text) and len(action) == len(written) == len(cut) == len(dropped) == nb
            assert (status == 0).all() and lines.sum() == written.sum()
            if len(xy) == 0:
                assert text == b"" and not lines.any() and not written.any() and set(action.tolist()) <= {3, 255}
            else:
                assert (action <= 1).sum() > 10 and written.sum() > 20 and cut.sum() > 10 and (lines[:9] == 0).all() and (lines[-9:] == 0).all()


def test_degenerate_tables_k21(native):
    for xy, pt_off, row_off in _degenerate():
        n, nb = len(row_off) - 1, len(pt_off) - 1
        t = (xy, pt_off, row_off, (np.arange(nb) % 3 - 1).astype(I32), np.full(n, 320.0), np.full(n, 240.0))
        status, pix_off, action, covered, owned, pixels = k21_both(native, t, background=200)
        assert len(status) == n and pix_off.tolist() == list(range(0, 76800 * n + 1, 76800)) and len(pixels) == 76800 * n
        assert len(action) == len(covered) == len(owned) == nb and (status == 0).all() and (owned <= covered).all()
        if len(xy) == 0:
            assert (pixels == 200).all() and not covered.any() and set(action.tolist()) <= {3, 255}
        else:
            assert (action == 0).sum() >= (covered > 0).sum() > 10 and (owned < covered).any()
            assert (pixels[:76800] == 200).all() and (pixels[-76800:] == 200).all() and set(np.unique(pixels).tolist()) == {0, 1, 200}


def _valid():
    """3 rows, 4 triangles"""
    xy = np.asarray([[10, 10, 200, 20, 100, 300]] * 4, np.float64).reshape(-1) + np.repeat(np.arange(4.0), 6)
    return xy, np.asarray([0, 3, 6, 9, 12], I32), np.asarray([0, 2, 2, 4], I32)


def _entry(native, name):
    """(xy, pt_off, row_off) -> the entry's outputs on a table of three 640 x 480 rows"""
    W, H, st = np.full(3, 640.0), np.full(3, 480.0), np.zeros(3, U8)
    if name == "k13":
        cid = np.asarray([7, 8, 9], I32)
        return (lambda xy, pt, row: native.yolo_seg_lines(xy, pt, row, None, W, H, cid),
                lambda xy, pt, row: yolo_seg_ref.seg_arrays(xy, pt, row, None, W, H, cid))
    if name == "k14":
        cls = np.asarray([0, 1, -1, 1], I32)
        return (lambda xy, pt, row: native.audit_polygons(xy, pt, row, cls, W, H, st, 2),
                lambda xy, pt, row: polygon_audit_ref.audit_arrays(xy, pt, row, cls, W, H, st, 2))
    if name == "k16":
        cat = np.asarray([1, 2, 0, 2], I32)
        return (lambda xy, pt, row: native.coco_annotations(xy, pt, row, cat, W, H, st),
                lambda xy, pt, row: coco_ref.coco_arrays(xy, pt, row, cat, W, H, st))
    if name == "k17":
        cid = np.asarray([7, 8, 9], I32)
        return (lambda xy, pt, row: native.yolo_obb_lines(xy, pt, row, None, W, H, cid, corners=True),
                lambda xy, pt, row: yolo_obb_ref.obb_arrays(xy, pt, row, None, W, H, cid))
    val = np.asarray([0, 1, -1, 1], I32)
    if name == "k20":
        return (lambda xy, pt, row: native.yolo_tile_lines(xy, pt, row, val, W, H, *K20_PARAMS),
                lambda xy, pt, row: tile_labels_ref.tile_arrays(xy, pt, row, val, W, H, *K20_PARAMS))
    return (lambda xy, pt, row: native.rasterize_polygons(xy, pt, row, val, W, H, 3, 1 << 20),
            lambda xy, pt, row: polygon_raster_ref.raster_arrays(xy, pt, row, val, W, H, 3, 1 << 20))


MALFORMED = {"row_off[0] = 1": ("row", [1, 2, 2, 4], r"row_off\[0\] != 0"), "row_off decreases": ("row", [0, 3, 2, 4], "row_off not monotone"),
             "pt_off[0] = 1": ("pt", [1, 3, 6, 9, 12], r"pt_off\[0\] != 0"), "pt_off decreases": ("pt", [0, 6, 3, 9, 12], "pt_off not monotone")}


@pytest.mark.parametrize("entry", ["k13", "k14", "k16", "k17", "k20", "k21"])
def test_malformed_tables(native, entry):
    run, ref = _entry(native, entry)
    xy, pt_off, row_off = _valid()
    for which, off, message in MALFORMED.values():
        bad = np.asarray(off, I32)
        with pytest.raises(native.NativeError, match="invalid argument: " + message):
            run(xy, bad if which == "pt" else pt_off, bad if which == "row" else row_off)
        got, want = run(xy, pt_off, row_off), ref(xy, pt_off, row_off)      # a valid call right after
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert bytes(a) == bytes(b) if isinstance(b, bytes) else np.array_equal(a, b, equal_nan=True)


def test_malformed_pt_off_k19(native):
    """K19 has no rows: the two pt_off cases through the same check"""
    xy, pt_off, _ = _valid()
    for which, off, message in MALFORMED.values():
        if which == "pt":
            with pytest.raises(native.NativeError, match="invalid argument: " + message):
                native.simplify_polygons(xy, np.asarray(off, I32), 1.0)
            k19_same(native.simplify_polygons(xy, pt_off, 1.0), polygon_simplify_ref.simplify_arrays(xy, pt_off, 1.0))


def _hand_back(native, entry, size):
    """the raw host-pointer entry on one row of one box / polygon -> (text pointer, length)"""
    L = native.lib()
    p = lambda a, dt: np.ascontiguousarray(a, dt).ctypes.data_as(CT.c_void_p)   # noqa: E731
    tri, box = np.asarray([10.0, 10, 200, 20, 100, 300]), np.asarray([10.0, 20, 110, 220])
    W, H, one = np.asarray([size]), np.asarray([480.0]), np.asarray([0, 1], I32)
    keep = [W, H, one, tri, box, np.asarray([0, 3], I32), np.asarray([5], I32), np.asarray([0 if size > 0 else 1], U8),
            np.zeros(2, np.int64), np.zeros(1, U8), np.zeros(1, U8), np.zeros(1), np.zeros(1, I32)]
    _, _, _, _, _, pt, cid, st, off, flag, act, area, kept = keep
    text, total = CT.c_void_p(), CT.c_int64(-1)
    if entry == "k7":
        rc = L.dyd_yolo_lines(p(box, np.float64), p(one, I32), None, p(W, np.float64), p(H, np.float64), p(cid, I32), 1, p(off, np.int64),
                              p(flag, U8), CT.byref(text), CT.byref(total))
    elif entry == "k13":
        rc = L.dyd_yolo_seg_lines(p(tri, np.float64), p(pt, I32), p(one, I32), None, p(W, np.float64), p(H, np.float64), p(cid, I32), 1,
                                  p(off, np.int64), p(flag, U8), p(act, U8), CT.byref(text), CT.byref(total))
    else:
        rc = L.dyd_coco_annotations(p(tri, np.float64), p(pt, I32), p(one, I32), p(cid, I32), p(W, np.float64), p(H, np.float64),
                                    p(st, U8), 1, 1, 1, 1, p(act, U8), p(area, np.float64), p(kept, I32), CT.byref(text),
                                    CT.byref(total))
    native.check(rc, entry)
    return L, text, total.value


ONE_TEXT = {"k7": b"5 0.093750 0.250000 0.156250 0.416667",
            "k13": b"5 0.015625 0.020833 0.312500 0.041667 0.156250 0.625000",
            "k16": b'{"id":1,"image_id":1,"category_id":5,"bbox":[10.00,10.00,190.00,290.00],"area":27100.00,"iscrowd":0,'
                   b'"segmentation":[[10.00,10.00,200.00,20.00,100.00,300.00]]}'}


@pytest.mark.parametrize("entry", ["k7", "k13", "k16"])
def test_text_hand_back(native, entry):
    L, text, total = _hand_back(native, entry, 640.0)                          # exactly one line / one object
    assert text.value and CT.string_at(text.value, total) == ONE_TEXT[entry]
    L.dyd_host_free(text)
    L, text, total = _hand_back(native, entry, 0.0)                            # a row without a size: a text of length 0
    assert total == 0 and text.value                                           # still a pointer the caller releases
    L.dyd_host_free(text)
    W, H, cid, row, pt, tri = [0.0], [480.0], [5], [0, 1], [0, 3], np.asarray([10.0, 10, 200, 20, 100, 300])
    assert native.yolo_lines(np.asarray([10.0, 20, 110, 220]), row, None, W, H, cid)[2] == b""
    assert native.yolo_seg_lines(tri, pt, row, None, W, H, cid)[3] == b""
    assert native.coco_annotations(tri, pt, row, cid, W, H, [1])[3] == b""
