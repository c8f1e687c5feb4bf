"""K16 (COCO annotation objects, csrc/k16_coco.hip) through both C-ABI entries and export_coco_csv, against the restatement in
tests/coco_ref.py.  Byte-exact.  Needs a real MI355X."""
import ctypes as CT
import functools
import math

import numpy as np
import pytest

import coco_ref as C
import test_class_selection_cpu as S
from test_coco_cpu import BE, _wound
from test_gpu_polygon_audit import random_table as k14_table
from test_gpu_yolo_seg import random_table as k13_table
from test_polygon_audit_cpu import _table
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu

WINDOW = 32 * 1024               # K16_WINDOW: bytes of text per print workgroup
ERR_RANGE = -5


@functools.lru_cache(maxsize=None)
def table(kind, seed):
    """(xy, pt_off, row_off, cat_id, W, H, size_status), cat_id drawn from {0, 1..7}"""
    rng = np.random.default_rng(seed)
    if kind == "k14":                                        # integer grids, special values, unusable sizes
        xy, pt_off, row_off, _, W, H, st, _ = k14_table(rng, 300)
    else:                                                    # floats, about 20 % of the polygons cross an edge
        xy, pt_off, row_off, _, W, H, _ = k13_table(rng, 300, max_polys=10, max_pts=20, with_sel=False)
        st = rng.choice([0, 0, 0, 0, 0, 1, 2], size=len(W)).astype(np.uint8)
    cat = rng.integers(0, 8, size=len(pt_off) - 1).astype(np.int32)
    return xy, pt_off, row_off, cat, W, H, st


@functools.lru_cache(maxsize=None)
def wanted(kind, seed, flags):
    return C.coco_arrays(*table(kind, seed), 1, 1, flags)


def same(got, want):
    action, area, kept, text = got
    assert np.array_equal(action, want[0])
    assert np.array_equal(np.isnan(area), np.isnan(want[1]))
    ok = ~np.isnan(want[1])
    assert np.array_equal(np.asarray(area)[ok].view(np.uint64), np.asarray(want[1])[ok].view(np.uint64))
    assert np.array_equal(kept, want[2])
    assert bytes(text) == want[3]


def run_dev(t, img_base=1, ann_base=1, flags=1, offset=3, hz=None):
    """the _dev entry on torch tensors: measure only, a buffer one byte too small, then the text at an odd address inside a guarded
    buffer with the other outputs at guarded offsets.  hz: the harness of tests/stream_contract.py (its decoys in the table's
    order), armed anew for every one of the calls; without one the calls go to torch's current stream"""
    import torch
    from deal_yolo_daya_amd import _native
    from stream_contract import PLAIN

    hz = hz or PLAIN
    xy, pt_off, row_off, cat, W, H, st = t
    dev = torch.device("cuda", 0)
    L = _native.lib()
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    n, nb, npnt = len(row_off) - 1, len(cat), len(xy) // 2
    xy_buf = torch.zeros(len(xy) + 4, dtype=torch.float64, device=dev)
    xy_buf[2:2 + len(xy)] = tt(xy, np.float64)                                  # 16-B aligned, not at the allocation's start
    keep = [tt(pt_off, np.int32), tt(row_off, np.int32), tt(cat if nb else np.zeros(1), np.int32), tt(W if n else np.zeros(1), np.float64),
            tt(H if n else np.zeros(1), np.float64), tt(st if n else np.zeros(1), np.uint8)]
    hz.arm([xy_buf[2:2 + len(xy)]] + keep)
    guard = 0xA5
    outs = lambda: (torch.full((nb + 2 * offset,), guard, dtype=torch.uint8, device=dev),          # noqa: E731
                    torch.full((nb + 2 * offset,), -7.0, dtype=torch.float64, device=dev),
                    torch.full((n + 2 * offset,), -7, dtype=torch.int32, device=dev))
    total = CT.c_int64(-1)

    def call(o, text, cap):
        hz.watch(*o)
        return hz.call(L.dyd_coco_annotations_dev, xy_buf.data_ptr() + 16, *(a.data_ptr() for a in keep), n, nb, npnt, img_base,
                       ann_base, flags, o[0].data_ptr() + offset, o[1].data_ptr() + 8 * offset, o[2].data_ptr() + 4 * offset,
                       text, cap, CT.byref(total))

    def unpack(o):
        hz.restore()
        h = [a.cpu().numpy() for a in o]
        for a, fill in zip(h, (guard, -7.0, -7)):
            assert (a[:offset] == fill).all() and (a[len(a) - offset:] == fill).all(), "write outside the outputs"
        return [a[offset:len(a) - offset] for a in h]

    o1 = outs()
    _native.check(call(o1, None, 0), "measure")
    measured, T = unpack(o1), total.value
    if T:
        small = torch.empty(max(T - 1, 1), dtype=torch.uint8, device=dev)
        total.value = -1
        assert call(outs(), small.data_ptr(), T - 1) == ERR_RANGE and total.value == T
    o2 = outs()
    buf = torch.full((T + offset + 32,), 0xAB, dtype=torch.uint8, device=dev)
    hz.watch(buf)
    _native.check(call(o2, buf.data_ptr() + offset, T), "print")
    printed = unpack(o2)
    b = buf.cpu().numpy()
    assert (b[:offset] == 0xAB).all() and (b[offset + T:] == 0xAB).all()      # nothing written outside the text
    for a, c in zip(measured, printed):
        assert np.array_equal(a, c, equal_nan=True)
    return printed[0], printed[1], printed[2], b[offset:offset + T].tobytes()


def check(native, t, img_base=1, ann_base=1, flags=1, want=None):
    want = want or C.coco_arrays(*t, img_base, ann_base, flags)
    same(native.coco_annotations(*t, img_base, ann_base, flags), want)
    same(run_dev(t, img_base, ann_base, flags), want)
    return want


@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("kind,seed", [("k14", 1), ("k14", 2), ("k14", 3), ("k13", 4)])
def test_random_tables(native, kind, seed, flags):
    want = check(native, table(kind, seed), flags=flags, want=wanted(kind, seed, flags))
    if flags:
        assert len(want[3]) > 2 * WINDOW                     # at least three print windows
    if kind == "k14":
        assert set(want[0].tolist()) == {0, 1, 2, 3, 4, 5, 255}


def _tri_table(pts, W, H, n_rows=None, cat=None):
    """polygons of equal length: pts [n, m, 2]; n_rows None: one row holds them all, else one polygon per row"""
    n, m = pts.shape[:2]
    rows = np.asarray([0, n], np.int32) if n_rows is None else np.arange(n + 1, dtype=np.int32)
    r = len(rows) - 1
    return (pts.reshape(-1), np.arange(0, m * n + 1, m, dtype=np.int32), rows, np.ones(n, np.int32) if cat is None else cat,
            np.full(r, float(W)), np.full(r, float(H)), np.zeros(r, np.uint8))


def test_window_edges(native):
    rng = np.random.default_rng(7)
    a = np.linspace(0, 2 * np.pi, 4000, endpoint=False)      # one polygon of 4,000 vertices crossing every image edge
    big = np.stack([320 + 330 * np.cos(a), 240 + 250 * np.sin(a)], 1)[None]
    want = check(native, _tri_table(big, 640, 480))
    assert want[0].tolist() == [1] and len(want[3]) > WINDOW
    pts = rng.uniform(-100, 700, (2000, 6, 2))               # a row of 2,000 six-point polygons
    want = check(native, _tri_table(pts, 640, 480))
    assert want[2].tolist() == [int((want[0] <= 1).sum())] and len(want[3]) > 3 * WINDOW
    pts[:, 0, 0] = -5.0                                      # every polygon clipped, one per row
    want = check(native, _tri_table(pts, 640, 480, n_rows=2000))
    assert (want[0] != 0).all() and (want[0] == 1).sum() > 1000


SPECIAL = [0.0, 0.005, 0.004999999999999999, 0.994, 0.995, 9.994999999999999, 9.995, 9.996, 99.995, 99.99499999999999, 999.995,
           9999.995, 99999.995, 999999.995, 9999999.995, 99999999.995, 1e9 - 0.005, 1e10 - 0.005, 1e11 - 0.005, 1e12 - 0.005, 0.125,
           0.375, 2.5, 1234567.125, 2.0 ** 42 + 0.125, math.nextafter(2.0 ** 43, 0.0) - 1.0]


def test_digits_of_values(native):
    rng = np.random.default_rng(5)
    side = math.nextafter(2.0 ** 43, 0.0)                    # the largest usable image
    vals = np.asarray(SPECIAL + [math.nextafter(v, 0.0) for v in SPECIAL[1:]] + [math.nextafter(v, math.inf) for v in SPECIAL])
    pts = rng.choice(vals, (600, 3, 2))
    pts[::2, :, 1] = rng.choice(vals[vals < 2.0], (300, 3))  # thin, so that the area stays below 2^43: long in x ...
    pts[1::2, :, 0] = rng.choice(vals[vals < 2.0], (300, 3))  # ... or in y
    pts[::7, 0, 0] = -3.0                                    # some clipped: intersections next to the special values
    want = check(native, _tri_table(pts, side, side))
    lengths = {len(v) for v in want[3].decode().replace("[", ",").replace("]", ",").replace(":", ",").split(",") if "." in v}
    assert lengths >= set(range(4, 17)) and {0, 1} <= set(want[0].tolist())
    # too_large: four turns round a 2^21 x 2^21 image; one turn is written with area 2^42
    s21 = float(2 ** 21)
    t = _tri_table(np.asarray([_wound(4, s21), _wound(1, s21) * 4, _wound(4, s21)[::-1]]), s21, s21)
    want = check(native, t)
    assert want[0].tolist() == [C.TOO_LARGE, C.TOO_LARGE, C.TOO_LARGE]
    t = _tri_table(np.asarray([_wound(1, s21), _wound(1, s21)[::-1]]), s21, s21)
    want = check(native, t)
    assert want[0].tolist() == [0, 0] and want[1].tolist() == [2.0 ** 42] * 2 and b'"area":4398046511104.00' in want[3]


def test_digits_of_ids(native):
    from deal_yolo_daya_amd import _native

    rng = np.random.default_rng(6)
    pts = rng.uniform(0, 500, (120, 4, 2))
    cat = rng.integers(0, 3, 120).astype(np.int32)           # the ids of unselected polygons are skipped, not reused
    cat[[0, 119]] = 2
    t = _tri_table(pts, 640, 480, n_rows=120, cat=cat)
    for base in (5, 95, 2 ** 31 - 50, 10 ** 15 - 7):         # 9 -> 10, 99 -> 100, 2^31 - 1 -> 2^31, 15 -> 16 digits inside the call
        want = check(native, t, img_base=base, ann_base=base + 1)
        assert f'"id":{base + 1},"image_id":{base},'.encode() in want[3] and f'"id":{base + 120},"image_id":{base + 119},'.encode() in want[3]
    top = 2 ** 53 - 1 - 120                                  # base + n just under 2^53
    want = check(native, t, img_base=top, ann_base=top)
    assert f'"id":{2 ** 53 - 2},"image_id":{2 ** 53 - 2},'.encode() in want[3]
    for bases in ((top + 1, 1), (1, top + 1), (-1, 1), (1, -1)):
        with pytest.raises(_native.NativeError, match="invalid argument"):
            native.coco_annotations(*t, *bases, 1)
        with pytest.raises(ValueError):
            C.coco_arrays(*t, *bases, 1)


def test_degenerate_tables(native):
    z = np.zeros(0)
    want = check(native, (z, np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), z, z, np.zeros(0, np.uint8)))   # no rows
    assert want[3] == b""
    want = check(native, (z, np.zeros(1, np.int32), np.zeros(5, np.int32), np.zeros(0, np.int32), np.ones(4), np.ones(4),
                          np.zeros(4, np.uint8)))                                                      # rows without polygons
    assert want[3] == b"" and want[2].tolist() == [0] * 4
    rng = np.random.default_rng(8)
    pts = rng.uniform(0, 400, (40, 5, 2))
    for cat, n_text in ((np.zeros(40, np.int32), 0),                                                   # no selected polygon
                        (np.eye(1, 40, 17, dtype=np.int32)[0] * 3, 1),                                 # exactly one printed: no comma
                        (np.r_[0, np.ones(38, np.int32), -4].astype(np.int32), 38)):                   # first and last not printed
        rows = np.r_[0, 0, np.arange(0, 40, 4)[1:], 40, 40].astype(np.int32)                           # empty rows at both ends
        r = len(rows) - 1
        t = (pts.reshape(-1), np.arange(0, 201, 5, dtype=np.int32), rows, cat, np.full(r, 640.0), np.full(r, 480.0), np.zeros(r, np.uint8))
        want = check(native, t)
        text = want[3].decode()
        assert text.count('{"id"') == n_text and not text.startswith(",") and not text.endswith(",") and ",," not in text
        assert text.count("},{") == max(n_text - 1, 0) and int(want[2].sum()) == n_text


def test_actions_and_areas_equal_k14(native):
    xy, pt_off, row_off, cls, W, H, st, nc = k14_table(np.random.default_rng(9), 700)
    cat, _, area, _, _ = native.audit_polygons(xy, pt_off, row_off, cls, W, H, st, nc)
    action, carea, kept, _ = native.coco_annotations(xy, pt_off, row_off, np.where(cls >= 0, cls + 1, 0), W, H, st)
    assert np.array_equal(action, cat) and (action <= 1).sum() > 300
    assert np.array_equal(carea.view(np.uint64)[action <= 1], area.view(np.uint64)[action <= 1]) and np.isnan(carea[action > 1]).all()
    assert kept.sum() == (action <= 1).sum()


def test_export_coco_csv_end_to_end(native, tmp_path):
    df = _table(300, 8)
    path = tmp_path / "t.csv"
    df.to_csv(path, index=False, encoding="utf-8-sig")
    got = P.export_coco_csv(str(path), tmp_path / "gpu.json", skipped_csv=str(tmp_path / "gpu.csv"))
    want = P.export_coco_csv(str(path), tmp_path / "ref.json", skipped_csv=str(tmp_path / "ref.csv"), backend=BE)
    assert open(got["output"], "rb").read() == open(want["output"], "rb").read() and got["annotations"] > 0
    assert open(got["skipped_output"], "rb").read() == open(want["skipped_output"], "rb").read()
    drop = ("output", "skipped_output")
    assert {k: v for k, v in got.items() if k not in drop} == {k: v for k, v in want.items() if k not in drop}


def test_four_exports_select_and_number_alike(native, tmp_path, monkeypatch):
    """tests/test_class_selection_cpu.py's table (6 rows in 3 chunks, images of at most 64 x 64) through K16, K23, K20 and K21"""
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 2)
    for classes, with_labels in S.CASES:
        S.check_steps(S.run_steps(S.table(), tmp_path, classes, with_labels, None), classes, with_labels)
