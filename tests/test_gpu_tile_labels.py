"""K20 (tiled YOLO label lines, csrc/k20_tile.hip) through both C-ABI entries and tile_yolo_csv, against the restatement in
tests/tile_labels_ref.py.  Exact: every output array and the text bytes.  Needs a real MI355X."""
import ctypes as C
import json
import math

import numpy as np
import pandas as pd
import pytest

import tile_labels_ref as R
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu

NAMES = ("row_status", "tile_off", "tile_line_count", "text_off", "action", "tiles_written", "tiles_cut", "tiles_dropped", "text")


def table(rows):
    """rows = [(W, H, [(class id, [(x, y)])])] -> (xy, pt_off, row_off, cls, width, height)"""
    xy, pt_off, row_off, cls, W, H = [], [0], [0], [], [], []
    for w, h, polys in rows:
        for c, pts in polys:
            xy += [v for p in pts for v in p]
            pt_off.append(pt_off[-1] + len(pts))
            cls.append(c)
        row_off.append(len(cls))
        W.append(w)
        H.append(h)
    return (np.asarray(xy, np.float64), np.asarray(pt_off, np.int32), np.asarray(row_off, np.int32), np.asarray(cls, np.int32),
            np.asarray(W, np.float64), np.asarray(H, np.float64))


def random_rows(rng, n_rows, max_polys=8, max_pts=45, max_size=300, class_ids=(0, 10, 100)):
    rows = []
    for _ in range(n_rows):
        w, h = int(rng.integers(8, max_size + 1)), int(rng.integers(8, max_size + 1))
        wide = rng.random() < 0.2                                         # about one row in five reaches outside the image
        polys = []
        for _ in range(int(rng.integers(0, max_polys + 1))):
            m = int(rng.integers(2, max_pts + 1)) if rng.random() < 0.3 else int(rng.integers(2, 9))
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            r = rng.choice([4.0, 20.0, 90.0])
            pts = np.stack([cx + rng.uniform(-r, r, m), cy + rng.uniform(-r, r, m)], axis=1)
            if not wide:
                pts = np.clip(pts, 0, [w, h])
            if rng.random() < 0.5:
                pts = np.round(pts)                                       # vertices on tile edges and repeated vertices
            if rng.random() < 0.03:
                pts[rng.integers(0, m), rng.integers(0, 2)] = rng.choice([np.nan, np.inf, 2.0 ** 43])
            c = -1 if rng.random() < 0.1 else int(rng.choice(class_ids))
            polys.append((c, [tuple(p) for p in pts.tolist()]))
        if rng.random() < 0.08:
            w = rng.choice([0.0, w + 0.5, math.nan, -3.0])                # rows that are not tiled
        rows.append((w, h, polys))
    return rows


def same(got, want):
    for g, w, what in zip(got, want, NAMES):
        if what == "text":
            assert bytes(g) == bytes(w), what
        else:
            assert np.asarray(g).dtype == np.asarray(w).dtype and np.array_equal(g, w), what


def run_dev(t, params, phase=0, measure_only=False, text_cap=None, hz=None):
    """the _dev entry on torch tensors: outputs at odd offsets inside guarded buffers, the text at `phase` bytes past a 16-byte
    boundary -> (the nine outputs, return code, *out_total).  hz: the harness of tests/stream_contract.py (its decoys in the
    table's order), armed anew for both calls; without one the calls go to torch's current stream"""
    import torch
    from deal_yolo_daya_amd import _native
    from stream_contract import PLAIN

    hz = hz or PLAIN
    xy, pt_off, row_off, cls, W, H = t
    tw, th, sx, sy, mv, mode, mx = params
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    n, nb, npnt = len(W), len(cls), len(xy) // 2
    d_xy = torch.zeros(len(xy) + 4, dtype=torch.float64, device=dev)
    d_xy[2:2 + len(xy)] = up(xy)
    d_pt, d_row, d_cls, d_w, d_h = up(pt_off), up(row_off), up(cls), up(W), up(H)
    _, nx, ny = P._fl.tile_grid(W, H, tw, th, sx, sy, mx)
    T = int((nx * ny).sum())
    g8, g32, g64 = 0xA5, -7, -7
    status = torch.full((n + 2,), g8, dtype=torch.uint8, device=dev)
    act = torch.full((nb + 2,), g8, dtype=torch.uint8, device=dev)
    tile_off = torch.full((n + 3,), g64, dtype=torch.int64, device=dev)
    text_off = torch.full((T + 3,), g64, dtype=torch.int64, device=dev)
    lines = torch.full((T + 2,), g32, dtype=torch.int32, device=dev)
    wr, cut, drop = (torch.full((nb + 2,), g32, dtype=torch.int32, device=dev) for _ in range(3))
    L = _native.lib()
    n_tiles, total = C.c_int64(-1), C.c_int64(-1)
    hz.arm([d_xy[2:2 + len(xy)], d_pt, d_row, d_cls, d_w, d_h])
    hz.watch(status, act, tile_off, text_off, lines, wr, cut, drop)

    def call(text_ptr, cap):
        return hz.call(L.dyd_yolo_tile_lines_dev, d_xy.data_ptr() + 16, d_pt.data_ptr(), d_row.data_ptr(), d_cls.data_ptr(),
                       d_w.data_ptr(), d_h.data_ptr(), n, nb, npnt, tw, th, sx, sy, float(mv), mode, mx, T, status.data_ptr() + 1,
                       tile_off.data_ptr() + 8, lines.data_ptr() + 4, text_off.data_ptr() + 8, act.data_ptr() + 1,
                       wr.data_ptr() + 4, cut.data_ptr() + 4, drop.data_ptr() + 4, C.byref(n_tiles), text_ptr, cap,
                       C.byref(total))

    rc = call(None, 0)
    assert rc == 0, L.dyd_last_error()
    assert n_tiles.value == T
    size = total.value
    text = b""
    if not measure_only:
        cap = size if text_cap is None else text_cap
        buf = torch.full((64 + 16 + size + 64,), 0x7e, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        at = 64 + phase
        hz.watch(buf)
        rc = call(buf.data_ptr() + at, cap)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        if rc == 0:
            text = out[at:at + size].tobytes()
            assert (out[:at] == 0x7e).all() and (out[at + size:] == 0x7e).all(), "write outside the text"
        else:
            assert (out == 0x7e).all()
    hz.restore()
    arrays = []
    for a, off, fill in ((status, 1, g8), (tile_off, 1, g64), (lines, 1, g32), (text_off, 1, g64), (act, 1, g8), (wr, 1, g32),
                         (cut, 1, g32), (drop, 1, g32)):
        a = a.cpu().numpy()
        assert (a[:off] == fill).all() and a[-1] == fill, "write outside the outputs"
        arrays.append(a[off:len(a) - 1])
    return (*arrays, text), rc, total.value


def both(native, t, params, want=None):
    want = R.tile_arrays(*t, *params) if want is None else want
    same(native.yolo_tile_lines(*t, *params), want)
    got, rc, total = run_dev(t, params)
    assert rc == 0 and total == len(want[-1])
    same(got, want)
    return want


# ----------------------------------------------------------------------------------------------- random tables
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(native, seed):
    rng = np.random.default_rng(seed)
    t = table(random_rows(rng, 40))
    tile = (int(rng.integers(32, 65)), int(rng.integers(32, 65)))
    step = (int(rng.integers(16, tile[0] + 1)), int(rng.integers(16, tile[1] + 1)))
    seen = set()
    for mode in (0, 1):
        for mv in (0.0, 0.3, 1.0):
            want = both(native, t, (*tile, *step, mv, mode, 4096))
            seen |= set(want[4].tolist())
            assert len(want[-1]) > 2000 and want[6].sum() > 0 and (mv == 0.0 or want[7].sum() > 0)
    assert {0, 1, 4, 255} <= seen and {1, 2} & set(want[0].tolist())


# ----------------------------------------------------------------------------------------------- hand-worked cases
BOX = [(0, [(5.0, 2.0), (15.0, 8.0)])]


def test_known_answers(native):
    t = table([(20, 10, BOX)])
    want = both(native, t, (10, 10, 10, 10, 0.5, 0, 4096))
    assert want[-1] == (b"0 0.500000 0.200000 1.000000 0.200000 1.000000 0.800000 0.500000 0.800000"
                        b"0 0.000000 0.200000 0.500000 0.200000 0.500000 0.800000 0.000000 0.800000")
    assert (want[5].tolist(), want[6].tolist(), want[7].tolist()) == ([2], [2], [0])
    want = both(native, t, (10, 10, 10, 10, 0.5000000000000001, 0, 4096))
    assert want[-1] == b"" and (want[5].tolist(), want[7].tolist()) == ([0], [2])
    want = both(native, t, (10, 10, 10, 10, 0.0, 1, 4096))
    assert want[-1] == b"0 0.750000 0.500000 0.500000 0.6000000 0.250000 0.500000 0.500000 0.600000"
    tri = table([(20, 10, [(0, [(5.0, 2.0), (10.0, 5.0), (5.0, 8.0)])])])        # a vertex on the shared edge x = 10
    want = both(native, tri, (10, 10, 10, 10, 0.0, 0, 4096))
    assert want[2].tolist() == [1, 0] and (want[5].tolist(), want[6].tolist(), want[7].tolist()) == ([1], [0], [0])
    grid = table([(25, 11, BOX), (10, 10, BOX), (7, 25, BOX)])                   # L = 25, T = 10, S = 8; L = T + 1; L <= T
    want = both(native, grid, (10, 10, 8, 10, 0.0, 0, 4096))
    assert want[1].tolist() == [0, 6, 7, 10]
    bad = table([(0, 10, BOX), (20.5, 10, BOX), (100, 100, BOX), (20, 10, BOX)])
    want = both(native, bad, (10, 10, 10, 10, 0.0, 0, 99))
    assert want[0].tolist() == [1, 2, 3, 0] and want[1].tolist() == [0, 0, 0, 0, 2] and want[4].tolist() == [5, 0, 0, 0]


def test_polygons_that_span_three_tiles_in_both_axes(native):
    star = [(c, [(50 + 45 * math.cos(a * 0.7) * (1 if a % 2 else 0.4), 50 + 45 * math.sin(a * 0.7) * (1 if a % 2 else 0.4))
                 for a in range(9)]) for c in (0, 10)]
    t = table([(100, 100, star + [(100, [(2.0, 3.0), (97.0, 99.0)])])])
    want = both(native, t, (30, 30, 25, 25, 0.05, 0, 4096))
    assert want[1].tolist() == [0, 16] and (want[5] >= 8).all() and (want[6] > 0).all()
    both(native, t, (30, 30, 25, 25, 0.05, 1, 4096))


@pytest.mark.parametrize("n_polys", [0, 1, 65, 300])
def test_rows_of_many_polygons(native, n_polys):
    rng = np.random.default_rng(n_polys)
    polys = []
    for k in range(n_polys):
        m = int(rng.integers(2, 12))
        c = rng.uniform(0, 120, 2)
        polys.append(((0, 10, 100)[k % 3], [tuple(p) for p in (c + rng.uniform(-25, 25, (m, 2))).tolist()]))
    t = table([(120, 120, polys[:n_polys // 2]), (64, 64, []), (120, 90, polys[n_polys // 2:])])
    want = both(native, t, (48, 40, 30, 30, 0.1, 0, 4096))
    assert n_polys == 0 or len(want[-1]) > 0
    both(native, t, (48, 40, 30, 30, 0.1, 1, 4096))


def test_long_text_at_every_phase(native):
    """one 256 x 256 image, tile 32, step 16, 60 polygons: 225 tiles whose text runs past several print windows; the text
    buffer at every 16-byte phase"""
    rng = np.random.default_rng(5)
    polys = []
    for k in range(60):
        m = int(rng.integers(3, 30))
        c = rng.uniform(20, 236, 2)
        polys.append(((0, 10, 100)[k % 3], [tuple(p) for p in (c + rng.uniform(-40, 40, (m, 2))).tolist()]))
    t = table([(256, 256, polys)])
    params = (32, 32, 16, 16, 0.0, 0, 4096)
    want = R.tile_arrays(*t, *params)
    assert want[1].tolist() == [0, 225] and len(want[-1]) > 4 * 8192
    same(native.yolo_tile_lines(*t, *params), want)
    for phase in range(16):
        got, rc, total = run_dev(t, params, phase=phase)
        assert rc == 0 and total == len(want[-1]), phase
        same(got, want)


def test_tiles_without_lines_between_tiles_with_lines(native):
    small = [(0, [(2.0, 2.0), (8.0, 2.0), (8.0, 8.0)]), (10, [(82.0, 2.0), (88.0, 2.0), (88.0, 8.0)]),
             (100, [(42.0, 42.0), (48.0, 42.0), (48.0, 48.0)])]
    t = table([(90, 50, small), (30, 30, []), (90, 50, small[::-1])])
    want = both(native, t, (10, 10, 10, 10, 0.1, 0, 4096))
    assert want[2].tolist().count(1) == 6 and want[2].sum() == 6 and want[2][0] == 1 and want[2][1] == 0
    both(native, t, (10, 10, 10, 10, 0.1, 1, 4096))


def test_empty_inputs(native):
    none = (np.zeros(0), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    want = both(native, none, (10, 10, 10, 10, 0.1, 0, 4096))                  # n_rows == 0
    assert want[1].tolist() == [0] and want[3].tolist() == [0] and want[-1] == b""
    t = table([(20, 10, [(-1, BOX[0][1])]), (20, 10, [])])                      # no selected polygon
    want = both(native, t, (10, 10, 10, 10, 0.0, 0, 4096))
    assert want[4].tolist() == [255] and want[2].tolist() == [0, 0, 0, 0] and want[-1] == b""


def test_measure_only_and_a_text_cap_that_is_too_small(native):
    t = table(random_rows(np.random.default_rng(8), 12))
    params = (40, 40, 30, 30, 0.2, 0, 4096)
    want = R.tile_arrays(*t, *params)
    assert len(want[-1]) > 100
    got, rc, total = run_dev(t, params, measure_only=True)
    assert rc == 0 and total == len(want[-1])
    same(got[:-1], want[:-1])
    got, rc, total = run_dev(t, params, text_cap=len(want[-1]) - 1)
    assert rc == -5 and total == len(want[-1])                                   # DYD_ERR_RANGE with the exact size
    assert b"too small" in native.lib().dyd_last_error()
    same(got[:-1], want[:-1])


@pytest.mark.parametrize("bad", [dict(step_x=11), dict(tile_w=0, step_x=0), dict(tile_h=0), dict(step_y=0), dict(min_visibility=math.nan),
                                 dict(min_visibility=1.5), dict(mode=2), dict(max_tiles_per_row=0), dict(tile_w=2 ** 20 + 1)])
def test_invalid_parameters_are_the_argument_error(native, bad):
    xy, pt_off, row_off, cls, W, H = table([(20, 10, BOX)])
    kw = dict(tile_w=10, tile_h=10, step_x=10, step_y=10, min_visibility=0.1, mode=0, max_tiles_per_row=4096)
    kw.update(bad)
    out = [np.zeros(8, d) for d in (np.uint8, np.int64, np.int32, np.int64, np.uint8, np.int32, np.int32, np.int32)]
    text, total, n_tiles = C.c_void_p(), C.c_int64(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    L = native.lib()
    rc = L.dyd_yolo_tile_lines(p(xy), p(pt_off), p(row_off), p(cls), p(W), p(H), 1, kw["tile_w"], kw["tile_h"], kw["step_x"],
                               kw["step_y"], kw["min_visibility"], kw["mode"], kw["max_tiles_per_row"], 2, *[p(a) for a in out],
                               C.byref(n_tiles), C.byref(text), C.byref(total))
    assert rc == -1 and b"invalid argument" in L.dyd_last_error() and not text.value
    rc = L.dyd_yolo_tile_lines_dev(None, None, None, None, None, None, 0, 0, 0, kw["tile_w"], kw["tile_h"], kw["step_x"],
                                   kw["step_y"], kw["min_visibility"], kw["mode"], kw["max_tiles_per_row"], 0, *[None] * 8,
                                   C.byref(n_tiles), None, 0, C.byref(total), None)
    assert rc == -1


def test_tile_arrays_that_are_too_small_report_the_count(native):
    xy, pt_off, row_off, cls, W, H = table([(20, 10, BOX)])
    out = [np.zeros(8, d) for d in (np.uint8, np.int64, np.int32, np.int64, np.uint8, np.int32, np.int32, np.int32)]
    text, total, n_tiles = C.c_void_p(), C.c_int64(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    rc = native.lib().dyd_yolo_tile_lines(p(xy), p(pt_off), p(row_off), p(cls), p(W), p(H), 1, 10, 10, 10, 10, 0.1, 0, 4096, 1,
                                          *[p(a) for a in out], C.byref(n_tiles), C.byref(text), C.byref(total))
    assert rc == -5 and n_tiles.value == 2 and out[1][:2].tolist() == [0, 2] and not text.value


# ----------------------------------------------------------------------------------------------- end to end
def test_tile_yolo_csv_end_to_end(native, tmp_path):
    rng = np.random.default_rng(21)
    names = ["a", "b", "c"]
    cells, rows = [], random_rows(rng, 50, max_polys=5, max_pts=12, max_size=120, class_ids=(0, 1, 2))
    for _, _, polys in rows:
        cells.append(json.dumps({"objects": [{"name": names[max(c, 0)], "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}
                                             for c, pts in polys if all(map(math.isfinite, sum(pts, ())))]}))
    df = pd.DataFrame({"source": [f"im{k}.jpg" for k in range(50)], P.ANNOTATION_COL: cells,
                       "width": [r[0] for r in rows], "height": [r[1] for r in rows]})
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    res = P.tile_yolo_csv(src, tmp_path / "ds", tile=48, step=32, min_visibility=0.25, classes=names, lost_csv=tmp_path / "lost.csv")
    back = pd.read_csv(src, encoding="utf-8-sig")

    from helpers import OracleBackend
    ref_be = type("RefBackend", (OracleBackend,), {"yolo_tile_lines": staticmethod(R.tile_arrays)})()
    want = P.tile_yolo_frame(back, tmp_path / "ref", tile=48, step=32, min_visibility=0.25, classes=names,
                             lost_csv=tmp_path / "ref_lost.csv", backend=ref_be)
    strip = ("output_dir", "manifest", "lost_output")
    assert {k: v for k, v in res.items() if k not in strip} == {k: v for k, v in want.items() if k not in strip}
    files = sorted(p.name for p in (tmp_path / "ds" / "labels" / "train").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "ref" / "labels" / "train").iterdir()) and len(files) > 30
    for f in files:
        assert (tmp_path / "ds" / "labels" / "train" / f).read_bytes() == (tmp_path / "ref" / "labels" / "train" / f).read_bytes()
    assert (tmp_path / "ds" / "tiles_train.csv").read_bytes() == (tmp_path / "ref" / "tiles_train.csv").read_bytes()
    assert (tmp_path / "lost.csv").read_bytes() == (tmp_path / "ref_lost.csv").read_bytes()
    assert res["lines"] > 50 and res["tiles_cut"] > 0
