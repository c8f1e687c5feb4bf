"""K13 (YOLO segmentation label lines, csrc/k13_seg.hip) through both C-ABI entries and yolo_seg_label_texts, against the
restatement in tests/yolo_seg_ref.py.  Byte-exact.  Needs a real MI355X."""
import ctypes as C
import random

import numpy as np
import pytest

import yolo_seg_ref as R
from test_yolo_host_cpu import _Sheets
from test_yolo_seg_cpu import _frames, _run
from deal_yolo_daya_amd import synth
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu


def random_table(rng, n_rows, max_polys=40, max_pts=30, special=True, with_sel=True):
    xy, pt_off, row_off = [], [0], [0]
    W = rng.choice([640.0, 1280.0, 1920.0, 333.0], size=n_rows)
    H = rng.choice([480.0, 720.0, 1080.0, 77.0], size=n_rows)
    cid = rng.integers(0, 1200, size=n_rows).astype(np.int32)
    if special:
        k = rng.integers(0, n_rows, size=max(1, n_rows // 20))
        W[k[::3]] = rng.choice([np.nan, -1.0, 0.0, np.inf, 2.0 ** 43])
        cid[k[1::3]] = -3
    for i in range(n_rows):
        for _ in range(int(rng.integers(0, max_polys + 1))):
            n = int(rng.integers(0, max_pts + 1))
            cx, cy = rng.uniform(0, W[i] if np.isfinite(W[i]) and W[i] > 0 else 100), rng.uniform(0, H[i])
            r = rng.uniform(1, 80) if rng.random() > 0.2 else rng.uniform(100, 900)   # about 20 % cross an edge
            pts = np.stack([cx + rng.uniform(-r, r, n), cy + rng.uniform(-r, r, n)], 1)
            if special and rng.random() < 0.05:
                pts[rng.integers(0, max(n, 1)) if n else 0:][:1] = rng.choice([np.nan, np.inf, 2.0 ** 43, -0.0, 0.0])
            if rng.random() < 0.05 and n:
                pts[:, 0] = rng.choice([0.0, W[i]])                         # on a border
            xy.append(pts.reshape(-1))
            pt_off.append(pt_off[-1] + n)
        row_off.append(len(pt_off) - 1)
    xy = np.concatenate(xy) if xy else np.zeros(0)
    sel = (rng.random(len(pt_off) - 1) < 0.8).astype(np.uint8) if with_sel else None
    return xy, np.asarray(pt_off, np.int32), np.asarray(row_off, np.int32), sel, W, H, cid


def check(native, xy, pt_off, row_off, sel, W, H, cid):
    got = native.yolo_seg_lines(xy, pt_off, row_off, sel, W, H, cid)
    want = R.seg_arrays(xy, pt_off, row_off, sel, W, H, cid)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2])
    assert got[3] == want[3]
    dev = check_dev(xy, pt_off, row_off, sel, W, H, cid)
    assert np.array_equal(dev[0], want[0]) and np.array_equal(dev[1], want[1]) and np.array_equal(dev[2], want[2])
    assert dev[3] == want[3]
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
    total = C.c_int64()
    args = (d_xy.data_ptr(), d_pt.data_ptr(), d_row.data_ptr(), d_sel.data_ptr() if d_sel is not None else None, d_w.data_ptr(),
            d_h.data_ptr(), d_cid.data_ptr(), n, nb, npnt, toff.data_ptr(), flag.data_ptr(), act.data_ptr())
    hz.arm([d_xy, d_pt, d_row, d_sel, d_w, d_h, d_cid])
    hz.watch(toff, flag, act)
    _native.check(hz.call(L.dyd_yolo_seg_lines_dev, *args, None, 0, C.byref(total)), "measure")
    T = total.value
    if T:
        small = torch.empty(T - 1 if T > 1 else 1, dtype=torch.uint8, device=dev)
        rc = hz.call(L.dyd_yolo_seg_lines_dev, *args, small.data_ptr(), T - 1, C.byref(total))
        assert rc != 0 and total.value == T                                    # DYD_ERR_RANGE with the needed size
    buf = torch.full((T + offset + 32,), 0xAB, dtype=torch.uint8, device=dev)
    hz.watch(buf)
    _native.check(hz.call(L.dyd_yolo_seg_lines_dev, *args, buf.data_ptr() + offset, T, C.byref(total)), "print")
    hz.restore()
    b = buf.cpu().numpy()
    assert (b[:offset] == 0xAB).all() and (b[offset + T:] == 0xAB).all()      # nothing written outside the text
    return toff.cpu().numpy(), flag.cpu().numpy()[:n], act.cpu().numpy()[:nb], b[offset:offset + T].tobytes()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(native, seed):
    rng = np.random.default_rng(seed)
    check(native, *random_table(rng, 300, with_sel=seed != 2))


def test_long_shapes(native):
    rng = np.random.default_rng(7)
    # one polygon of 10,000 vertices crossing every edge
    a = np.linspace(0, 2 * np.pi, 10000, endpoint=False)
    big = np.stack([320 + 400 * np.cos(a), 240 + 300 * np.sin(a)], 1).reshape(-1)
    check(native, big, np.asarray([0, 10000], np.int32), np.asarray([0, 1], np.int32), None, np.asarray([640.0]), np.asarray([480.0]),
          np.asarray([12], np.int32))
    # a row of 2,000 polygons, then every polygon clipped, then empty tables
    xy, pt_off, row_off, sel, W, H, cid = random_table(rng, 1, max_polys=1, special=False)
    n = 2000
    pts = rng.uniform(-100, 700, (n, 6, 2))
    pt_off = np.arange(0, 6 * n + 1, 6, dtype=np.int32)
    check(native, pts.reshape(-1), pt_off, np.asarray([0, n], np.int32), None, np.asarray([640.0]), np.asarray([480.0]),
          np.asarray([3], np.int32))
    rows = np.arange(n + 1, dtype=np.int32)
    pts[:, 0, 0] = -5.0
    got = check(native, pts.reshape(-1), pt_off, rows, None, np.full(n, 640.0), np.full(n, 480.0), np.zeros(n, np.int32))
    assert (got[2] != 0).all()
    check(native, np.zeros(0), np.zeros(1, np.int32), np.zeros(5, np.int32), None, np.ones(4), np.ones(4), np.zeros(4, np.int32))
    off, flag, action, text = native.yolo_seg_lines(np.zeros(0), np.zeros(1, np.int32), np.zeros(1, np.int32), None, np.zeros(0),
                                                    np.zeros(0), np.zeros(0, np.int32))
    assert text == b"" and len(flag) == 0


def test_random_bit_patterns_in_the_image(native):
    rng = np.random.default_rng(11)
    n = 4000
    W, H = 1920.0, 1080.0
    u = rng.integers(0, 2 ** 63, (n * 5, 2), dtype=np.int64).view(np.float64)
    pts = np.abs(u)
    pts = np.where(np.isfinite(pts), pts, 0.0)
    pts[:, 0] = np.where(pts[:, 0] <= W, pts[:, 0], rng.uniform(0, W, n * 5))
    pts[:, 1] = np.where(pts[:, 1] <= H, pts[:, 1], rng.uniform(0, H, n * 5))
    check(native, pts.reshape(-1), np.arange(0, 5 * n + 1, 5, dtype=np.int32), np.arange(n + 1, dtype=np.int32), None,
          np.full(n, W), np.full(n, H), np.arange(n, dtype=np.int32) % 100)


def test_label_texts_on_synthetic_rows(native):
    t = synth.generate(1_000_000, seed=5)
    cells = synth.json_cells(t)
    n = t.n_rows
    first = t.label[t.box_off[:-1]]
    labels = [f"c{v}" for v in first.tolist()]                 # the row's first object carries its label
    cids = first.astype(int).tolist()
    ws, hs = [t.width] * n, [t.height] * n
    stats = {}
    texts, reasons = P.yolo_seg_label_texts(cells, labels, cids, ws, hs, native, stats)
    assert stats["rows"] == n and stats["polygons"] == sum(stats[a] for a in R.ACTIONS) > n
    assert stats["clipped"] > 0 and stats["written"] > stats["clipped"]
    totals = {a: 0 for a in R.ACTIONS}
    for i in random.Random(3).sample(range(n), 20_000):
        want = R.seg_row(cells[i], labels[i], cids[i], ws[i], hs[i])
        assert (texts[i], reasons[i]) == want[:2], i
        for a in want[2]:
            totals[a] += 1
    assert sum(totals.values()) > 20_000


def test_dev_on_10m_rows(native):
    import torch
    from deal_yolo_daya_amd import _native

    dev = torch.device("cuda", 0)
    d = synth.generate_device(10_000_000, 3, dev)
    xy, pt_off, row_off = d["xy"].contiguous(), d["pt_off"], d["box_off"]
    N, B, P_ = row_off.numel() - 1, pt_off.numel() - 1, xy.shape[0]
    W = torch.full((N,), 1920.0, dtype=torch.float64, device=dev)
    H = torch.full((N,), 1080.0, dtype=torch.float64, device=dev)
    cid = (torch.arange(N, device=dev, dtype=torch.int32) % 20).contiguous()
    toff = torch.empty(N + 1, dtype=torch.int64, device=dev)
    flag = torch.empty(N, dtype=torch.uint8, device=dev)
    act = torch.empty(B, dtype=torch.uint8, device=dev)
    L, sp, total = _native.lib(), torch.cuda.current_stream().cuda_stream, C.c_int64()
    args = (xy.data_ptr(), pt_off.data_ptr(), row_off.data_ptr(), None, W.data_ptr(), H.data_ptr(), cid.data_ptr(), N, B, P_,
            toff.data_ptr(), flag.data_ptr(), act.data_ptr())
    _native.check(L.dyd_yolo_seg_lines_dev(*args, None, 0, C.byref(total), sp), "measure")
    T = total.value
    text = torch.empty(T, dtype=torch.uint8, device=dev)
    _native.check(L.dyd_yolo_seg_lines_dev(*args, text.data_ptr(), T, C.byref(total), sp), "print")
    torch.cuda.synchronize()
    # every line is digits + 18 * m bytes: count the rows' bytes from the actions
    lines = text.cpu().numpy().tobytes()
    off = toff.cpu().numpy()
    a = act.cpu().numpy()
    rng = np.random.default_rng(0)
    pt_h, row_h = pt_off.cpu().numpy(), row_off.cpu().numpy()
    for i in rng.choice(N, 10_000, replace=False).tolist():
        b0, b1 = int(row_h[i]), int(row_h[i + 1])
        p0, p1 = int(pt_h[b0]), int(pt_h[b1])
        pts = xy[p0:p1].cpu().numpy().reshape(-1)
        loc = pt_h[b0:b1 + 1] - p0
        want = R.seg_arrays(pts, loc, np.asarray([0, b1 - b0]), None, [1920.0], [1080.0], [i % 20])
        assert lines[off[i]:off[i + 1]] == want[3], i
        assert np.array_equal(a[b0:b1], want[2])
    n_lines = 0
    for i in range(200_000):                                    # rows lie back to back: split each row's text on its own
        for line in lines[off[i]:off[i + 1]].split(b"\n"):
            parts = line.split(b" ")
            assert len(line) == len(parts[0]) + 18 * ((len(parts) - 1) // 2) and len(parts) % 2 == 1
            assert all(0.0 <= float(v) <= 1.0 and len(v) == 8 for v in parts[1:])
            n_lines += 1
    assert n_lines > 200_000


def test_generate_segment_on_the_device(native, tmp_path):
    import os

    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    want = _run(_frames(tmp_path / "a", True), tmp_path / "a", task="segment")             # the restatement as the device
    book = tmp_path / "b" / "cat.xlsx"
    book.write_bytes(b"")
    with _Sheets(_frames(tmp_path / "b", True)):
        got = P.generate_yolo_datasets_from_excels([str(book)], str(tmp_path / "b" / "out"), download_images=False, backend=native,
                                                   task="segment")
    n = 0
    for split in ("train", "val"):
        da, db = want["datasets"][0] / "labels" / split, got["datasets"][0] / "labels" / split
        assert sorted(os.listdir(da)) == sorted(os.listdir(db))
        for fn in os.listdir(da):
            assert (da / fn).read_bytes() == (db / fn).read_bytes()
            n += 1
    assert n == 40
