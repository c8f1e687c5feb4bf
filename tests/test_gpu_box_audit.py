"""K10 (box audit) on the MI355X: both ABI entries against the numpy restatement of tests/box_audit_ref.py — row lengths
around the 64-box chunk and past 1024, special values, 20 and 5,000 classes (LDS and global accumulation), nb in {1, 16, 64} —
and the step functions on synthetic tables of 100k and 1M rows against the definition."""

import numpy as np
import pandas as pd
import pytest

from box_audit_ref import audit_arrays, audit_table, check_audit

from deal_yolo_daya_amd import _native
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu
COL = P.BBOX_COL


def _table(sizes, n_classes, rng, special=True):
    """-> (box4 [B,4], row_off, cls, W, H, status) with boundary-landing values, every size status and unmatchable boxes"""
    sizes = np.asarray(sizes, np.int64)
    n = len(sizes)
    row_off = np.zeros(n + 1, np.int32)
    np.cumsum(sizes, out=row_off[1:])
    B = int(row_off[-1])
    W = rng.choice([640.0, 1024.0, 1280.0, 333.0], n)
    H = rng.choice([480.0, 768.0, 720.0, 77.0], n)
    status = rng.choice([0, 0, 0, 0, 0, 0, 1, 2], n).astype(np.uint8)
    row = np.repeat(np.arange(n), sizes)
    x1 = rng.uniform(-40, 1.05 * W[row])
    y1 = rng.uniform(-40, 1.05 * H[row])
    bw = rng.choice([0.0, 1.0, 31.9, 32.0, 96.0, 200.0], B) * rng.integers(0, 2, B) + rng.uniform(0, 120, B)
    bh = rng.uniform(0, 120, B)
    box4 = np.stack([x1, y1, x1 + bw, y1 + bh], axis=1)
    box4 = np.round(box4, 1)
    if B:
        k = rng.random(B)
        # boxes landing exactly on bin edges and on the image edge: xc = 0.5, wn = 1/4, x2 == W, v = 1.0
        e = np.flatnonzero(k < 0.05)
        Wb, Hb = W[row[e]], H[row[e]]
        box4[e] = np.stack([Wb / 4, Hb / 4, 3 * Wb / 4, 3 * Hb / 4], axis=1)
        e = np.flatnonzero((k >= 0.05) & (k < 0.08))
        box4[e] = np.stack([np.zeros(len(e)), np.zeros(len(e)), W[row[e]], H[row[e]]], axis=1)
        e = np.flatnonzero((k >= 0.08) & (k < 0.10))
        box4[e, 2] = box4[e, 0]                             # degenerate
        if special:
            e = np.flatnonzero((k >= 0.10) & (k < 0.12))
            box4[e, rng.integers(0, 4, len(e))] = rng.choice([np.nan, np.inf, -np.inf], len(e))
            e = np.flatnonzero((k >= 0.12) & (k < 0.13))
            box4[e, 0] = -1e308
            box4[e, 2] = 1e308                              # bw = inf: writable, clamped bins, large
    cls = rng.integers(0, n_classes, B).astype(np.int32) if n_classes else np.full(B, -1, np.int32)
    if B:
        cls[rng.random(B) < 0.03] = -1
    W[status != 0] = 0.0
    H[status != 0] = 0.0
    return box4, row_off, cls, W, H, status


SIZES = [0, 1, 63, 64, 65, 0, 2, 127, 128, 129, 1500, 3, 0, 0, 17, 256, 300, 64, 5]


def _sizes(rng, n=3000):
    return np.concatenate([SIZES, rng.integers(0, 40, n), [1025, 2049]])


def _dev_call(box4, row_off, cls, W, H, status, n_classes, nb, hz=None):
    """dyd_box_audit_dev on a delayed side stream through the harness of tests/stream_contract.py (`hz`: the caller's own,
    with its own decoys)"""
    import torch
    from stream_contract import Harness, box_table_decoy

    hz = hz or Harness(box_table_decoy(box4, row_off, cls, W, H, status, n_classes))

    dev = torch.device("cuda:0")
    n, B = len(row_off) - 1, len(cls)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_box, d_off, d_cls, d_w, d_h, d_st = t(box4.reshape(-1)), t(row_off), t(cls), t(W), t(H), t(status)
    flag = torch.full((max(B, 1),), 0xEE, dtype=torch.uint8, device=dev)
    rows = torch.full((max(n, 1), 6), -7, dtype=torch.int32, device=dev)
    cc = torch.full((max(n_classes, 1), 9), -7, dtype=torch.int64, device=dev)
    wh = torch.full((max(n_classes, 1) * nb * nb,), -7, dtype=torch.int64, device=dev)
    xy = torch.full_like(wh, -7)
    bpi = torch.full((257,), -7, dtype=torch.int64, device=dev)
    hz.arm([d_box, d_off, d_cls, d_w, d_h, d_st])
    hz.watch(flag, rows, cc, wh, xy, bpi)
    L = _native.lib()
    rc = hz.call(L.dyd_box_audit_dev, d_box.data_ptr(), d_off.data_ptr(), n, B, d_cls.data_ptr(), d_w.data_ptr(), d_h.data_ptr(),
                 d_st.data_ptr(), n_classes, nb, flag.data_ptr(), rows.data_ptr(), cc.data_ptr(), wh.data_ptr(),
                 xy.data_ptr(), bpi.data_ptr())
    assert hz.s.cuda_stream != 0
    _native.check(rc, "dyd_box_audit_dev")
    hz.restore()
    C_ = n_classes
    return (flag.cpu().numpy()[:B], rows.cpu().numpy()[:n], cc.cpu().numpy()[:C_],
            wh.cpu().numpy()[:C_ * nb * nb].reshape(C_, nb, nb), xy.cpu().numpy()[:C_ * nb * nb].reshape(C_, nb, nb),
            bpi.cpu().numpy())


def _same(got, want):
    names = ("flag", "row_counts", "class_counts", "hist_wh", "hist_xy", "boxes_per_image")
    for nm, g, w in zip(names, got, want):
        assert g.shape == w.shape, nm
        assert np.array_equal(g, w), f"{nm}: {int((g != w).sum())} entries differ"


@pytest.mark.parametrize("n_classes,nb", [(20, 16), (20, 1), (20, 64), (5000, 16), (5000, 64), (1, 64), (0, 16)])
def test_both_entries_match_the_restatement(n_classes, nb):
    rng = np.random.default_rng(n_classes * 131 + nb)
    args = _table(_sizes(rng), n_classes, rng)
    want = audit_arrays(*args, n_classes, nb)
    _same(_native.box_audit(*args, n_classes, nb), want)
    _same(_dev_call(*args, n_classes, nb), want)
    assert want[3].sum() > 0 or n_classes == 0


def test_dense_rows_and_one_class():
    rng = np.random.default_rng(7)
    args = _table(np.full(700, 256), 1, rng, special=False)
    _same(_native.box_audit(*args, 1, 16), audit_arrays(*args, 1, 16))
    args = _table([70000, 0, 5], 20, rng)                     # one row much longer than a tile
    _same(_dev_call(*args, 20, 64), audit_arrays(*args, 20, 64))


def test_entries_refuse_bad_arguments():
    rng = np.random.default_rng(1)
    args = _table([3, 4], 2, rng)
    for nb in (0, 65):
        with pytest.raises(ValueError):
            _native.box_audit(*args, 2, nb)
    box4, row_off, cls, W, H, st = args
    bad = cls.copy()
    bad[0] = 2
    with pytest.raises(_native.NativeError):
        _native.box_audit(box4, row_off, bad, W, H, st, 2, 16)


def _synthetic_frame(n, rng, n_classes=20):
    names = [f"cls_{k:02d}" for k in range(n_classes)]
    k = rng.integers(0, 12, n)
    W = rng.choice([640, 1280, 1920], n)
    H = rng.choice([480, 720, 1080], n)
    B = int(k.sum())
    row = np.repeat(np.arange(n), k)
    x1 = np.round(rng.uniform(-20, W[row] * 1.02), 2)
    y1 = np.round(rng.uniform(-20, H[row] * 1.02), 2)
    x2 = np.round(x1 + rng.uniform(0, 300, B), 2)
    y2 = np.round(y1 + rng.uniform(0, 300, B), 2)
    inj = rng.random(B)
    x2 = np.where(inj < 0.02, x1, x2)                        # degenerate
    x2 = np.where((inj >= 0.02) & (inj < 0.04), W[row] + 5.5, x2)   # out of image
    nm = rng.integers(0, n_classes, B)
    parts = [[] for _ in range(n)]
    for r, a, b, c, d, j in zip(row.tolist(), x1.tolist(), y1.tolist(), x2.tolist(), y2.tolist(), nm.tolist()):
        parts[r].append('{"name": "%s", "polygon": {"ptList": [{"x": %r, "y": %r}, {"x": %r, "y": %r}]}}'
                        % (names[j], a, b, c, d))
    cells = ['{"objects": [' + ", ".join(p) + "]}" for p in parts]
    w = W.astype(np.float64)
    w[rng.random(n) < 0.01] = np.nan                         # what pandas reads back for an empty size
    h = H.astype(np.int64)
    h[rng.random(n) < 0.01] = 0
    return pd.DataFrame({"source": [f"img_{i}.jpg" for i in range(n)], COL: cells, "width": w, "height": h})


@pytest.mark.parametrize("n", [100_000, 1_000_000])
def test_step_functions_on_synthetic_tables(n, tmp_path):
    rng = np.random.default_rng(n)
    df = _synthetic_frame(n, rng)
    a = P.audit_boxes_frame(df)
    check_audit(a, audit_table(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), 16))
    assert a.totals["python_cells"] == 0 and a.per_class["out_of_image"].sum() > 0 and a.per_class["degenerate"].sum() > 0
    assert a.per_row["source"].tolist()[:3] == ["img_0.jpg", "img_1.jpg", "img_2.jpg"]
    if n == 100_000:
        path = tmp_path / "t.csv"
        df.to_csv(path, index=False, encoding="utf-8-sig")
        res = P.audit_boxes_csv(path, tmp_path / "out", nbins=64)
        assert P.LAST_IO_PATH["audit"] == "native"
        b = P.audit_boxes_frame(pd.read_csv(path, encoding="utf-8-sig"), nbins=64)
        got = pd.read_csv(res["paths"]["classes"], encoding="utf-8-sig")
        assert got.equals(pd.read_csv(io_csv(b.per_class), encoding="utf-8-sig"))
        with np.load(res["paths"]["hist"]) as z:
            assert np.array_equal(z["hist_wh"], b.hist_wh) and np.array_equal(z["hist_xy"], b.hist_xy)
        assert res["boxes"] == b.totals["boxes"]


def io_csv(frame):
    import io

    buf = io.StringIO()
    frame.to_csv(buf, index=False)
    buf.seek(0)
    return buf
