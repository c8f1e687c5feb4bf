"""K11 (box repair) on the MI355X: both ABI entries against the numpy restatement of tests/box_repair_ref.py — row lengths
around the 64-box chunk and past 1024, special values, boxes landing on the image edge, 20 and 5,000 classes (LDS and global
class counters) — then the step functions on synthetic tables of 100k and 1M rows against the definition, and the invariants
(idempotence, the audit after the repair, YOLO label lines in [0, 1])."""

import numpy as np
import pytest

from box_repair_ref import check_repair, repair_arrays, repair_table
from test_gpu_box_audit import _synthetic_frame, _table

from deal_yolo_daya_amd import _native
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu
COL = P.BBOX_COL
SIZES = [0, 1, 63, 64, 65, 0, 2, 127, 128, 129, 1500, 3, 0, 0, 17, 256, 300, 64, 5]


def _sizes(rng, n=3000):
    return np.concatenate([SIZES, rng.integers(0, 40, n), [1025, 2049]])


def _with_edges(args, rng):
    """boxes one ulp past the image edge, on it, straddling it and wholly outside, added to _table's"""
    box4, row_off, cls, W, H, st = args
    box4 = box4.copy()
    B = len(cls)
    row = np.repeat(np.arange(len(W)), np.diff(row_off))
    if B:
        k = rng.random(B)
        Wb, Hb = W[row], H[row]
        e = k < 0.04
        box4[e, 2] = np.nextafter(Wb[e], np.inf)
        e = (k >= 0.04) & (k < 0.07)
        box4[e, 0], box4[e, 2] = -0.0, Wb[e]
        e = (k >= 0.07) & (k < 0.10)
        box4[e, 0], box4[e, 2] = Wb[e], Wb[e] + 30.0            # clipped to zero width: outside
        e = (k >= 0.10) & (k < 0.13)
        box4[e, 1], box4[e, 3] = -Hb[e], 0.5 * Hb[e]            # visible third
    return box4, row_off, cls, W, H, st


def _dev_call(box4, row_off, cls, W, H, status, n_classes, mv, ms, hz=None):
    """dyd_repair_boxes_dev on a delayed side stream through the harness of tests/stream_contract.py (`hz`: the caller's own,
    with its own decoys)"""
    import torch
    from stream_contract import Harness, box_table_decoy

    hz = hz or Harness(box_table_decoy(box4, row_off, cls, W, H, status, n_classes))

    dev = torch.device("cuda:0")
    n, B = len(row_off) - 1, len(cls)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_box, d_off, d_cls, d_w, d_h, d_st = t(box4.reshape(-1)), t(row_off), t(cls), t(W), t(H), t(status)
    act = torch.full((max(B, 1),), 0xEE, dtype=torch.uint8, device=dev)
    obox = torch.full((max(B, 1), 4), -7.0, dtype=torch.float64, device=dev)
    rows = torch.full((max(n, 1), 8), -7, dtype=torch.int32, device=dev)
    cc = torch.full((max(n_classes, 1), 8), -7, dtype=torch.int64, device=dev)
    hz.arm([d_box, d_off, d_cls, d_w, d_h, d_st])
    hz.watch(act, obox, rows, cc)
    rc = hz.call(_native.lib().dyd_repair_boxes_dev, d_box.data_ptr(), d_off.data_ptr(), n, B, d_cls.data_ptr(), d_w.data_ptr(),
                 d_h.data_ptr(), d_st.data_ptr(), n_classes, mv, ms, act.data_ptr(), obox.data_ptr(), rows.data_ptr(),
                 cc.data_ptr())
    _native.check(rc, "dyd_repair_boxes_dev")
    hz.restore()
    return act.cpu().numpy()[:B], obox.cpu().numpy()[:B], rows.cpu().numpy()[:n], cc.cpu().numpy()[:n_classes]


def _same(got, want):
    for nm, g, w in zip(("action", "box4", "row_counts", "class_counts"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, nm
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)          # bit for bit, -0.0 and NaN payloads included
        assert np.array_equal(g, w), f"{nm}: {int((g != w).sum())} entries differ"


@pytest.mark.parametrize("n_classes,mv,ms", [(20, 0.0, 0.0), (20, 0.5, 4.0), (5000, 0.0, 0.0), (5000, 0.3, 2.5),
                                             (256, 1.0, 0.0), (257, 0.0, 1.0), (1, 0.0, 0.0), (0, 0.2, 0.0)])
def test_both_entries_match_the_restatement(n_classes, mv, ms):
    rng = np.random.default_rng(n_classes * 7 + int(mv * 10) + int(ms))
    args = _with_edges(_table(_sizes(rng), n_classes, rng), rng)
    want = repair_arrays(*args, n_classes, mv, ms)
    _same(_native.repair_boxes(*args, n_classes, mv, ms), want)
    _same(_dev_call(*args, n_classes, mv, ms), want)
    code = want[0] & 7
    assert (code == 5).any() and (code == 3).any() and ((code == 1).any() or mv == 1.0)


def test_long_rows_and_one_class():
    rng = np.random.default_rng(3)
    args = _with_edges(_table(np.full(700, 256), 1, rng, special=False), rng)
    _same(_native.repair_boxes(*args, 1, 0.25, 3.0), repair_arrays(*args, 1, 0.25, 3.0))
    args = _with_edges(_table([70000, 0, 5], 20, rng), rng)
    _same(_dev_call(*args, 20, 0.0, 0.0), repair_arrays(*args, 20, 0.0, 0.0))


def test_entries_refuse_bad_arguments():
    rng = np.random.default_rng(1)
    args = _table([3, 4], 2, rng)
    for mv, ms in ((-0.1, 0.0), (1.1, 0.0), (0.0, -1.0), (0.0, np.inf)):
        with pytest.raises(ValueError):
            _native.repair_boxes(*args, 2, mv, ms)
        assert _native.lib().dyd_repair_boxes_dev(None, None, 0, 0, None, None, None, None, 0, mv, ms, None, None, None, None,
                                                  None) != 0
    box4, row_off, cls, W, H, st = args
    bad = cls.copy()
    bad[0] = 2
    with pytest.raises(_native.NativeError):
        _native.repair_boxes(box4, row_off, bad, W, H, st, 2)


@pytest.mark.parametrize("n", [100_000, 1_000_000])
def test_step_functions_on_synthetic_tables(n, tmp_path):
    rng = np.random.default_rng(n + 1)
    df = _synthetic_frame(n, rng)
    cells, w, h = df[COL].tolist(), df["width"].tolist(), df["height"].tolist()
    stats = {}
    out, ch, pc = P.repair_boxes_frame(df, min_visibility=0.2, min_size=1.0, stats=stats)
    ref = repair_table(cells, w, h, 0.2, 1.0)
    check_repair((out[COL].tolist(), ch, pc), ref, None, stats)
    assert stats["python_cells"] == 0 and stats["boxes_clipped"] > 0 and stats["boxes_removed"] > 0
    assert out.drop(columns=[COL]).equals(df.drop(columns=[COL]))
    if n == 100_000:
        path = tmp_path / "t.csv"
        df.to_csv(path, index=False, encoding="utf-8-sig")
        res = P.repair_boxes_csv(path, tmp_path / "o.csv", tmp_path / "c.csv", tmp_path / "k.csv", min_visibility=0.2,
                                 min_size=1.0)
        assert P.LAST_IO_PATH["repair"] == "native"
        for k, v in ref["totals"].items():
            assert res[k] == v, k
        import pandas as pd

        assert pd.read_csv(tmp_path / "o.csv", encoding="utf-8-sig")[COL].tolist() == ref["cells"]


def _yolo_numbers(texts):
    vals = [float(v) for t in texts if t for line in t.split("\n") for v in line.split()[1:]]
    return np.asarray(vals, np.float64)


def test_invariants_on_the_gpu():
    rng = np.random.default_rng(11)
    df = _synthetic_frame(100_000, rng)
    w, h = df["width"].tolist(), df["height"].tolist()
    out, ch, pc = P.repair_boxes_cells(df[COL].to_numpy(), w, h)
    again, ch2, _ = P.repair_boxes_cells(out, w, h)
    assert len(ch) > 0 and len(ch2) == 0 and all(a is b for a, b in zip(again, out))
    after = P.audit_boxes_cells(out, w, h)
    apc = after.per_class.set_index("class")
    assert (apc[["bad_coords", "degenerate", "out_of_image"]].to_numpy() == 0).all()
    rpc = pc.set_index("class")
    gone = rpc.index.difference(apc.index)
    assert (rpc.loc[gone, ["keep", "clip", "no_size"]].to_numpy() == 0).all()
    rpc = rpc.loc[apc.index]
    assert (apc["writable"] == rpc["keep"] + rpc["clip"]).all() and (apc["no_size"] == rpc["no_size"]).all()
    ok = np.flatnonzero(after.per_row["size_status"].to_numpy() == "ok")[:20000]
    names = [f"cls_{k % 20:02d}" for k in ok]
    texts, _ = P.yolo_label_texts([out[k] for k in ok], names, [k % 20 for k in ok], [w[k] for k in ok], [h[k] for k in ok])
    nums = _yolo_numbers(texts)
    assert len(nums) > 1000 and ((nums >= 0) & (nums <= 1)).all()
