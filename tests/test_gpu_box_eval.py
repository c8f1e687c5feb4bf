"""K24 (scored box evaluation) on the MI355X: both ABI entries against the plain-Python restatement (tests/box_eval_ref.py),
every array bit for bit, on the smallest tables at which the kernels can go wrong (tests/box_eval_tables.py names the tile
sizes), and the step functions end to end over several chunks.  pycocotools is not installed: equality with it is not checked."""
import json

import numpy as np
import pandas as pd
import pytest

from box_eval_ref import ACC_NAMES, MATCH_NAMES, REC, THR, accumulate, check_evaluation, expected_evaluation, match_rows, same_arrays
from box_eval_tables import ACC_TILE, TILES, acc_table, dense_table, match_table

from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu
COL = P.BBOX_COL
T32 = np.linspace(0.05, 1.0, 32)
_WANT = {}


def _match_call(native, g, g_off, g_cls, d, d_off, d_cls, score, C, thr, max_dets):
    """dyd_eval_match_boxes with every output prefilled with a sentinel, so that an unwritten element shows"""
    g, d = np.ascontiguousarray(g, np.float64).reshape(-1), np.ascontiguousarray(d, np.float64).reshape(-1)
    g_off, d_off = np.ascontiguousarray(g_off, np.int32), np.ascontiguousarray(d_off, np.int32)
    g_cls, d_cls = np.ascontiguousarray(g_cls, np.int32), np.ascontiguousarray(d_cls, np.int32)
    score, thr = np.ascontiguousarray(score, np.float64), np.ascontiguousarray(thr, np.float64)
    ng, nd = int(g_off[-1]), int(d_off[-1])
    outs = [np.full(nd, -7, np.int32), np.full(nd, 0xDEADBEEF, np.uint32), np.full(nd, -7, np.int32), np.full(nd, -7.0),
            np.full(nd, -7.0), np.full(ng, 0xDEADBEEF, np.uint32), np.full(ng, -7.0)]
    p = native._ptr
    rc = native.lib().dyd_eval_match_boxes(p(g), p(g_off), p(g_cls), p(d), p(d_off), p(d_cls), p(score), len(g_off) - 1, int(C),
                                           p(thr), len(thr), int(max_dets), *(p(o) for o in outs))
    native.check(rc, "dyd_eval_match_boxes")
    return outs


def _check_match(native, key, table, thr=THR, max_dets=100):
    k = (key, tuple(np.asarray(thr).tolist()), max_dets)
    if k not in _WANT:
        _WANT[k] = match_rows(*table, thr, max_dets)
    same_arrays(_match_call(native, *table, thr, max_dets), _WANT[k], MATCH_NAMES, f"{key}, direct call")
    same_arrays(native.eval_match_boxes(*table, thr, max_dets), _WANT[k], MATCH_NAMES, f"{key}, wrapper")
    return _WANT[k]


def _acc_call(native, cls, score, tp, C, T, npig, rec=REC):
    cls, score, tp = np.ascontiguousarray(cls, np.int32), np.ascontiguousarray(score, np.float64), np.ascontiguousarray(tp, np.uint32)
    npig, rec = np.ascontiguousarray(npig, np.int64), np.ascontiguousarray(rec, np.float64)
    R = len(rec)
    outs = [np.full((C, T, R), -7.0), np.full((C, T, R), -7.0), *(np.full((C, T), -7.0) for _ in range(4)),
            np.full((C, T), -7, np.int64), np.full((C, T), -7, np.int64)]
    p = native._ptr
    rc = native.lib().dyd_eval_accumulate(p(cls), p(score), p(tp), len(cls), C, T, p(npig), p(rec), R, *(p(o) for o in outs))
    native.check(rc, "dyd_eval_accumulate")
    return outs


def _check_acc(native, table, what):
    want = accumulate(*table)
    same_arrays(_acc_call(native, *table), want, ACC_NAMES, f"{what}, direct call")
    same_arrays(native.eval_accumulate(*table, REC), want, ACC_NAMES, f"{what}, wrapper")


# ----------------------------------------------------------------------------------------------- matching
def test_k24_empty_tables(native):
    z4, zi, zo, zs = np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0)
    assert [len(v) for v in native.eval_match_boxes(z4, zo, zi, z4, zo, zi, zs, 2, THR)] == [0] * 7
    off = np.zeros(5, np.int32)
    assert [len(v) for v in _match_call(native, z4, off, zi, z4, off, zi, zs, 2, THR, 100)] == [0] * 7
    _check_acc(native, ([], [], [], 3, 2, [0, 4, 1]), "no detections")
    assert [v.size for v in native.eval_accumulate([], [], [], 0, 1, [], REC)] == [0] * 8


@pytest.mark.parametrize("C,thr", [(1, [0.5]), (3, THR), (40, T32)], ids=["C1_T1", "C3_T10", "C40_T32"])
def test_k24_group_rows(native, C, thr):
    """rows of the 16-lane launch: none / one side only, the tile filled exactly (16 GT boxes, 32 detections)"""
    (g, d), _ = TILES
    fixed = [(0, 0), (0, 5), (5, 0), (1, 1), (g, d), (g - 1, d - 1), (g, 1), (1, d), (0, d), (g, 0)]
    rng = np.random.default_rng(24)
    sizes = np.concatenate([np.asarray(fixed), np.stack([rng.integers(0, g + 1, 120), rng.integers(0, d + 1, 120)], axis=1)])
    rng.shuffle(sizes)
    _check_match(native, f"group{C}", match_table(sizes, 24 + C, n_classes=C), thr)


def test_k24_wave_rows(native):
    """rows that exceed the 16-lane tile by one on either side, the 64-lane tile filled exactly (64 GT boxes, 128 detections)"""
    (g, d), (G, D) = TILES
    fixed = [(g + 1, d), (g, d + 1), (g + 1, d + 1), (g + 1, 0), (0, d + 1), (G, D), (G - 1, D - 1), (G, 1), (1, D), (G, 0), (0, D)]
    rng = np.random.default_rng(25)
    sizes = np.concatenate([np.asarray(fixed), np.stack([rng.integers(0, G + 1, 30), rng.integers(0, D + 1, 30)], axis=1)])
    rng.shuffle(sizes)
    _check_match(native, "wave", match_table(sizes, 25), THR)


def test_k24_big_rows(native):
    """rows that exceed the 64-lane tile by one on either side, and one row of 300 GT boxes and 700 detections in 3 classes"""
    _, (G, D) = TILES
    sizes = [(3, 2), (G + 1, D), (G, D + 1), (G + 1, 0), (0, D + 1), (300, 700), (G + 1, D + 1), (4, 4), (1, D + 1), (G + 1, 1)]
    table = match_table(sizes, 26)
    _check_match(native, "big", table, THR)
    _check_match(native, "big", table, T32[::4], max_dets=20)


@pytest.mark.parametrize("max_dets", [100, 1])
def test_k24_max_dets_plus_one(native, max_dets):
    """a (row, class) of max_dets + 1 detections: in a 16-lane row (max_dets 1), a 64-lane row (101) and a big row (301, of which
    201 are cut at 100)"""
    rng = np.random.default_rng(27)
    sizes = [(3, max_dets + 1), (2, 3), (40, max_dets + 1), (5, 301)]
    g, g_off, g_cls, d, d_off, d_cls, score, C = match_table(sizes, 27, n_classes=2, special=False)
    for r in (0, 2, 3):
        d_cls[d_off[r]:d_off[r + 1]] = 1
    score = rng.random(len(score))                         # no ties: exactly one detection is cut in rows 0 and 2
    want = _check_match(native, f"max_dets{max_dets}", (g, g_off, g_cls, d, d_off, d_cls, score, C), [0.5, 0.9], max_dets)
    cut = want[0] == 1
    assert [int(cut[d_off[r]:d_off[r + 1]].sum()) for r in (0, 2, 3)] == [1, 1, 301 - max_dets]


def test_k24_hand_worked(native):
    """the cases of tests/test_box_eval_cpu.py, where the restatement's answers are derived by hand"""
    rows = [([[0, 0, 10, 10], [20, 20, 30, 30]], [[0, 0, 10, 10], [50, 50, 60, 60], [20, 20, 30, 30]], [0.9, 0.8, 0.7]),
            ([[0, 0, 10, 10], [0, 0, 10, 10]], [[0, 0, 10, 10]], [0.5]),
            ([[0, 0, 2, 1]], [[0, 0, 1, 1]], [0.3]),
            ([[0, 0, 10, 10], [1, 0, 10, 8]], [[0, 0, 6, 10], [1, 0, 10, 10]], [0.9, 0.8]),
            ([[0, 0, 10, 10]], [[0, 0, 10, 10], [0, 0, 10, 10]], [-0.0, 0.0]),
            ([[0, 0, 10, 10]], [[0, 0, 10, 10]] * 3, [np.nan, np.inf, 0.1]),
            ([[0, 0, 10, np.nan], [0, 0, 10, 10]], [[0, 0, np.nan, 10], [0, 0, 10, 10]], [0.9, 0.8])]
    g = np.asarray([b for r in rows for b in r[0]], np.float64)
    d = np.asarray([b for r in rows for b in r[1]], np.float64)
    g_off = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.int32)
    d_off = np.cumsum([0] + [len(r[1]) for r in rows]).astype(np.int32)
    table = (g, g_off, np.zeros(len(g), np.int32), d, d_off, np.zeros(len(d), np.int32), np.concatenate([r[2] for r in rows]), 1)
    state, tp, gt, iou, *_ = _check_match(native, "hand", table, [0.5, 0.75])
    assert tp.tolist() == [3, 0, 3, 3, 1, 1, 3, 3, 0, 0, 0, 3, 0, 3] and gt[3] == 1 and iou[4] == 0.5
    state1, *_ = _check_match(native, "hand", table, [0.5], max_dets=1)
    assert state1[d_off[4]:d_off[5]].tolist() == [0, 1] and state1[d_off[5]:d_off[6]].tolist() == [2, 2, 0]


def test_k24_dense_jittered_copies(native):
    """about 2,000 rows of at most 12 GT boxes; the matched sets differ between the thresholds"""
    table = dense_table(28)
    want = _check_match(native, "dense", table, THR)
    bits = np.asarray([bin(int(v)).count("1") for v in want[1]])
    assert ((bits > 0) & (bits < len(THR))).sum() > 1000


# ----------------------------------------------------------------------------------------------- accumulation
def test_k24_accumulate_segments(native):
    """class segments of 1 detection, one short of / exactly / one more than a tile of the walk, and 5,000; a class without
    detections and one without ground truth"""
    _check_acc(native, acc_table([1, ACC_TILE - 1, ACC_TILE, ACC_TILE + 1, 5000, 0, 40], 29, T=2), "segments")


@pytest.mark.parametrize("C,T", [(1, 1), (3, 10), (40, 32)])
def test_k24_accumulate_classes_and_thresholds(native, C, T):
    rng = np.random.default_rng(30 + C)
    _check_acc(native, acc_table(rng.integers(0, 120, C).tolist(), 30 + C, T=T, decimals=1), f"C={C} T={T}")


def test_k24_accumulate_from_matching(native):
    """the dense table's matching fed to the accumulation, as the step does"""
    table = dense_table(28)
    state, tp, *_ = _check_match(native, "dense", table, THR)
    ev = state == 0
    npig = np.bincount(table[2], minlength=3)
    _check_acc(native, (table[5][ev], table[6][ev], tp[ev], 3, len(THR), npig), "dense")


# ----------------------------------------------------------------------------------------------- rejected inputs
def test_k24_rejected_inputs(native):
    one, cls, sc = np.array([[0.0, 0.0, 1.0, 1.0]] * 2), np.zeros(2, np.int32), np.array([0.5, 0.4])
    off = np.array([0, 2], np.int32)
    ok = (one, off, cls, one, off, cls, sc, 1)
    native.eval_match_boxes(*ok, [0.5])
    for what, args, kw in (("monotone", (one, np.array([0, 2, 1, 2], np.int32), cls, one, np.array([0, 0, 1, 2], np.int32), cls, sc, 1), {}),
                           ("class id", (one, off, np.array([0, 1], np.int32), one, off, cls, sc, 1), {}),
                           ("class id", (one, off, cls, one, off, np.array([-1, 0], np.int32), sc, 1), {}),
                           ("T outside", ok, {"thr": []}), ("T outside", ok, {"thr": [0.5] * 33}),
                           ("max_dets", ok, {"max_dets": 0})):
        with pytest.raises(native.NativeError, match=what):
            _match_call(native, *args, kw.get("thr", [0.5]), kw.get("max_dets", 100))
        assert what.split()[0].encode() in native.lib().dyd_last_error()
    for what, args in (("T outside", ([0], [0.5], [1], 1, 0, [1])), ("T outside", ([0], [0.5], [1], 1, 33, [1])),
                       ("class id", ([1], [0.5], [1], 1, 1, [1])), ("not finite", ([0], [np.nan], [1], 1, 1, [1])),
                       ("npig", ([0], [0.5], [1], 1, 1, [-1]))):
        with pytest.raises(native.NativeError, match=what):
            _acc_call(native, *args)
    with pytest.raises(native.NativeError, match="ascending"):
        _acc_call(native, [0], [0.5], [1], 1, 1, [1], rec=[0.5, 0.1])


# ----------------------------------------------------------------------------------------------- step level
def ob(name, x1, y1, x2, y2, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x1, "y": y1}, {"x": x2, "y": y2}]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def test_step_over_several_chunks_and_csv(native, monkeypatch, tmp_path):
    """evaluate_boxes_frame with small chunks feeding one accumulation, against the restatement; the CSV entry's files reload to
    the frame entry's arrays"""
    rng = np.random.default_rng(31)
    names = ["car", "人", "dog"]
    gt, pred, conf = [], [], []
    for r in range(60):
        g = [ob(names[rng.integers(0, 3)], *(rng.integers(0, 50, 2).tolist()), *(rng.integers(60, 120, 2).tolist()))
             for _ in range(rng.integers(0, 6))]
        d = []
        for o in g:
            if rng.random() < 0.85:
                p = [dict(pt) for pt in o["polygon"]["ptList"]]
                p[1]["y"] = p[0]["y"] + (p[1]["y"] - p[0]["y"]) * [1.0, 0.9, 0.7, 0.55][rng.integers(0, 4)]
                d.append({"name": o["name"] if rng.random() < 0.9 else "dog", "polygon": {"ptList": p}})
        d += [ob("car", 1, 1, 30, 30)] * int(rng.integers(0, 2))
        gt.append(cell(*g)), pred.append(cell(*d)), conf.append(json.dumps(np.round(rng.random(len(d)), 1).tolist()))
    df_gt = pd.DataFrame({"source": [f"s{r}" for r in range(60)], COL: gt})
    order = rng.permutation(60)[:55]
    df_pred = pd.DataFrame({"source": [f"s{r}" for r in order] + ["extra"], COL: [pred[r] for r in order] + [cell(ob("car", 0, 0, 5, 5))],
                            "conf": [conf[r] for r in order] + ["[0.5]"]})
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 7)
    res = P.evaluate_boxes_frame(df_gt, df_pred, score_col="conf")
    kept = set(order.tolist())
    want = expected_evaluation(gt, [pred[r] if r in kept else "{}" for r in range(60)],
                               scores=[json.loads(conf[r]) if r in kept else None for r in range(60)], sources=df_gt["source"].tolist())
    check_evaluation(res, want)
    assert res.unpaired["key"].tolist() == ["extra"] and res.totals["rows_only_gt"] == 5 and res.totals["python_cells"] == 0
    df_gt.to_csv(tmp_path / "gt.csv", index=False, encoding="utf-8-sig")
    df_pred.to_csv(tmp_path / "pred.csv", index=False, encoding="utf-8-sig")
    out = P.evaluate_boxes_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "out", score_col="conf")
    assert sorted(out["paths"]) == ["classes", "curves", "missed", "rows"] and out["evaluated"] == res.totals["evaluated"]
    z = np.load(out["paths"]["curves"])
    assert z["classes"].tolist() == res.classes and np.array_equal(z["recall_points"], REC)
    same_arrays([z[k] for k in ("iou_thresholds", "precision", "score_at", "recall", "ap")],
                [res.iou_thresholds, res.precision, res.score_at, res.recall, res.ap], ["thr", "precision", "score_at", "recall", "ap"])
    assert pd.read_csv(out["paths"]["classes"], encoding="utf-8-sig")["tp"].tolist() == res.per_class["tp"].tolist()
