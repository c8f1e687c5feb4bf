"""Scored box evaluation (core/processor.py: evaluate_boxes_*), host side: the restatement of K24 (tests/box_eval_ref.py)
pinned on hand-worked cases whose values are derived in the docstrings, then the argument checks, the score plumbing and the
row alignment of the step functions, driven by a test backend whose device stage is that restatement.  No GPU.

pycocotools is not installed here, so nothing in this file (or anywhere else) checks equality with it."""
import json

import numpy as np
import pandas as pd
import pytest

from box_eval_ref import ACC_NAMES, EPS, MATCH_NAMES, REC, accumulate, check_evaluation, expected_evaluation, match_rows, same_arrays
from helpers import OracleBackend

from deal_yolo_daya_amd.core import processor as P

COL = P.BBOX_COL
NAN = float("nan")


class EvalBackend(OracleBackend):
    def eval_match_boxes(self, gt_box4, gt_off, gt_cls, dt_box4, dt_off, dt_cls, dt_score, n_classes, iou_thr, max_dets=100):
        return match_rows(gt_box4, gt_off, gt_cls, dt_box4, dt_off, dt_cls, dt_score, n_classes, iou_thr, max_dets)

    def eval_accumulate(self, cls, score, tp, n_classes, n_thresholds, npig, rec):
        return accumulate(cls, score, tp, n_classes, n_thresholds, npig, rec)


BE = EvalBackend()


def ob(name, x1, y1, x2, y2, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x1, "y": y1}, {"x": x2, "y": y2}]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def one_row(gt, dt, score, thr=(0.5,), max_dets=100, gt_cls=None, dt_cls=None, C=1):
    """match_rows on one row of boxes, every box of class 0 unless told otherwise"""
    gt, dt = np.asarray(gt, np.float64).reshape(-1, 4), np.asarray(dt, np.float64).reshape(-1, 4)
    return match_rows(gt, [0, len(gt)], gt_cls or [0] * len(gt), dt, [0, len(dt)], dt_cls or [0] * len(dt), score, C, thr, max_dets)


def mean_in_order(values):
    total = 0.0
    for v in values:
        total += v
    return total / len(values)


FULL_AP = mean_in_order([1 - EPS] * 101)          # every recall point at 1/(1+eps)


def evaluate(cells_gt, cells_pred, **kw):
    res = P.evaluate_boxes_cells(cells_gt, cells_pred, backend=BE, **kw)
    want = expected_evaluation(cells_gt, cells_pred, **{k: v for k, v in kw.items() if k != "stats"})
    check_evaluation(res, want)
    return res


# ----------------------------------------------------------------------------------------------- the rule, by hand
def test_tp_fp_tp_curve():
    """One class, GT boxes A and B; detections: A itself (0.9), a box far away (0.8), B itself (0.7) -> TP, FP, TP.
    rc = 1/2, 1/2, 2/2.  pr = 1/(1+eps), 1/(2+eps), 2/(3+eps) with eps = 2^-52: 1/(1+2^-52) rounds to 1 - 2^-52 (the "1.0" of
    COCO's curves is that value), 2+eps and 3+eps round to 2 and 3, so pr = 1-2^-52, 0.5, 2/3; the running maximum from the
    right makes it 1-2^-52, 2/3, 2/3.  The recall points 0 .. 0.5 (51 of them: REC[50] is exactly 0.5) are first reached at
    k = 0, the 50 points above at k = 2.  F1 at the three run ends: 2/3, 2/4, 4/5 -> the last one."""
    state, tp, gt, iou, best, hit, g_best = one_row([[0, 0, 10, 10], [20, 20, 30, 30]],
                                                    [[0, 0, 10, 10], [50, 50, 60, 60], [20, 20, 30, 30]], [0.9, 0.8, 0.7])
    assert state.tolist() == [0, 0, 0] and tp.tolist() == [1, 0, 1] and gt.tolist() == [0, -1, 1]
    assert iou.tolist() == [1.0, 0.0, 1.0] and best.tolist() == [1.0, 0.0, 1.0]
    assert hit.tolist() == [1, 1] and g_best.tolist() == [1.0, 1.0]
    precision, score_at, recall, ap, f1, bs, btp, bd = accumulate([0, 0, 0], [0.9, 0.8, 0.7], tp, 1, 1, [2])
    top = 1 / (1 + EPS)
    assert REC[50] == 0.5 and top == 1 - EPS and 2 / (3 + EPS) == 2 / 3
    assert precision[0, 0].tolist() == [top] * 51 + [2 / 3] * 50
    assert score_at[0, 0].tolist() == [0.9] * 51 + [0.7] * 50
    assert recall[0, 0] == 1.0 and ap[0, 0] == mean_in_order([top] * 51 + [2 / 3] * 50)
    assert (f1[0, 0], bs[0, 0], btp[0, 0], bd[0, 0]) == (4 / 5, 0.7, 2, 3)


def test_equal_iou_takes_the_highest_gt_index():
    """two identical GT boxes and one detection on them: both IoUs are 1.0, and COCOeval's loop replaces on `>=`"""
    _, tp, gt, iou, _, hit, _ = one_row([[0, 0, 10, 10], [0, 0, 10, 10]], [[0, 0, 10, 10]], [0.5])
    assert tp.tolist() == [1] and gt.tolist() == [1] and iou.tolist() == [1.0] and hit.tolist() == [0, 1]


def test_iou_exactly_at_the_threshold_matches():
    """[0,0,2,1] against [0,0,1,1]: intersection 1, union 2 + 1 - 1 = 2, IoU exactly 0.5 >= 0.5"""
    _, tp, gt, iou, _, _, _ = one_row([[0, 0, 2, 1]], [[0, 0, 1, 1]], [0.3], thr=(0.5, 0.5000000001))
    assert tp.tolist() == [1] and gt.tolist() == [0] and iou.tolist() == [0.5]


def test_a_detection_takes_different_gt_boxes_at_different_thresholds():
    """GT A = [0,0,10,10], B = [1,0,10,8]; d1 = [0,0,6,10] (0.9), d2 = [1,0,10,10] (0.8); thresholds 0.5 and 0.75.
    IoU(A,d1) = 60/100 = 0.6, IoU(B,d1) = 40/(72+60-40) = 0.43, IoU(A,d2) = 90/100 = 0.9, IoU(B,d2) = 72/90 = 0.8.
    At 0.5: d1 takes A (B is below), so d2 finds only B free.  At 0.75: d1 takes nothing, A stays free and d2 takes it (0.9 > 0.8)."""
    state, tp, gt, iou, best, hit, g_best = one_row([[0, 0, 10, 10], [1, 0, 10, 8]], [[0, 0, 6, 10], [1, 0, 10, 10]], [0.9, 0.8],
                                                    thr=(0.5, 0.75))
    assert tp.tolist() == [0b01, 0b11] and gt.tolist() == [0, 1] and iou.tolist() == [0.6, 0.8]
    assert best.tolist() == [0.6, 0.9] and hit.tolist() == [0b11, 0b01] and g_best.tolist() == [0.9, 0.8]


def test_max_dets_one_cuts_the_lower_score():
    state, tp, *_ = one_row([[0, 0, 10, 10]], [[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]], [0.2, 0.9, 0.9], max_dets=1)
    assert state.tolist() == [1, 0, 1] and tp.tolist() == [0, 1, 0]            # of the two 0.9 the earlier position ranks first
    two = one_row([[0, 0, 10, 10]], [[0, 0, 10, 10], [0, 0, 10, 10]], [0.2, 0.9], max_dets=1, dt_cls=[0, 1], C=2)
    assert two[0].tolist() == [0, 0]                                           # the rank counts within the class


def test_equal_scores_across_rows_keep_table_order():
    """two detections of score 0.5, the first (row 0) a FP, the second (row 1) a TP, two GT boxes: pr = 0/(1+eps), 1/(2+eps) ->
    the envelope is 0.5, 0.5; were the TP taken first the curve would start at 1-2^-52"""
    precision, _, recall, *_ = accumulate([0, 0], [0.5, 0.5], [0, 1], 1, 1, [2])
    assert precision[0, 0].tolist() == [0.5] * 51 + [0.0] * 50 and recall[0, 0] == 0.5


def test_negative_zero_equals_zero():
    """-0.0 first, 0.0 second: equal numbers, so the earlier position ranks first and max_dets = 1 cuts the second"""
    state, *_ = one_row([[0, 0, 10, 10]], [[0, 0, 10, 10], [0, 0, 10, 10]], [-0.0, 0.0], max_dets=1)
    assert state.tolist() == [0, 1]
    _, score_at, *_ = accumulate([0], [-0.0], [1], 1, 1, [1])
    assert np.signbit(score_at[0, 0]).sum() == 0                               # reported as 0.0


def test_scores_that_are_not_finite_take_no_part():
    state, tp, gt, _, best, hit, _ = one_row([[0, 0, 10, 10]], [[0, 0, 10, 10]] * 3, [NAN, float("inf"), 0.1])
    assert state.tolist() == [2, 2, 0] and tp.tolist() == [0, 0, 1] and best.tolist() == [0.0, 0.0, 1.0] and hit.tolist() == [1]
    res = evaluate([cell(ob("a", 0, 0, 10, 10))], [cell(*[ob("a", 0, 0, 10, 10)] * 3)], scores=[[NAN, float("-inf"), 0.1]])
    assert res.per_class[["evaluated", "bad_score", "tp", "fp"]].values.tolist() == [[1, 2, 1, 0]]
    assert res.totals["map"] == mean_in_order([FULL_AP] * 10)


def test_nan_corner_on_either_side():
    """a GT box with a NaN corner is ground truth that nothing can match; a detection with one is evaluated and a FP"""
    state, tp, _, _, best, hit, g_best = one_row([[0, 0, 10, NAN], [0, 0, 10, 10]], [[0, 0, NAN, 10], [0, 0, 10, 10]], [0.9, 0.8])
    assert state.tolist() == [0, 0] and tp.tolist() == [0, 1] and hit.tolist() == [0, 1]
    assert best.tolist() == [0.0, 1.0] and g_best.tolist() == [0.0, 1.0]


def test_class_without_gt_is_undefined_and_class_without_detection_scores_zero():
    gt = [cell(ob("a", 0, 0, 10, 10), ob("b", 20, 20, 30, 30))]
    pred = [cell(ob("a", 0, 0, 10, 10), ob("c", 0, 0, 10, 10))]
    res = evaluate(gt, pred, scores=[[0.9, 0.8]], iou_thresholds=[0.5, 0.75])
    assert res.classes == ["a", "b", "c"]
    assert np.isnan(res.ap[2]).all() and np.isnan(res.precision[2]).all() and (res.ap[1] == 0.0).all()
    ap = res.per_class["ap"].tolist()
    assert ap[0] == mean_in_order([FULL_AP] * 2) and ap[1] == 0.0 and ap[2] != ap[2]
    assert res.totals["map"] == (ap[0] + 0.0) / 2 and res.totals["map50"] == res.totals["map"]
    assert res.per_class["fn"].tolist() == [0, 1, 0] and res.per_class["fp"].tolist() == [0, 0, 1]
    assert res.missed[["row", "object", "name", "best_iou"]].values.tolist() == [[0, 1, "b", 0.0]]


def test_best_f1_does_not_split_a_run_of_equal_scores():
    """scores 0.9 (TP), 0.5 (TP), 0.5 (FP), 0.5 (FP), two GT boxes.  After the second detection F1 would be 2*2/(2+2) = 1, but no
    cut "score >= s" ends there.  The run ends are k = 0 (2*1/(1+2) = 2/3) and k = 3 (2*2/(4+2) = 2/3): a tie, the smaller k."""
    *_, f1, bs, btp, bd = accumulate([0] * 4, [0.9, 0.5, 0.5, 0.5], [1, 1, 0, 0], 1, 1, [2])
    assert (f1[0, 0], bs[0, 0], btp[0, 0], bd[0, 0]) == (2 / 3, 0.9, 1, 1)
    *_, f1, bs, btp, bd = accumulate([], [], [], 1, 1, [2])
    assert f1[0, 0] != f1[0, 0] and bs[0, 0] != bs[0, 0] and (btp[0, 0], bd[0, 0]) == (0, 0)


# ----------------------------------------------------------------------------------------------- arguments and scores
def test_argument_checks():
    c = cell(ob("a", 0, 0, 1, 1))
    for bad in ([], [0.5] * 33, [0.0], [1.5], ["0.5"], [True], [NAN]):
        with pytest.raises(ValueError, match="iou_thresholds"):
            P.evaluate_boxes_cells([c], [c], scores=[[1]], iou_thresholds=bad, backend=BE)
    for bad in (0, -1, 1.0, True, "3"):
        with pytest.raises(ValueError, match="max_dets"):
            P.evaluate_boxes_cells([c], [c], scores=[[1]], max_dets=bad, backend=BE)
    with pytest.raises(ValueError, match="exactly one"):
        P.evaluate_boxes_cells([c], [c], backend=BE)
    with pytest.raises(ValueError, match="exactly one"):
        P.evaluate_boxes_cells([c], [c], scores=[[1]], score_key="s", backend=BE)
    with pytest.raises(ValueError, match="one cell per image"):
        P.evaluate_boxes_cells([c], [c, c], scores=[[1], [1]], backend=BE)
    with pytest.raises(TypeError, match="eval_match_boxes"):
        P.evaluate_boxes_cells([c], [c], scores=[[1]], backend=OracleBackend())
    assert P.evaluate_boxes_cells([c], [c], scores=[[1]], iou_thresholds=1.0, max_dets=np.int64(2), backend=BE).totals["max_dets"] == 2


def test_scores_by_object_position():
    """the score of a box is scores[row][its object], whatever objects without a box sit in between"""
    pred = [cell({"name": "note"}, ob("a", 0, 0, 10, 10), ob("a", 20, 20, 30, 30)), cell(), cell(ob("a", 0, 0, 5, 5))]
    gt = [cell(ob("a", 0, 0, 10, 10)), cell(ob("a", 1, 1, 2, 2)), cell()]
    res = evaluate(gt, pred, scores=[[0.1, 0.7, 0.2], None, (True,)])
    assert res.detections[["row", "object", "score", "state"]].values.tolist()[:2] == [[0, 1, 0.7, "evaluated"], [0, 2, 0.2, "evaluated"]]
    assert res.detections["state"].tolist()[2] == "bad_score"                  # a bool is no number
    with pytest.raises(ValueError, match="row 0"):
        P.evaluate_boxes_cells(gt, pred, scores=[[0.1, 0.7], None, [1]], backend=BE)
    with pytest.raises(ValueError, match="row 2"):
        P.evaluate_boxes_cells(gt, pred, scores=[[0.1, 0.7, 0.2], None, None], backend=BE)
    with pytest.raises(ValueError, match="one entry per row"):
        P.evaluate_boxes_cells(gt, pred, scores=[[0.1, 0.7, 0.2]], backend=BE)


def test_score_key_reads_the_objects():
    pred = [cell(ob("a", 0, 0, 10, 10, conf=0.8), ob("a", 0, 0, 9, 10), ob("b", 0, 0, 10, 10, conf="0.9")), cell()]
    gt = [cell(ob("a", 0, 0, 10, 10), ob("b", 0, 0, 10, 10)), cell(ob("b", 0, 0, 1, 1))]
    stats = {}
    res = evaluate(gt, pred, score_key="conf", stats=stats)
    assert res.detections["state"].tolist() == ["evaluated", "bad_score", "bad_score"]      # a missing key, a string
    assert stats["python_score_cells"] == 1 and stats["bad_score"] == 2 and stats["gt_boxes"] == 3


def test_chunks_feed_one_accumulation(monkeypatch):
    rng = np.random.default_rng(5)
    gt, pred, scores = [], [], []
    for r in range(23):
        g = [ob("abc"[rng.integers(0, 3)], *(rng.integers(0, 20, 2).tolist()), *(rng.integers(20, 40, 2).tolist())) for _ in range(rng.integers(0, 4))]
        d = [dict(o) for o in g if rng.random() < 0.8] + [ob("a", 1, 1, 30, 30)]
        gt.append(cell(*g)), pred.append(cell(*d)), scores.append(np.round(rng.random(len(d)), 1).tolist())
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 5)
    res = evaluate(gt, pred, scores=scores, sources=[f"s{r}" for r in range(23)])
    assert res.totals["rows"] == 23 and list(res.per_row.columns[:2]) == ["row", "source"]


# ----------------------------------------------------------------------------------------------- frames, keys, CSV
def frames():
    gt = [cell(ob("a", 0, 0, 10, 10)), cell(ob("b", 0, 0, 10, 10), ob("a", 50, 50, 60, 60)), cell(ob("c", 1, 1, 5, 5))]
    pred = [cell(ob("a", 50, 50, 60, 60), ob("b", 0, 0, 10, 9)), cell(ob("a", 0, 0, 10, 10)), cell(ob("x", 1, 1, 2, 2))]
    df_gt = pd.DataFrame({"source": ["u0", "u1", "u2"], COL: gt})
    df_pred = pd.DataFrame({"source": ["u1", "u0", "u9"], COL: pred, "conf": ["[0.9, 0.6]", "[0.8]", "[0.7]"]})
    return df_gt, df_pred


def test_frame_rows_of_one_side_only():
    """u2 has no predictions: it is evaluated without detections and its box is missed; u9 has no ground truth: unpaired"""
    df_gt, df_pred = frames()
    stats = {}
    res = P.evaluate_boxes_frame(df_gt, df_pred, score_col="conf", backend=BE, stats=stats)
    want = expected_evaluation(df_gt[COL].tolist(), [df_pred[COL].iat[1], df_pred[COL].iat[0], "{}"],
                               scores=[[0.8], [0.9, 0.6], None], sources=["u0", "u1", "u2"])
    check_evaluation(res, want)
    assert res.per_row[["row", "gt_boxes", "detections", "tp", "fn"]].values.tolist() == [[0, 1, 1, 1, 0], [1, 2, 2, 2, 0], [2, 1, 0, 0, 1]]
    assert res.unpaired["key"].tolist() == ["u9"] and stats["rows_only_pred"] == 1 and stats["rows_only_gt"] == 1
    assert res.missed[["row", "source", "name"]].values.tolist() == [[2, "u2", "c"]]


def test_frame_by_position_one_frame_and_errors():
    df_gt, df_pred = frames()
    res = P.evaluate_boxes_frame(df_gt, df_pred, key=None, score_col="conf", backend=BE)
    check_evaluation(res, expected_evaluation(df_gt[COL].tolist(), df_pred[COL].tolist(), scores=[[0.9, 0.6], [0.8], [0.7]],
                                              sources=["u0", "u1", "u2"]))
    both = df_gt.assign(pred=df_pred[COL].to_numpy(), conf=[[0.9, 0.6], (0.8,), np.asarray([0.7])])
    res2 = P.evaluate_boxes_frame(both, other_col="pred", score_col="conf", iou_thresholds=[0.3], backend=BE)
    assert res2.detections["score"].tolist() == [0.9, 0.6, 0.8, 0.7] and res2.iou_thresholds.tolist() == [0.3]
    with pytest.raises(ValueError, match="exactly one"):
        P.evaluate_boxes_frame(df_gt, df_pred, backend=BE)
    with pytest.raises(ValueError, match="row 1"):                             # u1's cell holds two boxes
        P.evaluate_boxes_frame(df_gt, df_pred.assign(conf=["[0.9]", "[0.8]", "oops"]), score_col="conf", backend=BE)


def test_csv_entry_writes_and_reloads(tmp_path, capsys):
    df_gt, df_pred = frames()
    df_gt.to_csv(tmp_path / "gt.csv", index=False, encoding="utf-8-sig")
    df_pred.to_csv(tmp_path / "pred.csv", index=False, encoding="utf-8-sig")
    out = P.evaluate_boxes_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "out", score_col="conf", backend=BE,
                               detections_csv=tmp_path / "out" / "dets.csv")
    res = P.evaluate_boxes_frame(df_gt, df_pred, score_col="conf", backend=BE)
    assert all(out[k] == v or (v != v and out[k] != out[k]) for k, v in res.totals.items())
    assert sorted(out["paths"]) == ["classes", "curves", "detections", "missed", "rows"]
    z = np.load(out["paths"]["curves"])
    assert z["classes"].tolist() == res.classes and np.array_equal(z["recall_points"], REC)
    same_arrays([z[k] for k in ("iou_thresholds", "precision", "score_at", "recall", "ap")],
                [res.iou_thresholds, res.precision, res.score_at, res.recall, res.ap], ["thr", "precision", "score_at", "recall", "ap"])
    assert pd.read_csv(out["paths"]["rows"], encoding="utf-8-sig")["fn"].tolist() == res.per_row["fn"].tolist()
    assert len(pd.read_csv(out["paths"]["detections"], encoding="utf-8-sig")) == len(res.detections)
    out2 = P.evaluate_boxes_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "out2", score_key="conf", backend=BE)
    assert "detections" not in out2["paths"] and out2["bad_score"] == 3        # no object has the key; u9 is not evaluated
    assert P.evaluate_boxes_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "o", score_col="nope", backend=BE) is None
    assert P.evaluate_boxes_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "o", key="nope", score_key="c", backend=BE) is None
    assert P.evaluate_boxes_csv(tmp_path / "none.csv", tmp_path / "pred.csv", tmp_path / "o", score_key="c", backend=BE) is None
    assert "缺少必要列 nope" in capsys.readouterr().out


def test_match_and_accumulate_names():
    assert len(MATCH_NAMES) == 7 and len(ACC_NAMES) == 8
