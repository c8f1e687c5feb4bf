"""Scored polygon evaluation (core/processor.py: evaluate_polygons_*), host side: the restatement of K25
(tests/polygon_eval_ref.py) pinned on hand-worked cases whose values are derived in the docstrings, then the step functions
(chunks and batches, scores, alignment, CSV, arguments), driven by a test backend whose device stage is that restatement, and the
box evaluation, which shares its result path, checked to return what it returned before.  No GPU.

pycocotools is not installed here, so nothing in this file (or anywhere else) checks equality with it."""
import json
import math

import numpy as np
import pandas as pd
import pytest

import box_eval_ref as BR
from box_eval_ref import REC, accumulate, check_evaluation, same_arrays
from helpers import OracleBackend
from polygon_compare_tables import box, random_rows, table
from polygon_eval_ref import NAMES, expected_polygon_evaluation, match_polygon_rows

from deal_yolo_daya_amd.core import processor as P

COL = P.ANNOTATION_COL
NAN = float("nan")
(STATUS, PAIR_OFF, G_ACT, D_ACT, G_PIX, D_PIX, STATE, TP, GT, IOU, BEST, HIT, G_BEST) = range(13)
L_SHAPE = [(0.0, 0.0), (4.0, 0.0), (4.0, 2.0), (2.0, 2.0), (2.0, 4.0), (0.0, 4.0)]


class PolyEvalBackend(OracleBackend):
    def __init__(self):
        self.calls = []

    def eval_match_polygons(self, *args):
        out = match_polygon_rows(*args)
        self.calls.append((len(args[9]), int(out[PAIR_OFF][-1])))
        return out

    def eval_accumulate(self, cls, score, tp, n_classes, n_thresholds, npig, rec):
        return accumulate(cls, score, tp, n_classes, n_thresholds, npig, rec)

    def eval_match_boxes(self, *args):
        return BR.match_rows(*args)


BE = PolyEvalBackend()


def one_row(gt, dt, score, thr=(0.5,), w=8, h=8, C=2, **kw):
    """match_polygon_rows on one row; gt / dt = [(cls, points)]"""
    return match_polygon_rows(*table([(w, h, gt, dt)])[:8], score, [w], [h], C, thr, **kw)


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def evaluate(cells_gt, cells_pred, widths, heights, **kw):
    res = P.evaluate_polygons_cells(cells_gt, cells_pred, widths, heights, backend=BE, **kw)
    ref_kw = {k: v for k, v in kw.items() if k not in ("stats", "batch_pixels", "batch_pairs")}
    check_evaluation(res, expected_polygon_evaluation(cells_gt, cells_pred, widths, heights, **ref_kw))
    return res


# ----------------------------------------------------------------------------------------------- the rule, by hand
def test_l_shape_against_its_bounding_box():
    """The L covers the pixels of [0,4) x [0,2) and [0,2) x [2,4): 8 + 4 = 12.  The detection is the box (0,0)-(4,4): 16 pixels,
    all 12 of the L among them.  IoU = 12 / (12 + 16 - 12) = 12/16 = 0.75 exactly: a match at 0.5 and at 0.75, none at 0.8.  The
    box evaluation sees the L's min/max box, which is the detection itself: IoU 1.0 at every threshold."""
    out = one_row([(0, L_SHAPE)], [(0, box(0, 0, 4, 4))], [0.9], thr=(0.5, 0.75, 0.8))
    assert out[G_PIX].tolist() == [12] and out[D_PIX].tolist() == [16]
    assert out[TP].tolist() == [0b011] and out[IOU].tolist() == [0.75] and out[BEST].tolist() == [0.75] and out[HIT].tolist() == [0b011]
    gt, pred = [cell(ob("a", L_SHAPE))], [cell(ob("a", box(0, 0, 4, 4)))]
    res = evaluate(gt, pred, [8], [8], scores=[[0.9]], iou_thresholds=[0.5, 0.75, 0.8])
    assert res.detections[["state", "tp_thresholds", "iou", "pixels"]].values.tolist() == [["evaluated", 2, 0.75, 16]]
    assert res.ap[0, 2] == 0.0 and res.ap[0, 0] == res.ap[0, 1] > 0.99
    boxes = P.evaluate_boxes_cells(gt, pred, scores=[[0.9]], iou_thresholds=[0.5, 0.75, 0.8], backend=BE)
    assert boxes.detections[["tp_thresholds", "iou"]].values.tolist() == [[3, 1.0]]          # 0b111: the gap this step closes


def test_iou_exactly_at_the_threshold_matches():
    """GT (0,0)-(4,4) has 16 pixels, the detection (0,0)-(4,2) has 8, all inside: IoU = 8 / (16 + 8 - 8) = 0.5 >= 0.5"""
    out = one_row([(0, box(0, 0, 4, 4))], [(0, box(0, 0, 4, 2))], [0.3], thr=(0.5, np.nextafter(0.5, 1)))
    assert out[TP].tolist() == [0b01] and out[GT].tolist() == [0] and out[IOU].tolist() == [0.5]


def test_two_identical_gt_polygons_the_higher_index_is_taken():
    sq = box(1, 1, 5, 5)
    out = one_row([(0, sq), (0, sq)], [(0, sq)], [0.5])
    assert out[TP].tolist() == [1] and out[GT].tolist() == [1] and out[HIT].tolist() == [0, 1] and out[G_BEST].tolist() == [1.0, 1.0]


def test_a_detection_takes_different_gt_polygons_at_different_thresholds():
    """GT A = (0,0)-(8,8): 64 px, B = (0,0)-(8,5): 40 px.  d1 = (0,0)-(8,4): 32 px (0.9), d2 = (0,0)-(8,7): 56 px (0.8).
    IoU(A,d1) = 32/64 = 0.5, IoU(B,d1) = 32/40 = 0.8, IoU(A,d2) = 56/64 = 0.875, IoU(B,d2) = 40/56 = 0.714...
    At 0.5: d1 takes B (0.8 > 0.5), d2 takes A.  At 0.85: d1 takes nothing, d2 takes A.  At 0.7 d1 takes B, d2 takes A; at 0.6
    the same.  So d2 holds A at every threshold and d1 holds B up to 0.8."""
    out = one_row([(0, box(0, 0, 8, 8)), (0, box(0, 0, 8, 5))], [(0, box(0, 0, 8, 4)), (0, box(0, 0, 8, 7))], [0.9, 0.8],
                  thr=(0.5, 0.85))
    assert out[TP].tolist() == [0b01, 0b11] and out[GT].tolist() == [1, 0] and out[IOU].tolist() == [0.8, 0.875]
    assert out[BEST].tolist() == [0.8, 0.875] and out[HIT].tolist() == [0b11, 0b01] and out[G_BEST].tolist() == [0.875, 0.8]
    # the lower score first: d2 (0.95) takes A at both thresholds; d1 then finds B at 0.5 and nothing at 0.85
    swapped = one_row([(0, box(0, 0, 8, 8)), (0, box(0, 0, 8, 5))], [(0, box(0, 0, 8, 4)), (0, box(0, 0, 8, 7))], [0.9, 0.95],
                      thr=(0.5, 0.85))
    assert swapped[TP].tolist() == [0b01, 0b11]
    # one GT polygon, two detections: at 0.5 the better-scored d1 (IoU 0.5) takes A, at 0.85 it cannot and d2 takes A
    one = one_row([(0, box(0, 0, 8, 8))], [(0, box(0, 0, 8, 4)), (0, box(0, 0, 8, 7))], [0.9, 0.8], thr=(0.5, 0.85))
    assert one[TP].tolist() == [0b01, 0b10] and one[GT].tolist() == [0, -1] and one[HIT].tolist() == [0b11]


def test_max_dets_equal_scores_negative_zero_and_scores_that_are_not_finite():
    sq = box(0, 0, 4, 4)
    out = one_row([(0, sq)], [(0, sq)] * 3, [0.2, 0.9, 0.9], max_dets=1)
    assert out[STATE].tolist() == [1, 0, 1] and out[TP].tolist() == [0, 1, 0]      # of the two 0.9 the earlier position ranks first
    two = one_row([(0, sq)], [(0, sq), (1, sq)], [0.2, 0.9], max_dets=1)
    assert two[STATE].tolist() == [0, 0]                                           # the rank counts within the class
    assert one_row([(0, sq)], [(0, sq)] * 2, [-0.0, 0.0], max_dets=1)[STATE].tolist() == [0, 1]
    out = one_row([(0, sq)], [(0, sq)] * 3, [NAN, math.inf, 0.1])
    assert out[STATE].tolist() == [2, 2, 0] and out[TP].tolist() == [0, 0, 1] and out[BEST].tolist() == [0.0, 0.0, 1.0]
    assert out[D_PIX].tolist() == [16, 16, 16]                                     # painted all the same


def test_a_gt_polygon_without_a_pixel_centre_counts_and_is_missed():
    speck = box(0.6, 0.6, 1.4, 1.4)
    out = one_row([(0, speck)], [(0, speck)], [0.9], thr=(0.05,))
    assert out[G_ACT].tolist() == [0] and out[G_PIX].tolist() == [0] and out[D_PIX].tolist() == [0]
    assert out[STATE].tolist() == [0] and out[TP].tolist() == [0] and out[HIT].tolist() == [0] and out[IOU].tolist() == [0.0]
    res = evaluate([cell(ob("a", speck))], [cell(ob("a", speck))], [8], [8], scores=[[0.9]])
    assert res.per_class[["gt_polygons", "evaluated", "tp", "fp", "fn"]].values.tolist() == [[1, 1, 0, 1, 1]]
    assert res.missed[["object", "pixels"]].values.tolist() == [[0, 0]] and (res.ap == 0.0).all()


def test_bad_coordinates_on_either_side_are_skipped():
    sq, bad = box(0, 0, 4, 4), [(1.0, 1.0), (math.inf, 2.0), (3.0, 3.0)]
    out = one_row([(0, bad), (0, sq)], [(0, sq), (0, bad), (0, [(2.0, 2.0)])], [0.9, 0.8, 0.7])
    assert out[G_ACT].tolist() == [2, 0] and out[D_ACT].tolist() == [0, 2, 3] and out[STATE].tolist() == [0, 3, 3]
    assert out[TP].tolist() == [1, 0, 0] and out[GT].tolist() == [1, -1, -1] and out[HIT].tolist() == [0, 1]
    big = 2.0 ** 43
    gt = [cell(ob("a", [(1.0, 1.0), (big, 2.0), (3.0, 3.0)]), ob("a", sq))]
    pred = [cell(ob("a", sq), ob("a", [(1.0, 1.0), (big, 2.0), (3.0, 3.0)]), ob("a", [(2.0, 2.0)]))]
    res = evaluate(gt, pred, [8], [8], scores=[[0.9, 0.8, 0.7]])
    assert res.per_class[["gt_polygons", "gt_skipped", "dt_skipped", "evaluated", "tp", "fn"]].values.tolist() == [[1, 1, 2, 1, 1, 0]]
    assert res.detections["state"].tolist() == ["evaluated", "skipped", "skipped"] and res.totals["gt_polygons"] == 1
    assert res.totals["skipped"] == 2 and res.totals["gt_skipped"] == 1 and len(res.missed) == 0


def test_the_row_rule():
    """no size, a fractional size, too large (5 x 4 > 16), too many pairs at na * nb = max_pairs_per_row + 1 = 7"""
    sq = [(0, box(0, 0, 2, 2))]
    rows = [(4, 4, sq * 2, sq * 3), (4, 4, sq, sq * 7), (0, 4, sq, sq), (4.5, 4, sq, sq), (5, 4, sq, sq), (4, 4, sq, [])]
    t = table(rows)
    nd = int(t[6][-1])
    out = match_polygon_rows(*t[:8], np.linspace(0.9, 0.1, nd), t[8], t[9], 1, [0.5], max_pixels_per_row=16, max_pairs_per_row=6)
    assert out[STATUS].tolist() == [0, 4, 1, 2, 3, 0] and out[PAIR_OFF].tolist() == [0, 6, 6, 6, 6, 6, 6]
    assert out[G_ACT].tolist() == [0, 0, 5, 5, 5, 5, 0] and out[STATE].tolist() == [0] * 3 + [3] * 10
    assert out[TP].tolist() == [1, 1, 0] + [0] * 10 and out[HIT].tolist() == [1, 1, 0, 0, 0, 0, 0]
    cells = [cell(*[ob("a", pts) for _, pts in r[k]]) for k in (2, 3) for r in rows]
    gt, pred = cells[:6], cells[6:]
    scores = [[0.5] * len(r[3]) for r in rows]
    res = evaluate(gt, pred, [r[0] for r in rows], [r[1] for r in rows], scores=scores, max_pixels_per_row=16, max_pairs_per_row=6)
    assert res.per_row["status"].tolist() == ["evaluated", "too_many_pairs", "no_size", "fractional_size", "too_large", "evaluated"]
    assert res.per_row["pixels"].tolist() == [16, 0, 0, 0, 0, 16] and res.per_row["gt_polygons"].tolist() == [2, 0, 0, 0, 0, 1]
    t_ = res.totals
    assert (t_["rows_evaluated"], t_["rows_no_size"], t_["rows_fractional_size"], t_["rows_too_large"], t_["rows_too_many_pairs"],
            t_["rows_size_mismatch"], t_["pixels"], t_["gt_polygons"], t_["gt_skipped"], t_["skipped"]) == (2, 1, 1, 1, 1, 0, 32, 3, 4, 10)


def test_a_heavy_overlap_with_another_class_only_is_no_match():
    sq = box(0, 0, 4, 4)
    out = one_row([(1, sq)], [(0, sq)], [0.9])
    assert out[TP].tolist() == [0] and out[BEST].tolist() == [0.0] and out[G_BEST].tolist() == [0.0] and out[HIT].tolist() == [0]
    assert one_row([(0, sq)], [(0, sq)], [0.9], thr=(NAN, 0.5))[TP].tolist() == [0b10]          # a NaN threshold matches nothing


def test_random_table_identities():
    """the random table of the GPU test: a detection's best IoU bounds its matched IoU, tp bits are nested in the hits"""
    rows = random_rows(7, n_rows=20, max_polys=6, max_size=40)
    t = table(rows)
    score = np.round(np.random.default_rng(7).random(int(t[6][-1])), 1)
    out = match_polygon_rows(*t[:8], score, t[8], t[9], 3, BR.THR, max_pixels_per_row=40 * 40, max_pairs_per_row=20)
    assert len(out) == len(NAMES) and (out[IOU] <= out[BEST]).all() and (out[STATE][out[D_ACT] != 0] == 3).all()
    assert sum(bin(int(v)).count("1") for v in out[TP]) == sum(bin(int(v)).count("1") for v in out[HIT]) > 20
    assert {0, 3} <= set(out[STATE].tolist()) and (out[TP][out[STATE] != 0] == 0).all()


# ----------------------------------------------------------------------------------------------- the host layer
NAMES3 = ["cat", "dog", "emu"]


def frames(n_rows=24, seed=9):
    rows = random_rows(seed, n_rows=n_rows, max_polys=5, max_size=40)
    rng = np.random.default_rng(seed)
    src = [f"im{k}.jpg" for k in range(n_rows)]
    sizes = {"width": [r[0] for r in rows], "height": [r[1] for r in rows]}
    cells, conf = [[], []], []
    for row in rows:
        for k in (0, 1):
            keep = [(c, pts) for c, pts in row[2 + k] if all(map(math.isfinite, sum(pts, ())))]
            cells[k].append(cell(*[ob(NAMES3[c] if c >= 0 else 7, pts) for c, pts in keep]))
        conf.append(json.dumps(np.round(rng.random(len(json.loads(cells[1][-1])["objects"])), 1).tolist()))
    return (pd.DataFrame({"source": src, COL: cells[0], **sizes}), pd.DataFrame({"source": src, COL: cells[1], "conf": conf, **sizes}))


def want_of(df_gt, df_pred, present=None, mismatch=None, **kw):
    """expected_polygon_evaluation over df_gt's rows, with df_pred's rows by key (those in `present`)"""
    by_key = {s: (c, json.loads(v)) for s, c, v in zip(df_pred["source"], df_pred[COL], df_pred["conf"])}
    pred, scores = [], []
    for s in df_gt["source"]:
        c, v = by_key.get(s, ("{}", None)) if present is None or s in present else ("{}", None)
        pred.append(c), scores.append(v)
    return expected_polygon_evaluation(df_gt[COL].tolist(), pred, df_gt["width"].tolist(), df_gt["height"].tolist(), scores=scores,
                                       sources=df_gt["source"].tolist(), mismatch=mismatch, **kw)


def test_chunks_and_batches_feed_one_accumulation(monkeypatch):
    df_gt, df_pred = frames()
    kw = dict(max_pixels_per_row=40 * 40, max_pairs_per_row=20, iou_thresholds=[0.3, 0.5, 0.75])
    want = want_of(df_gt, df_pred, **kw)
    one = PolyEvalBackend()
    check_evaluation(P.evaluate_polygons_frame(df_gt, df_pred, score_col="conf", backend=one, **kw), want)
    assert len(one.calls) == 1 and want["totals"]["evaluated"] > 20 and want["per_class"]["tp"].sum() > 10
    assert {"evaluated", "no_size", "fractional_size", "too_many_pairs"} <= set(want["per_row"]["status"])
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 5)
    be = PolyEvalBackend()
    check_evaluation(P.evaluate_polygons_frame(df_gt, df_pred, score_col="conf", backend=be, batch_pixels=1500, **kw), want)
    assert len(be.calls) > 6
    be = PolyEvalBackend()
    check_evaluation(P.evaluate_polygons_frame(df_gt, df_pred, score_col="conf", backend=be, batch_pairs=12, **kw), want)
    assert len(be.calls) > 5


def test_scores_and_score_key():
    sq, half = box(0, 0, 4, 4), box(0, 0, 4, 2)
    gt = [cell(ob("a", sq)), cell(ob("a", sq), ob("b", L_SHAPE))]
    pred = [cell({"name": "note"}, ob("a", half, conf=0.8)), cell(ob("b", sq, conf="0.9"), ob("a", sq))]
    res = evaluate(gt, pred, [8, 8], [8, 8], scores=[[0.1, 0.7], (0.5, True)])
    assert res.detections[["row", "object", "score", "state"]].values.tolist()[:2] == [[0, 1, 0.7, "evaluated"], [1, 0, 0.5, "evaluated"]]
    assert res.detections["state"].tolist() == ["evaluated", "evaluated", "bad_score"]      # a bool is no number
    stats = {}
    res = evaluate(gt, pred, [8, 8], [8, 8], score_key="conf", stats=stats)
    assert res.detections["state"].tolist() == ["evaluated", "bad_score", "bad_score"]      # a string, a missing key
    assert stats["python_score_cells"] == 2 and stats == res.totals
    with pytest.raises(ValueError, match="row 0"):
        P.evaluate_polygons_cells(gt, pred, [8, 8], [8, 8], scores=[[0.1], [0.5, 0.5]], backend=BE)


def test_frame_by_key_by_position_and_rows_of_one_side_only():
    df_gt, df_pred = frames()
    kw = dict(max_pairs_per_row=20)
    want = want_of(df_gt, df_pred, **kw)
    check_evaluation(P.evaluate_polygons_frame(df_gt, df_pred, key=None, score_col="conf", backend=BE, **kw), want)
    shuffled = df_pred.iloc[::-1].reset_index(drop=True)
    check_evaluation(P.evaluate_polygons_frame(df_gt, shuffled, score_col="conf", backend=BE, **kw), want)
    both = df_gt.assign(other=df_pred[COL], conf=df_pred["conf"])
    check_evaluation(P.evaluate_polygons_frame(both, other_col="other", score_col="conf", backend=BE, **kw), want)
    # rows on one side only, and a row whose two sizes differ
    part = shuffled.iloc[3:].reset_index(drop=True).copy()
    part = pd.concat([part, part.iloc[:1].assign(source="new.jpg")], ignore_index=True)
    ok = np.flatnonzero(want["per_row"]["status"].to_numpy() == "evaluated")
    hit = df_gt["source"][ok[ok >= 5][0]]
    part.loc[part["source"] == hit, "width"] += 1
    stats = {}
    res = P.evaluate_polygons_frame(df_gt, part, score_col="conf", backend=BE, stats=stats, **kw)
    present = set(part["source"])
    check_evaluation(res, want_of(df_gt, df_pred, present=present, mismatch=(df_gt["source"] == hit).to_numpy(), **kw))
    assert res.unpaired["key"].tolist() == ["new.jpg"] and stats["rows_only_pred"] == 1 and stats["rows_only_gt"] == 3
    assert res.per_row.set_index("source").loc[hit, "status"] == "size_mismatch" and stats["rows_size_mismatch"] == 1
    assert res.per_row["detections"][-3:].tolist() == [0, 0, 0] and stats == res.totals        # the reversed frame lost im21 .. im23
    no_size = P.evaluate_polygons_frame(df_gt, part.drop(columns=["width", "height"]), score_col="conf", backend=BE, **kw)
    assert no_size.totals["rows_size_mismatch"] == 0
    with pytest.raises(ValueError, match="by position"):
        P.evaluate_polygons_frame(df_gt, df_pred.iloc[:3], key=None, score_col="conf", backend=BE)


def test_csv_entry_writes_and_reloads(tmp_path, capsys):
    df_gt, df_pred = frames()
    df_gt.to_csv(tmp_path / "gt.csv", index=False, encoding="utf-8-sig")
    df_pred.iloc[::-1].to_csv(tmp_path / "pred.csv", index=False, encoding="utf-8-sig")
    kw = dict(score_col="conf", backend=BE, max_pairs_per_row=20)
    out = P.evaluate_polygons_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "out", detections_csv=tmp_path / "out" / "d.csv", **kw)
    res = P.evaluate_polygons_frame(df_gt, df_pred, **kw)
    assert all(out[k] == v or (v != v and out[k] != out[k]) for k, v in res.totals.items())
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["d.csv", "polygon_eval_classes.csv", "polygon_eval_curves.npz",
                                                                   "polygon_eval_missed.csv", "polygon_eval_rows.csv"]
    z = np.load(out["paths"]["curves"])
    assert z["classes"].tolist() == [P.COMPARE_NONE if c is None else c for c in res.classes] and np.array_equal(z["recall_points"], REC)
    same_arrays([z[k] for k in ("iou_thresholds", "precision", "score_at", "recall", "ap")],
                [res.iou_thresholds, res.precision, res.score_at, res.recall, res.ap], ["thr", "precision", "score_at", "recall", "ap"])
    rows = pd.read_csv(out["paths"]["rows"], encoding="utf-8-sig")
    assert rows["fn"].tolist() == res.per_row["fn"].tolist() and rows["status"].tolist() == res.per_row["status"].tolist()
    assert pd.read_csv(out["paths"]["classes"], encoding="utf-8-sig")["gt_skipped"].tolist() == res.per_class["gt_skipped"].tolist()
    assert pd.read_csv(out["paths"]["missed"], encoding="utf-8-sig")["pixels"].tolist() == res.missed["pixels"].tolist()
    assert len(pd.read_csv(out["paths"]["detections"], encoding="utf-8-sig")) == len(res.detections) > 20
    capsys.readouterr()
    assert P.evaluate_polygons_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "o", score_col="nope", backend=BE) is None
    assert "缺少必要列 nope" in capsys.readouterr().out
    assert P.evaluate_polygons_csv(tmp_path / "none.csv", tmp_path / "pred.csv", tmp_path / "o", score_key="c", backend=BE) is None
    assert "读取失败" in capsys.readouterr().out
    assert P.evaluate_polygons_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "o", key="nope", score_key="c", backend=BE) is None


def test_arguments():
    c = [cell(ob("a", box(0, 0, 2, 2)))]
    kw = dict(scores=[[1]], backend=BE)
    for bad in ([], [0.5] * 33, [0.0], [1.5], ["0.5"], [True], [NAN]):
        with pytest.raises(ValueError, match="iou_thresholds"):
            P.evaluate_polygons_cells(c, c, [4], [4], iou_thresholds=bad, **kw)
    for bad in (0, -1, 1.0, True, "3"):
        with pytest.raises(ValueError, match="max_dets"):
            P.evaluate_polygons_cells(c, c, [4], [4], max_dets=bad, **kw)
    for bad in (dict(max_pixels_per_row=0), dict(max_pixels_per_row=2 ** 30 + 1), dict(max_pairs_per_row=0),
                dict(max_pairs_per_row=2 ** 24 + 1), dict(max_pairs_per_row=2.0), dict(batch_pixels=0), dict(batch_pairs=0)):
        with pytest.raises(ValueError):
            P.evaluate_polygons_cells(c, c, [4], [4], **bad, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        P.evaluate_polygons_cells(c, c, [4], [4], backend=BE)
    with pytest.raises(ValueError, match="exactly one"):
        P.evaluate_polygons_cells(c, c, [4], [4], score_key="s", **kw)
    with pytest.raises(ValueError, match="one cell per image"):
        P.evaluate_polygons_cells(c, c + c, [4], [4], scores=[[1], [1]], backend=BE)
    with pytest.raises(ValueError, match="widths and heights"):
        P.evaluate_polygons_cells(c, c, [4, 4], [4], **kw)
    with pytest.raises(TypeError, match="eval_match_polygons"):
        P.evaluate_polygons_cells(c, c, [4], [4], scores=[[1]], backend=OracleBackend())

    class Off(PolyEvalBackend):
        def eval_match_polygons(self, *a):
            out = list(super().eval_match_polygons(*a))
            out[0] = np.where(out[0] == 0, 3, out[0]).astype(np.uint8)
            return out

    with pytest.raises(RuntimeError, match="differ from the host"):
        P.evaluate_polygons_cells(c, c, [4], [4], scores=[[1]], backend=Off())
    empty = P.evaluate_polygons_cells([cell()], [cell()], [4], [4], scores=[None], backend=BE)
    assert empty.classes == [] and empty.totals["pixels"] == 16 and len(empty.per_class) == 0 and math.isnan(empty.totals["map"])


# ----------------------------------------------------------------------------------------------- the box evaluation is unchanged
def test_the_box_evaluation_returns_what_it_returned():
    """evaluate_boxes_* shares _eval_fields and the alignment with the polygon step: its results on the cases of
    box_eval_ref.expected_evaluation stay what that restatement says, field by field and column by column"""
    bob = lambda name, x1, y1, x2, y2, **e: ob(name, [(x1, y1), (x2, y2)], **e)   # noqa: E731
    rng = np.random.default_rng(5)
    gt, pred, scores = [], [], []
    for r in range(23):
        g = [bob("abc"[rng.integers(0, 3)], *(rng.integers(0, 20, 2).tolist()), *(rng.integers(20, 40, 2).tolist())) for _ in range(rng.integers(0, 4))]
        d = [dict(o) for o in g if rng.random() < 0.8] + [bob("a", 1, 1, 30, 30)]
        gt.append(cell(*g)), pred.append(cell(*d)), scores.append(np.round(rng.random(len(d)), 1).tolist())
    src = [f"s{r}" for r in range(23)]
    res = P.evaluate_boxes_cells(gt, pred, scores=scores, backend=BE, sources=src)
    check_evaluation(res, BR.expected_evaluation(gt, pred, scores=scores, sources=src))
    assert type(res) is P.BoxEvaluation and list(res.per_class.columns[:3]) == ["class", "gt_boxes", "detections"]
    assert list(res.per_row.columns) == ["row", "source", "gt_boxes", "detections", "tp", "fp", "fn"]
    assert list(res.totals) == ["rows", "gt_boxes", "detections", "evaluated", "cut", "bad_score", "map", "map50", "map75", "mar",
                                "python_cells", "python_score_cells", "max_dets"]
    df_gt = pd.DataFrame({"source": src, P.BBOX_COL: gt})
    order = rng.permutation(23)[:20]
    df_pred = pd.DataFrame({"source": [src[r] for r in order] + ["extra"], P.BBOX_COL: [pred[r] for r in order] + [cell(bob("a", 0, 0, 5, 5))],
                            "conf": [json.dumps(scores[r]) for r in order] + ["[0.5]"]})
    stats = {}
    res = P.evaluate_boxes_frame(df_gt, df_pred, score_col="conf", backend=BE, stats=stats)
    kept = set(order.tolist())
    check_evaluation(res, BR.expected_evaluation(gt, [pred[r] if r in kept else "{}" for r in range(23)],
                                                 scores=[scores[r] if r in kept else None for r in range(23)], sources=src))
    assert res.unpaired["key"].tolist() == ["extra"] and stats["rows_only_gt"] == 3 and stats["rows_only_pred"] == 1
    assert list(stats)[-2:] == ["rows_only_gt", "rows_only_pred"] and stats == res.totals
