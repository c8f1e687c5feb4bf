"""K25 (scored polygon evaluation, csrc/k25_poly_eval.hip) on the MI355X: dyd_eval_match_polygons against the plain-Python
restatement (tests/polygon_eval_ref.py), all thirteen arrays bit for bit, on the smallest tables at which the paint kernel's
evaluation flavour and the match kernel can go wrong; against K24 on boxes and K22 on the same tables; and the step functions
end to end over several chunks and batches.  Every image is at most 96 pixels on a side.  pycocotools is not installed: equality
with it is not checked."""
import functools
import json
import math

import numpy as np
import pandas as pd
import pytest

from box_eval_ref import MATCH_NAMES, REC, THR, check_evaluation, same_arrays
from polygon_compare_tables import RANDOM, blob, box, random_rows, table
from polygon_eval_ref import NAMES, expected_polygon_evaluation, match_polygon_rows
from test_gpu_box_eval import _check_match as k24_check_match

from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu
COL = P.ANNOTATION_COL
T32 = np.linspace(0.05, 1.0, 32)
ERR_INVALID = -1
(STATUS, PAIR_OFF, G_ACT, D_ACT, G_PIX, D_PIX, STATE, TP, GT, IOU, BEST, HIT, G_BEST) = range(13)
LIMITS = dict(max_pixels_per_row=RANDOM["max_pixels_per_row"], max_pairs_per_row=RANDOM["max_pairs_per_row"])


def direct(native, t, score, C, thr, max_dets=100, max_pixels_per_row=1 << 26, max_pairs_per_row=1 << 20, check=True, null=None):
    """dyd_eval_match_polygons with every output prefilled with a sentinel, so that an unwritten element shows -> the thirteen
    outputs (check=False: the return code); null: the index of an argument passed as NULL"""
    gx, gp, gr, gc, dx, dp, dr, dc, W, H = t
    gx, dx = (np.ascontiguousarray(v, np.float64).reshape(-1) for v in (gx, dx))
    gp, gr, gc, dp, dr, dc = (np.ascontiguousarray(v, np.int32) for v in (gp, gr, gc, dp, dr, dc))
    W, H, score, thr = (np.ascontiguousarray(v, np.float64) for v in (W, H, score, thr))
    n, ng, nd = len(W), len(gc), len(dc)
    outs = [np.full(n, 0xA5, np.uint8), np.full(n + 1, -7, np.int64), np.full(ng, 0xA5, np.uint8), np.full(nd, 0xA5, np.uint8),
            np.full(ng, -7, np.int64), np.full(nd, -7, np.int64), np.full(nd, -7, np.int32), np.full(nd, 0xDEADBEEF, np.uint32),
            np.full(nd, -7, np.int32), np.full(nd, -7.0), np.full(nd, -7.0), np.full(ng, 0xDEADBEEF, np.uint32), np.full(ng, -7.0)]
    p = lambda a: native._ptr(a) if a.size else None     # noqa: E731
    args = [p(gx), native._ptr(gp), native._ptr(gr), p(gc), p(dx), native._ptr(dp), native._ptr(dr), p(dc), p(score), native._ptr(W),
            native._ptr(H), n, int(C), native._ptr(thr) if thr.size else None, len(thr), int(max_dets), int(max_pixels_per_row),
            int(max_pairs_per_row), *(p(o) if k > 1 else native._ptr(o) for k, o in enumerate(outs))]
    if null is not None:
        args[null] = None
    rc = native.lib().dyd_eval_match_polygons(*args)
    if not check:
        return rc
    native.check(rc, "dyd_eval_match_polygons")
    return outs


def both(native, t, score, C, thr, want=None, **kw):
    """the direct call and the wrapper against the restatement -> the restatement's outputs"""
    want = match_polygon_rows(*t[:8], score, t[8], t[9], C, thr, **kw) if want is None else want
    same_arrays(direct(native, t, score, C, thr, **kw), want, NAMES, "direct call")
    same_arrays(native.eval_match_polygons(*t[:8], score, t[8], t[9], C, thr, **kw), want, NAMES, "wrapper")
    return want


def option(native, strip=0, crossings=0, chunk=0, grid=0):
    for key, v in ((b"k22_strip", strip), (b"k22_crossings", crossings), (b"k22_chunk", chunk), (b"k22_grid", grid)):
        native.check(native.lib().dyd_set_option(key, v), "opt")


@functools.lru_cache(maxsize=None)
def random_case(C):
    """the comparison's random table drawn over C classes, scores of one decimal (ties), some of them not finite"""
    t = table(random_rows(5, n_rows=40, max_polys=8, max_size=96, n_classes=C))
    rng = np.random.default_rng(50 + C)
    score = np.round(rng.random(len(t[7])), 1)
    score[rng.random(len(score)) < 0.1] = np.nan
    score[rng.random(len(score)) < 0.03] = -0.0
    return t, score


@functools.lru_cache(maxsize=None)
def random_want(C, T):
    t, score = random_case(C)
    thr = {1: [0.5], 10: THR, 32: T32}[T]
    return thr, match_polygon_rows(*t[:8], score, t[8], t[9], C, thr, **LIMITS)


# ----------------------------------------------------------------------------------------------- 1. empty tables
def test_k25_empty_tables(native):
    none = tuple(np.zeros(k, d) for k, d in ((0, np.float64), (1, np.int32), (1, np.int32), (0, np.int32)) * 2) + (np.zeros(0), np.zeros(0))
    assert [len(v) for v in native.eval_match_polygons(*none[:8], [], none[8], none[9], 2, THR)] == [0, 1] + [0] * 11
    assert [len(v) for v in direct(native, none, [], 2, THR)] == [0, 1] + [0] * 11       # n_rows == 0 returns at once
    a = [(0, box(0, 0, 4, 4)), (1, box(2, 2, 6, 6))]
    t = table([(8, 8, a, []), (8, 8, [], a), (8, 8, [], []), (8, 8, a, a)])
    want = both(native, t, [0.9, 0.8, 0.7, 0.6], 2, [0.5])
    assert want[TP].tolist() == [0, 0, 1, 1] and want[HIT].tolist() == [0, 0, 1, 1] and want[PAIR_OFF].tolist() == [0, 0, 0, 0, 4]
    both(native, table([(8, 8, a, []), (8, 8, a, [])]), [], 2, THR)                         # no detection at all
    both(native, table([(8, 8, [], a), (8, 8, [], a)]), [0.1, 0.2, 0.3, 0.4], 2, THR)      # no ground truth at all
    both(native, table([(8, 8, [], []), (0, 8, [], [])]), [], 1, [0.5])                     # rows without polygons


# ----------------------------------------------------------------------------------------------- 2. random table
@pytest.mark.parametrize("C,T", [(1, 1), (3, 10), (40, 32)], ids=["C1_T1", "C3_T10", "C40_T32"])
def test_k25_random_table(native, C, T):
    (t, score), (thr, want) = random_case(C), random_want(C, T)
    assert (want[STATUS] == 0).sum() > 25 and {0, 2, 3} <= set(want[STATE].tolist()) and want[TP].any()
    both(native, t, score, C, thr, want, **LIMITS)
    if C == 3:
        bits = np.asarray([bin(int(v)).count("1") for v in want[TP]])
        assert ((bits > 0) & (bits < T)).sum() > 5, "the matched sets differ between the thresholds"


# ----------------------------------------------------------------------------------------------- 3. option capacities
@pytest.mark.parametrize("opts", [dict(strip=64), dict(strip=17), dict(crossings=3), dict(crossings=1), dict(chunk=1), dict(chunk=2),
                                  dict(chunk=3), dict(grid=3), dict(strip=17, crossings=1, chunk=1, grid=3)],
                         ids=lambda o: "_".join(f"{k}{v}" for k, v in o.items()))
def test_k25_option_capacities(native, opts):
    (t, score), (thr, want) = random_case(3), random_want(3, 10)
    try:
        option(native, **opts)
        same_arrays(direct(native, t, score, 3, thr, **LIMITS), want, NAMES, str(opts))
    finally:
        option(native)


# ----------------------------------------------------------------------------------------------- 4. chunk and wave boundaries
def overlapping(n, w, h, n_classes, seed):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, n_classes)), blob(rng, w / 2 + rng.uniform(-2, 2), h / 2 + rng.uniform(-1, 1), w / 2, 6)) for _ in range(n)]


def pixel_boxes(n, shift=0):
    """n boxes of 2 x 1 pixels on a 32 x 32 image, classes alternating; shift moves them by a pixel (IoU 1/3 with the unshifted)"""
    return [(k % 2, box((2 * k) % 32 + shift, (2 * k) // 32, (2 * k) % 32 + 2 + shift, (2 * k) // 32 + 1)) for k in range(n)]


def test_k25_one_more_detection_than_the_default_chunk(native):
    t = table([(16, 8, overlapping(3, 16, 8, 2, 70), overlapping(33, 16, 8, 2, 71))])
    want = both(native, t, np.round(np.random.default_rng(72).random(33), 1), 2, [0.1, 0.3, 0.5])
    assert want[TP].any() and (want[BEST] > 0).sum() > 20 and want[BEST][32] > 0


@pytest.mark.parametrize("max_dets", [100, 1])
def test_k25_rows_longer_than_a_wave(native, max_dets):
    """70 GT polygons (lanes stride) and 150 detections (the score order goes through the scratch column) in 2 classes; a second
    row with max_dets + 1 detections in one (row, class)"""
    rng = np.random.default_rng(73)
    dets = pixel_boxes(70) + pixel_boxes(70, shift=1) + pixel_boxes(10)
    assert len(dets) == 150
    sq = box(0, 0, 8, 8)
    rows = [(32, 32, pixel_boxes(70), dets), (32, 32, [(1, sq), (0, sq)], [(1, sq)] * (max_dets + 1) + [(0, sq)])]
    t = table(rows)
    score = np.round(rng.random(150 + max_dets + 2), 2)
    score[150:150 + max_dets + 1] = rng.permutation(max_dets + 1) / 1000                  # no ties: exactly one is cut
    want = both(native, t, score, 2, [0.3, 0.5, 1.0], max_dets=max_dets)
    cut = want[STATE] == 1
    assert int(cut[150:].sum()) == 1 and want[TP][:150].astype(bool).sum() >= (70 if max_dets == 100 else 2)
    assert (want[HIT][:70] > 0).all() if max_dets == 100 else (want[HIT][:70] > 0).sum() == 2


# ----------------------------------------------------------------------------------------------- 5. against K24 on boxes
def test_k25_equals_k24_on_integer_boxes(native):
    """two-point boxes with integer corners inside a 24 x 20 image cover exactly their area in pixels, so the mask IoU is the
    box IoU bit for bit and K24 on the same boxes gives the same seven matching outputs; zero-area boxes included"""
    rng = np.random.default_rng(74)
    rows, boxes = [], [[], []]
    for r in range(30):
        sides = [[], []]
        for _ in range(int(rng.integers(0, 7))):
            x, y = sorted(rng.integers(0, 25, 2).tolist()), sorted(rng.integers(0, 21, 2).tolist())
            if rng.random() < 0.1:
                x[1] = x[0]                                                               # a zero-area box
            c = int(rng.integers(0, 2))
            corners = [[x[0], y[0], x[1], y[1]]]
            if rng.random() < 0.8:                                                        # a detection a pixel or two off
                j = rng.integers(-2, 3, 4)
                corners.append([int(np.clip(x[0] + j[0], 0, 24)), int(np.clip(y[0] + j[1], 0, 20)), int(np.clip(x[1] + j[2], 0, 24)),
                                int(np.clip(y[1] + j[3], 0, 20))])
            if rng.random() < 0.3:                                                        # and one anywhere
                corners.append([*rng.integers(0, 25, 2).tolist(), *rng.integers(0, 21, 2).tolist()])
                corners[-1] = [corners[-1][0], corners[-1][2], corners[-1][1], corners[-1][3]]
            for k, b in enumerate(corners):
                sides[min(k, 1)].append((c, box(*b)))
                boxes[min(k, 1)].append(b)
        rows.append((24, 20, *sides))
    t = table(rows)
    score = np.round(rng.random(len(t[7])), 1)
    thr = [0.25, 0.5, 0.75, 1.0]
    got = direct(native, t, score, 2, thr)
    k24 = native.eval_match_boxes(np.asarray(boxes[0], np.float64).reshape(-1, 4), t[2], t[3], np.asarray(boxes[1], np.float64).reshape(-1, 4),
                                  t[6], t[7], score, 2, thr)
    same_arrays(got[STATE:], k24, MATCH_NAMES, "K25 against K24")
    assert k24[1].astype(bool).sum() > 15 and (got[D_PIX] == 0).sum() > 3


def tie_boxes(n, shift=0):
    """n boxes of 2 x 1 pixels as corners, 16 to a scanline, classes in pairs (0 0 1 1 ..): moved right by a pixel a box has IoU
    1/3 with the box at its own place and with the next one, which for an even k is of its class"""
    return [((k // 2) % 2, [2 * (k % 16) + shift, k // 16, 2 * (k % 16) + 2 + shift, k // 16 + 1]) for k in range(n)]


@pytest.mark.parametrize("max_dets", [100, 1])
def test_k25_strided_row_equals_k24_big_row(native, max_dets):
    """One row of 65 GT boxes and 129 detections in 2 classes, the smallest that leaves K24's 64-lane tile on both sides
    (k24_big_rows_kernel), makes K25's lanes stride and sends the score order through the scratch column: the two kernels run one
    rank pass (eval_match.h) and the same arg-max.  Integer two-point boxes inside a 34 x 8 image, so mask IoU and box IoU are
    equal bit for bit; the detections are the GT boxes and 64 of them moved by a pixel (IoU 1/3, for an even k with two GT boxes
    of its class: the highest index wins); scores of one decimal, so equal scores are settled by position."""
    gts, dets = tie_boxes(65), tie_boxes(65) + tie_boxes(64, shift=1)
    t = table([(34, 8, [(c, box(*b)) for c, b in gts], [(c, box(*b)) for c, b in dets])])
    score = np.round(np.random.default_rng(75).random(129), 1)
    thr = [0.25, 0.5, 1.0]
    as_boxes = (np.asarray([b for _, b in gts], np.float64), t[2], t[3], np.asarray([b for _, b in dets], np.float64), t[6], t[7], score, 2)
    want = both(native, t, score, 2, thr, max_dets=max_dets)
    k24_check_match(native, "tie_boxes", as_boxes, thr, max_dets)
    same_arrays(direct(native, t, score, 2, thr, max_dets=max_dets)[STATE:], native.eval_match_boxes(*as_boxes, thr, max_dets),
                MATCH_NAMES, "K25 against K24")
    assert all(((want[TP] >> k) & 1).any() for k in range(3)), "a true positive at every threshold"
    if max_dets == 1:
        assert (want[STATE] == 1).sum() == 127
    else:
        taken = want[GT][65::2]                                                           # the moved copies of the even boxes
        assert (taken == np.arange(1, 65, 2)).any() and (taken == np.arange(0, 64, 2)).any(), "ties to the highest free index"


# ----------------------------------------------------------------------------------------------- 6. against K22
def test_k25_equals_k22_on_rows_polygons_and_pixels(native):
    t, score = random_case(3)
    got = direct(native, t, score, 3, [0.5], **LIMITS)
    k22 = native.compare_polygons(*t, 3, **LIMITS)
    for k in (STATUS, PAIR_OFF, G_ACT, D_ACT, G_PIX, D_PIX):
        assert got[k].dtype == k22[k].dtype and np.array_equal(got[k], k22[k]), NAMES[k]


# ----------------------------------------------------------------------------------------------- 7. status rows
def test_k25_rows_that_are_not_evaluated(native):
    sq = [(0, box(0, 0, 2, 2))]
    rows = [(4, 4, sq * 2, sq * 3), (4, 4, sq, sq * 7), (0, 4, sq, sq), (4.5, 4, sq, sq), (5, 4, sq, sq), (math.nan, 4, sq, sq),
            (4, 4, sq, sq)]
    t = table(rows)
    nd = len(t[7])
    want = both(native, t, np.linspace(0.9, 0.1, nd), 1, [0.5], max_pixels_per_row=16, max_pairs_per_row=6)
    assert want[STATUS].tolist() == [0, 4, 1, 2, 3, 1, 0] and want[PAIR_OFF].tolist() == [0, 6, 6, 6, 6, 6, 6, 7]
    off = (want[STATUS] != 0)
    g_off, d_off = np.repeat(off, np.diff(t[2])), np.repeat(off, np.diff(t[6]))
    assert (want[G_ACT][g_off] == 5).all() and (want[D_ACT][d_off] == 5).all() and (want[STATE][d_off] == 3).all()
    assert not want[TP][d_off].any() and not want[HIT][g_off].any() and (want[GT][d_off] == -1).all()
    assert want[TP][~d_off].tolist() == [1, 1, 0, 1]


# ----------------------------------------------------------------------------------------------- 8. rejected inputs
def test_k25_rejected_inputs(native):
    sq = [(0, box(0, 0, 4, 4))]
    t = table([(8, 8, sq, sq)])
    score = [0.5]
    bad_cls = table([(8, 8, sq, [(2, box(0, 0, 4, 4))])])
    cases = [("T outside", dict(thr=[])), ("T outside", dict(thr=[0.5] * 33)), ("max_dets", dict(max_dets=0)),
             ("n_classes", dict(C=0)), ("n_classes", dict(C=1024)), ("class id", dict(t=bad_cls)), ("null", dict(null=8)),
             ("null", dict(null=19)), ("null", dict(null=30)), ("max_pixels_per_row", dict(max_pixels_per_row=0)),
             ("max_pairs_per_row", dict(max_pairs_per_row=(1 << 24) + 1))]
    for what, kw in cases:
        args = dict(t=t, score=score, C=2, thr=[0.5])
        args.update(kw)
        rc = direct(native, args.pop("t"), args.pop("score"), args.pop("C"), args.pop("thr"), check=False, **args)
        assert rc == ERR_INVALID, (what, rc)
        assert what.split()[0].encode() in native.lib().dyd_last_error(), (what, native.lib().dyd_last_error())
        want = both(native, t, score, 2, [0.5])                                            # a valid call afterwards succeeds
        assert want[TP].tolist() == [1]


# ----------------------------------------------------------------------------------------------- 9. the public step
def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def test_l_shape_through_the_public_step(native):
    """12 of 16 pixels: IoU 0.75 exactly (tests/test_polygon_eval_cpu.py has the arithmetic)"""
    L = [(0.0, 0.0), (4.0, 0.0), (4.0, 2.0), (2.0, 2.0), (2.0, 4.0), (0.0, 4.0)]
    gt, pred = [cell(ob("a", L))], [cell(ob("a", box(0, 0, 4, 4)))]
    res = P.evaluate_polygons_cells(gt, pred, [8], [8], scores=[[0.9]], iou_thresholds=[0.5, 0.75, 0.8])
    assert res.detections[["tp_thresholds", "iou", "pixels"]].values.tolist() == [[2, 0.75, 16]]
    check_evaluation(res, expected_polygon_evaluation(gt, pred, [8], [8], scores=[[0.9]], iou_thresholds=[0.5, 0.75, 0.8]))
    assert P.evaluate_boxes_cells(gt, pred, scores=[[0.9]], iou_thresholds=[0.5, 0.75, 0.8]).detections["tp_thresholds"].tolist() == [3]


def test_step_over_several_chunks_batches_and_csv(native, monkeypatch, tmp_path):
    names = ["cat", "人", "emu"]
    rows = random_rows(9, n_rows=30, max_polys=5, max_size=40)
    rng = np.random.default_rng(75)
    src = [f"im{k}.jpg" for k in range(30)]
    gt, pred, conf = [], [], []
    for row in rows:
        cells = [cell(*[ob(names[c] if c >= 0 else 7, pts) for c, pts in row[k] if all(map(math.isfinite, sum(pts, ())))]) for k in (2, 3)]
        gt.append(cells[0]), pred.append(cells[1])
        conf.append(np.round(rng.random(len(json.loads(cells[1])["objects"])), 1).tolist())
    sizes = {"width": [r[0] for r in rows], "height": [r[1] for r in rows]}
    df_gt = pd.DataFrame({"source": src, COL: gt, **sizes})
    order = rng.permutation(30)[:26]
    df_pred = pd.DataFrame({"source": [src[r] for r in order] + ["extra"], COL: [pred[r] for r in order] + [cell(ob("cat", box(0, 0, 5, 5)))],
                            "conf": [json.dumps(conf[r]) for r in order] + ["[0.5]"],
                            "width": [sizes["width"][r] for r in order] + [9], "height": [sizes["height"][r] for r in order] + [9]})
    kept = set(order.tolist())
    kw = dict(max_pairs_per_row=20, iou_thresholds=[0.3, 0.5, 0.75])
    want = expected_polygon_evaluation(gt, [pred[r] if r in kept else "{}" for r in range(30)], sizes["width"], sizes["height"],
                                       scores=[conf[r] if r in kept else None for r in range(30)], sources=src, **kw)
    assert want["totals"]["evaluated"] > 20 and want["per_class"]["tp"].sum() > 10
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 7)
    res = P.evaluate_polygons_frame(df_gt, df_pred, score_col="conf", batch_pixels=2500, **kw)
    check_evaluation(res, want)
    assert res.unpaired["key"].tolist() == ["extra"] and res.totals["rows_only_gt"] == 4
    df_gt.to_csv(tmp_path / "gt.csv", index=False, encoding="utf-8-sig")
    df_pred.to_csv(tmp_path / "pred.csv", index=False, encoding="utf-8-sig")
    out = P.evaluate_polygons_csv(tmp_path / "gt.csv", tmp_path / "pred.csv", tmp_path / "out", score_col="conf", batch_pairs=30, **kw)
    assert sorted(out["paths"]) == ["classes", "curves", "missed", "rows"] and out["evaluated"] == res.totals["evaluated"]
    z = np.load(out["paths"]["curves"])
    assert z["classes"].tolist() == [P.COMPARE_NONE if c is None else c for c in res.classes] and np.array_equal(z["recall_points"], REC)
    same_arrays([z[k] for k in ("iou_thresholds", "precision", "score_at", "recall", "ap")],
                [res.iou_thresholds, res.precision, res.score_at, res.recall, res.ap], ["thr", "precision", "score_at", "recall", "ap"])
    assert pd.read_csv(out["paths"]["classes"], encoding="utf-8-sig")["tp"].tolist() == res.per_class["tp"].tolist()
