"""Restatement of the scored box evaluation (K24, core/processor.py: evaluate_boxes_*) for the tests, in plain Python: loops
over rows, classes, thresholds, detections and GT boxes, as the rule in include/dyd.h reads.

- ``match_rows``: the seven outputs of dyd_eval_match_boxes.
- ``accumulate``: the eight outputs of dyd_eval_accumulate.
- ``expected_evaluation``: cells -> what evaluate_boxes_cells returns, through CPython's json.
- ``same_arrays``: bit equality of f64 arrays (NaN patterns by their isnan masks).

pycocotools is not installed where these tests run: equality with it is not checked anywhere.
"""
import json
import math

import numpy as np
import pandas as pd

from box_compare_ref import _cell_boxes, records

EPS = 2.0 ** -52
REC = np.linspace(0, 1, 101)
THR = np.linspace(0.5, 0.95, 10)
STATES = ("evaluated", "cut", "bad_score")


def _iou(box1, box2):
    """tests/box_compare_ref.py: _iou_py float by float (reference core/processor.py:328-339), box1 the GT box"""
    x1_inter = max(box1[0], box2[0])
    y1_inter = max(box1[1], box2[1])
    x2_inter = min(box1[2], box2[2])
    y2_inter = min(box1[3], box2[3])
    intersection = max(0, x2_inter - x1_inter) * max(0, y2_inter - y1_inter)
    if intersection == 0:
        return 0.0
    area1 = (box1[2] - box1[0]) * (box1[3] - box1[1])
    area2 = (box2[2] - box2[0]) * (box2[3] - box2[1])
    union = area1 + area2 - intersection
    return intersection / union if union != 0 else 0.0


def _normalise(b):
    return (min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3]))


def _boxes(box4):
    return [_normalise([float(v) for v in b]) for b in np.asarray(box4, np.float64).reshape(-1, 4).tolist()]


def match_rows(gt_box4, gt_off, gt_cls, dt_box4, dt_off, dt_cls, dt_score, n_classes, iou_thr, max_dets):
    """-> (dt_state i32, dt_tp u32, dt_gt i32, dt_iou f64, dt_best f64, gt_hit u32, gt_best f64)"""
    G, D = _boxes(gt_box4), _boxes(dt_box4)
    gt_off, dt_off = [int(v) for v in gt_off], [int(v) for v in dt_off]
    gt_cls, dt_cls = [int(v) for v in gt_cls], [int(v) for v in dt_cls]
    score = [float(v) + 0.0 for v in np.asarray(dt_score, np.float64).reshape(-1).tolist()]     # -0.0 -> 0.0
    lims = [min(float(t), 1 - 1e-10) for t in np.asarray(iou_thr, np.float64).reshape(-1).tolist()]
    state, tp, gt = [0] * len(D), [0] * len(D), [-1] * len(D)
    d_iou, d_best = [0.0] * len(D), [0.0] * len(D)
    hit, g_best = [0] * len(G), [0.0] * len(G)
    for r in range(len(gt_off) - 1):
        g0, g1, d0, d1 = gt_off[r], gt_off[r + 1], dt_off[r], dt_off[r + 1]
        order = []
        for c in range(int(n_classes)):
            ranked = []
            for j in range(d0, d1):
                if dt_cls[j] != c:
                    continue
                if not math.isfinite(score[j]):
                    state[j] = 2
                    continue
                ranked.append(j)
            ranked.sort(key=lambda j: -score[j])            # stable: ties to the earlier position
            for rank, j in enumerate(ranked):
                if rank >= max_dets:
                    state[j] = 1
                else:
                    order.append(j)                         # class after class: one of the allowed interleavings
        ious = {}                                           # each pair's IoU is computed once and looked up per threshold
        for j in order:
            for g in range(g0, g1):
                if gt_cls[g] != dt_cls[j]:
                    continue
                iou = ious[g, j] = _iou(G[g], D[j])
                if iou > d_best[j]:
                    d_best[j] = iou
                if iou > g_best[g]:
                    g_best[g] = iou
        for t, lim in enumerate(lims):
            taken = set()
            for j in order:
                best, m = lim, -1
                for g in range(g0, g1):
                    if gt_cls[g] != dt_cls[j] or g in taken:
                        continue
                    iou = ious[g, j]
                    if not iou >= best:                     # COCOeval: `if ious < iou: continue`, then replace
                        continue
                    best, m = iou, g
                if m < 0:
                    continue
                taken.add(m)
                tp[j] |= 1 << t
                hit[m] |= 1 << t
                if t == 0:
                    gt[j], d_iou[j] = m - g0, best
    return (np.asarray(state, np.int32), np.asarray(tp, np.uint32), np.asarray(gt, np.int32), np.asarray(d_iou, np.float64),
            np.asarray(d_best, np.float64), np.asarray(hit, np.uint32), np.asarray(g_best, np.float64))


def accumulate(cls, score, tp, n_classes, T, npig, rec=REC):
    """-> (precision [C,T,R], score_at [C,T,R], recall [C,T], ap [C,T], best_f1, best_score [C,T] f64, best_tp, best_dets i64)"""
    cls = [int(v) for v in cls]
    score = [float(v) + 0.0 for v in np.asarray(score, np.float64).reshape(-1).tolist()]
    tp = [int(v) for v in tp]
    rec = [float(v) for v in rec]
    C, R, nan = int(n_classes), len(rec), float("nan")
    precision, score_at = np.zeros((C, T, R)), np.zeros((C, T, R))
    recall, ap, f1, bs = np.zeros((C, T)), np.zeros((C, T)), np.full((C, T), nan), np.full((C, T), nan)
    btp, bd = np.zeros((C, T), np.int64), np.zeros((C, T), np.int64)
    for c in range(C):
        dets = sorted((i for i in range(len(cls)) if cls[i] == c), key=lambda i: -score[i])     # stable: table order
        n = int(npig[c])
        for t in range(T):
            if n == 0:
                precision[c, t], score_at[c, t], recall[c, t], ap[c, t] = nan, nan, nan, nan
                continue
            tps, rc, pr = 0, [], []
            for k, i in enumerate(dets):
                tps += (tp[i] >> t) & 1
                fps = (k + 1) - tps
                rc.append(tps / n)
                pr.append(tps / ((tps + fps) + EPS))
            for k in range(len(pr) - 1, 0, -1):
                if pr[k] > pr[k - 1]:
                    pr[k - 1] = pr[k]
            for r in range(R):
                for k in range(len(rc)):
                    if rc[k] >= rec[r]:
                        precision[c, t, r], score_at[c, t, r] = pr[k], score[dets[k]]
                        break
            recall[c, t] = rc[-1] if rc else 0.0
            total = 0.0
            for r in range(R):
                total += float(precision[c, t, r])
            ap[c, t] = total / R
            tps, best = 0, None
            for k, i in enumerate(dets):
                tps += (tp[i] >> t) & 1
                if k + 1 < len(dets) and score[dets[k + 1]] == score[i]:
                    continue                                # inside a run of equal scores: no cut "score >= s" ends here
                v = 2 * tps / ((k + 1) + n)
                if best is None or v > best[0]:
                    best = (v, score[i], tps, k + 1)
            if best is not None:
                f1[c, t], bs[c, t], btp[c, t], bd[c, t] = best
    return precision, score_at, recall, ap, f1, bs, btp, bd


def same_arrays(got, want, names, what=""):
    """equal shapes and contents: f64 arrays bit for bit (every NaN equal to every NaN), the others by value"""
    for nm, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what} {nm}: {g.shape} against {w.shape}"
        if g.dtype == np.float64:
            assert w.dtype == np.float64, f"{what} {nm}: dtype"
            gn, wn = np.isnan(g), np.isnan(w)
            assert np.array_equal(gn, wn), f"{what} {nm}: NaN pattern differs"
            g, w = np.where(gn, 0.0, g).view(np.uint64), np.where(wn, 0.0, w).view(np.uint64)
        else:
            g, w = g.astype(np.int64), w.astype(np.int64)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert len(bad) == 0, f"{what} {nm}: {len(bad)} differ, first at {bad[0]}: {g.reshape(-1)[bad[0]]} != {w.reshape(-1)[bad[0]]}"


MATCH_NAMES = ("dt_state", "dt_tp", "dt_gt", "dt_iou", "dt_best", "gt_hit", "gt_best")
ACC_NAMES = ("precision", "score_at", "recall", "ap", "best_f1", "best_score", "best_tp", "best_dets")


# ------------------------------------------------------------------------------------------------ cells -> BoxEvaluation
def _score_of(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return float("nan")
    try:
        return float(v)
    except OverflowError:
        return float("nan")


def _nanmean(values):
    vals = [float(v) for v in values if v == v]
    return sum(vals) / len(vals) if vals else float("nan")


def expected_evaluation(cells_gt, cells_pred, scores=None, score_key=None, iou_thresholds=None, max_dets=100, sources=None):
    """-> dict(classes, per_class, precision, score_at, recall, ap, per_row, detections, missed, totals)"""
    thr = np.asarray(THR if iou_thresholds is None else iou_thresholds, np.float64)
    T, n = len(thr), len(cells_gt)
    rows_g, rows_d = [_cell_boxes(c) for c in cells_gt], [_cell_boxes(c) for c in cells_pred]
    names = {b[1] for row in rows_g + rows_d for b in row if isinstance(b[1], str)}
    odd = any(not isinstance(b[1], str) for row in rows_g + rows_d for b in row)
    classes = sorted(names) + ([None] if odd else [])
    cid = {c: k for k, c in enumerate(classes)}
    C = len(classes)
    sc = []
    for r, row in enumerate(rows_d):
        objs = json.loads(cells_pred[r]).get("objects", []) if (score_key is not None and row) else None
        for b in row:
            if score_key is not None:
                o = objs[b[0]]
                sc.append(_score_of(o.get(score_key)) if isinstance(o, dict) else float("nan"))
            else:
                sc.append(_score_of(scores[r][b[0]]))

    def table(rows):
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        flat = [b for r in rows for b in r]
        return (np.asarray([b[2:] for b in flat], np.float64).reshape(-1, 4), off,
                np.asarray([cid[b[1] if isinstance(b[1], str) else None] for b in flat], np.int64), flat)

    box_g, off_g, cls_g, flat_g = table(rows_g)
    box_d, off_d, cls_d, flat_d = table(rows_d)
    sc = np.asarray(sc, np.float64)
    state, tp, gt, d_iou, d_best, hit, g_best = match_rows(box_g, off_g, cls_g, box_d, off_d, cls_d, sc, C, thr, max_dets)
    ev = np.flatnonzero(state == 0)
    npig = np.bincount(cls_g, minlength=C)[:C] if C else np.zeros(0, np.int64)
    precision, score_at, recall, ap, f1, bs, btp, bd = accumulate(cls_d[ev], sc[ev], tp[ev], C, T, npig)
    row_d = np.repeat(np.arange(n), np.diff(off_d))
    row_g = np.repeat(np.arange(n), np.diff(off_g))
    tp0, hit0 = (tp & 1).astype(bool), (hit & 1).astype(bool)

    def at(value):
        k = [i for i, t in enumerate(thr.tolist()) if t == value]
        return k[0] if k else None

    per_class = []
    for c in range(C):
        dc, gc = cls_d == c, cls_g == c
        e = int((dc & (state == 0)).sum())
        t0 = int((dc & tp0).sum())
        k50, k75 = at(0.5), at(0.75)
        per_class.append((classes[c], int(gc.sum()), int(dc.sum()), e, int((dc & (state == 1)).sum()), int((dc & (state == 2)).sum()),
                          _nanmean(ap[c]), ap[c, k50] if k50 is not None else float("nan"),
                          ap[c, k75] if k75 is not None else float("nan"), _nanmean(recall[c]), t0, e - t0, int(gc.sum()) - t0,
                          f1[c, 0], bs[c, 0], btp[c, 0] / bd[c, 0] if bd[c, 0] else float("nan"),
                          btp[c, 0] / int(gc.sum()) if bd[c, 0] else float("nan")))
    per_class = pd.DataFrame(per_class, columns=["class", "gt_boxes", "detections", "evaluated", "cut", "bad_score", "ap", "ap50",
                                                 "ap75", "recall", "tp", "fp", "fn", "best_f1", "best_score", "precision_at_best",
                                                 "recall_at_best"])
    per_class["class"] = per_class["class"].astype(object)
    pr = {"row": np.arange(n, dtype=np.int64)}
    if sources is not None:
        pr["source"] = np.asarray(sources, object)
    tp_r = np.bincount(row_d[tp0], minlength=n)
    pr.update({"gt_boxes": np.diff(off_g), "detections": np.diff(off_d), "tp": tp_r,
               "fp": np.bincount(row_d[state == 0], minlength=n) - tp_r, "fn": np.diff(off_g) - tp_r})
    src = (lambda r: (sources[r],)) if sources is not None else (lambda r: ())
    dets = [(int(row_d[j]), *src(int(row_d[j])), flat_d[j][0], flat_d[j][1], float(sc[j]), STATES[state[j]], bin(int(tp[j])).count("1"),
             flat_g[off_g[row_d[j]] + gt[j]][0] if gt[j] >= 0 else -1, float(d_iou[j]), float(d_best[j])) for j in range(len(flat_d))]
    detections = pd.DataFrame(dets, columns=["row", *(("source",) if sources is not None else ()), "object", "name", "score",
                                             "state", "tp_thresholds", "gt_object", "iou", "best_iou"])
    miss = [(int(row_g[g]), *src(int(row_g[g])), flat_g[g][0], flat_g[g][1], float(g_best[g]), *box_g[g].tolist())
            for g in range(len(flat_g)) if not hit0[g]]
    missed = pd.DataFrame(miss, columns=["row", *(("source",) if sources is not None else ()), "object", "name", "best_iou",
                                         "x1", "y1", "x2", "y2"])
    has = npig > 0
    k50, k75 = at(0.5), at(0.75)
    totals = {"rows": n, "gt_boxes": len(flat_g), "detections": len(flat_d), "evaluated": int((state == 0).sum()),
              "cut": int((state == 1).sum()), "bad_score": int((state == 2).sum()),
              "map": _nanmean(per_class["ap"][has]), "map50": _nanmean(ap[has, k50]) if k50 is not None else float("nan"),
              "map75": _nanmean(ap[has, k75]) if k75 is not None else float("nan"), "mar": _nanmean(per_class["recall"][has]),
              "max_dets": int(max_dets)}
    return {"classes": classes, "iou_thresholds": thr, "per_class": per_class, "precision": precision, "score_at": score_at,
            "recall": recall, "ap": ap, "per_row": pd.DataFrame(pr), "detections": detections, "missed": missed, "totals": totals}


def check_evaluation(got, want):
    """assert that a BoxEvaluation equals expected_evaluation's answer (the python_* counts and the unpaired rows aside)"""
    assert got.classes == want["classes"]
    same_arrays([got.iou_thresholds], [want["iou_thresholds"]], ["iou_thresholds"])
    for nm in ("per_class", "per_row", "detections", "missed"):
        g, w = getattr(got, nm), want[nm]
        assert list(g.columns) == list(w.columns), nm
        assert records(g) == records(w), nm
    names = ("precision", "score_at", "recall", "ap")
    same_arrays([getattr(got, nm) for nm in names], [want[nm] for nm in names], names)
    for k, v in want["totals"].items():
        gv = got.totals[k]
        assert gv == v or (isinstance(v, float) and v != v and gv != gv), (k, gv, v)
