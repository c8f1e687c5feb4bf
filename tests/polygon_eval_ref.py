"""Restatement of the scored polygon evaluation (K25, core/processor.py: evaluate_polygons_*) for the tests, in plain Python on
top of polygon_raster_ref.cover / row_size and polygon_compare_ref._actions, as the rule in include/dyd.h (K25) reads: whole
images per polygon, loops over rows, thresholds, detections and GT polygons.

- ``match_polygon_rows``: the thirteen outputs of dyd_eval_match_polygons.
- ``expected_polygon_evaluation``: cells -> what evaluate_polygons_cells returns, through CPython's json and
  box_eval_ref.accumulate.

pycocotools is not installed where these tests run: equality with it is not checked anywhere.
"""
import json
import math

import numpy as np
import pandas as pd

from box_eval_ref import STATES as BOX_STATES
from box_eval_ref import THR, _nanmean, _score_of, accumulate
from polygon_compare_ref import STATUS_PAIRS, _actions
from polygon_raster_ref import cover, row_size

STATES = (*BOX_STATES, "skipped")
STATUS = ("evaluated", "no_size", "fractional_size", "too_large", "too_many_pairs")
NAMES = ("row_status", "pair_off", "gt_action", "dt_action", "gt_pixels", "dt_pixels", "dt_state", "dt_tp", "dt_gt", "dt_iou",
         "dt_best", "gt_hit", "gt_best")


def match_polygon_rows(gt_xy, gt_pt_off, gt_row_off, gt_cls, dt_xy, dt_pt_off, dt_row_off, dt_cls, dt_score, width, height,
                       n_classes, iou_thr, max_dets=100, max_pixels_per_row=1 << 26, max_pairs_per_row=1 << 20):
    """-> the thirteen arrays of NAMES, in that order"""
    gt_xy, dt_xy = (np.asarray(v, np.float64).reshape(-1, 2) for v in (gt_xy, dt_xy))
    gt_pt_off, gt_row_off, gt_cls, dt_pt_off, dt_row_off, dt_cls = (np.asarray(v, np.int64) for v in
                                                                   (gt_pt_off, gt_row_off, gt_cls, dt_pt_off, dt_row_off, dt_cls))
    W, H = np.asarray(width, np.float64), np.asarray(height, np.float64)
    score = [float(v) + 0.0 for v in np.asarray(dt_score, np.float64).reshape(-1).tolist()]     # -0.0 -> 0.0
    lims = [min(float(t), 1 - 1e-10) for t in np.asarray(iou_thr, np.float64).reshape(-1).tolist()]
    n, NG, ND = len(W), len(gt_cls), len(dt_cls)
    status, pair_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    g_act, d_act = np.full(NG, 255, np.uint8), np.full(ND, 255, np.uint8)
    g_pix, d_pix = np.zeros(NG, np.int64), np.zeros(ND, np.int64)
    state, tp, gt = [3] * ND, [0] * ND, [-1] * ND
    d_iou, d_best = [0.0] * ND, [0.0] * ND
    hit, g_best = [0] * NG, [0.0] * NG
    for r in range(n):
        g0, g1, d0, d1 = int(gt_row_off[r]), int(gt_row_off[r + 1]), int(dt_row_off[r]), int(dt_row_off[r + 1])
        ng, nd = g1 - g0, d1 - d0
        status[r], w, h = row_size(W[r], H[r], max_pixels_per_row)
        if status[r] == 0 and ng * nd > max_pairs_per_row:
            status[r] = STATUS_PAIRS
        ok = status[r] == 0
        pair_off[r + 1] = pair_off[r] + (ng * nd if ok else 0)
        g_act[g0:g1] = _actions(gt_xy, gt_pt_off, g0, g1, gt_cls, ok)
        d_act[d0:d1] = _actions(dt_xy, dt_pt_off, d0, d1, dt_cls, ok)
        if not ok:
            continue
        cov_g = {g: cover(gt_xy[gt_pt_off[g]:gt_pt_off[g + 1]], w, h) for g in range(g0, g1) if g_act[g] == 0}
        cov_d = {j: cover(dt_xy[dt_pt_off[j]:dt_pt_off[j + 1]], w, h) for j in range(d0, d1) if d_act[j] == 0}
        for g, c in cov_g.items():
            g_pix[g] = int(c.sum())
        for j, c in cov_d.items():
            d_pix[j] = int(c.sum())
        order = []
        for c in range(int(n_classes)):
            ranked = []
            for j in range(d0, d1):
                if dt_cls[j] != c or d_act[j] != 0:
                    continue
                if not math.isfinite(score[j]):
                    state[j] = 2
                    continue
                ranked.append(j)
            ranked.sort(key=lambda j: -score[j])            # stable: ties to the earlier position
            for rank, j in enumerate(ranked):
                state[j] = 1 if rank >= max_dets else 0
                if rank < max_dets:
                    order.append(j)                         # class after class: one of the allowed interleavings
        ious = {}
        for j in order:
            for g in cov_g:
                if gt_cls[g] != dt_cls[j]:
                    continue
                inter = int((cov_g[g] & cov_d[j]).sum())
                iou = ious[g, j] = inter / (int(g_pix[g]) + int(d_pix[j]) - inter) if inter > 0 else 0.0
                if iou > d_best[j]:
                    d_best[j] = iou
                if iou > g_best[g]:
                    g_best[g] = iou
        for t, lim in enumerate(lims):
            taken = set()
            for j in order:
                best, m = lim, -1
                for g in cov_g:                             # ascending: `>=` leaves the highest index of equal IoUs
                    if gt_cls[g] != dt_cls[j] or g in taken:
                        continue
                    iou = ious[g, j]
                    if iou == 0.0 or not iou >= best:       # inter > 0 and iou >= lim
                        continue
                    best, m = iou, g
                if m < 0:
                    continue
                taken.add(m)
                tp[j] |= 1 << t
                hit[m] |= 1 << t
                if t == 0:
                    gt[j], d_iou[j] = m - g0, best
    return (status, pair_off, g_act, d_act, g_pix, d_pix, np.asarray(state, np.int32), np.asarray(tp, np.uint32),
            np.asarray(gt, np.int32), np.asarray(d_iou, np.float64), np.asarray(d_best, np.float64), np.asarray(hit, np.uint32),
            np.asarray(g_best, np.float64))


# ------------------------------------------------------------------------------------------------ cells -> PolygonEvaluation
def _cell_polygons(cell):
    """[(object index, name, [(x, y)])] of a regular cell: every object with a polygon.ptList of {x, y} numbers"""
    out = []
    for k, o in enumerate(json.loads(cell).get("objects", [])):
        pts = o.get("polygon", {}).get("ptList") if isinstance(o, dict) else None
        if isinstance(pts, list):
            out.append((k, o.get("name"), [(float(p["x"]), float(p["y"])) for p in pts]))
    return out


def expected_polygon_evaluation(cells_gt, cells_pred, widths, heights, scores=None, score_key=None, iou_thresholds=None, max_dets=100,
                                max_pixels_per_row=1 << 26, max_pairs_per_row=1 << 20, sources=None, mismatch=None):
    """-> dict(classes, per_class, precision, score_at, recall, ap, per_row, detections, missed, totals); mismatch: rows reported
    as size_mismatch, which reach the rule without a size"""
    thr = np.asarray(THR if iou_thresholds is None else iou_thresholds, np.float64)
    T, n = len(thr), len(cells_gt)
    rows_g, rows_d = [_cell_polygons(c) for c in cells_gt], [_cell_polygons(c) for c in cells_pred]
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
    sc = np.asarray(sc, np.float64)

    def table(rows):
        flat = [b for r in rows for b in r]
        row_off = np.zeros(n + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=row_off[1:])
        pt_off = np.zeros(len(flat) + 1, np.int64)
        np.cumsum([len(b[2]) for b in flat], out=pt_off[1:])
        xy = np.asarray([v for b in flat for p in b[2] for v in p], np.float64)
        return xy, pt_off, row_off, np.asarray([cid[b[1] if isinstance(b[1], str) else None] for b in flat], np.int64), flat

    xy_g, pt_g, off_g, cls_g, flat_g = table(rows_g)
    xy_d, pt_d, off_d, cls_d, flat_d = table(rows_d)
    W = np.asarray([float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else math.nan for v in widths], np.float64)
    H = np.asarray([float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) else math.nan for v in heights], np.float64)
    if mismatch is not None:
        W, H = np.where(mismatch, np.nan, W), np.where(mismatch, np.nan, H)
    (status, _, g_act, d_act, g_pix, d_pix, state, tp, gt, d_iou, d_best, hit, g_best) = match_polygon_rows(
        xy_g, pt_g, off_g, cls_g, xy_d, pt_d, off_d, cls_d, sc, W, H, max(C, 1), thr, max_dets, max_pixels_per_row, max_pairs_per_row)
    live = g_act == 0
    ev = np.flatnonzero(state == 0)
    npig = np.bincount(cls_g[live], minlength=C)[:C] if C else np.zeros(0, np.int64)
    precision, score_at, recall, ap, f1, bs, btp, bd = accumulate(cls_d[ev], sc[ev], tp[ev], C, T, npig)
    row_d = np.repeat(np.arange(n), np.diff(off_d))
    row_g = np.repeat(np.arange(n), np.diff(off_g))
    tp0, hit0 = (tp & 1).astype(bool), (hit & 1).astype(bool)

    def at(value):
        k = [i for i, t in enumerate(thr.tolist()) if t == value]
        return k[0] if k else None

    k50, k75 = at(0.5), at(0.75)
    per_class = []
    for c in range(C):
        dc, gc = cls_d == c, (cls_g == c) & live
        e = int((dc & (state == 0)).sum())
        t0 = int((dc & tp0).sum())
        per_class.append((classes[c], int(gc.sum()), int(dc.sum()), e, int((dc & (state == 1)).sum()), int((dc & (state == 2)).sum()),
                          _nanmean(ap[c]), ap[c, k50] if k50 is not None else float("nan"),
                          ap[c, k75] if k75 is not None else float("nan"), _nanmean(recall[c]), t0, e - t0, int(gc.sum()) - t0,
                          f1[c, 0], bs[c, 0], btp[c, 0] / bd[c, 0] if bd[c, 0] else float("nan"),
                          btp[c, 0] / int(gc.sum()) if bd[c, 0] else float("nan"),
                          int(((cls_g == c) & ~live).sum()), int((dc & (state == 3)).sum())))
    per_class = pd.DataFrame(per_class, columns=["class", "gt_polygons", "detections", "evaluated", "cut", "bad_score", "ap", "ap50",
                                                 "ap75", "recall", "tp", "fp", "fn", "best_f1", "best_score", "precision_at_best",
                                                 "recall_at_best", "gt_skipped", "dt_skipped"])
    per_class["class"] = per_class["class"].astype(object)
    pr = {"row": np.arange(n, dtype=np.int64)}
    if sources is not None:
        pr["source"] = np.asarray(sources, object)
    tp_r = np.bincount(row_d[tp0], minlength=n)
    n_gt = np.bincount(row_g[live], minlength=n)
    names_r = np.asarray(STATUS, object)[status]
    if mismatch is not None:
        names_r[np.asarray(mismatch, bool)] = "size_mismatch"
    pixels = np.asarray([int(W[r]) * int(H[r]) if status[r] == 0 else 0 for r in range(n)], np.int64)
    pr.update({"gt_polygons": n_gt, "detections": np.diff(off_d), "tp": tp_r,
               "fp": np.bincount(row_d[state == 0], minlength=n) - tp_r, "fn": n_gt - tp_r, "status": names_r, "pixels": pixels})
    src = (lambda r: (sources[r],)) if sources is not None else (lambda r: ())
    name_of = lambda b: b[1] if isinstance(b[1], str) else None   # noqa: E731
    dets = [(int(row_d[j]), *src(int(row_d[j])), flat_d[j][0], name_of(flat_d[j]), float(sc[j]), STATES[state[j]], bin(int(tp[j])).count("1"), flat_g[off_g[row_d[j]] + gt[j]][0] if gt[j] >= 0 else -1, float(d_iou[j]),
             float(d_best[j]), int(d_pix[j])) for j in range(len(flat_d))]
    detections = pd.DataFrame(dets, columns=["row", *(("source",) if sources is not None else ()), "object", "name", "score",
                                             "state", "tp_thresholds", "gt_object", "iou", "best_iou", "pixels"])
    miss = [(int(row_g[g]), *src(int(row_g[g])), flat_g[g][0], name_of(flat_g[g]), float(g_best[g]), int(g_pix[g]))
            for g in range(len(flat_g)) if live[g] and not hit0[g]]
    missed = pd.DataFrame(miss, columns=["row", *(("source",) if sources is not None else ()), "object", "name", "best_iou", "pixels"])
    has = npig > 0
    totals = {"rows": n, "gt_polygons": int(live.sum()), "detections": len(flat_d), "evaluated": int((state == 0).sum()),
              "cut": int((state == 1).sum()), "bad_score": int((state == 2).sum()), "skipped": int((state == 3).sum()),
              "gt_skipped": int((~live).sum()),
              "map": _nanmean(per_class["ap"][has]), "map50": _nanmean(ap[has, k50]) if k50 is not None else float("nan"),
              "map75": _nanmean(ap[has, k75]) if k75 is not None else float("nan"), "mar": _nanmean(per_class["recall"][has]),
              "max_dets": int(max_dets), "pixels": int(pixels.sum()),
              **{f"rows_{s}": int((names_r == s).sum()) for s in (*STATUS, "size_mismatch")}}
    return {"classes": classes, "iou_thresholds": thr, "per_class": per_class, "precision": precision, "score_at": score_at,
            "recall": recall, "ap": ap, "per_row": pd.DataFrame(pr), "detections": detections, "missed": missed, "totals": totals}
