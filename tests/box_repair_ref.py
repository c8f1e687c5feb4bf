"""The box repair restated from its definition, for tests/test_box_repair_cpu.py and
tests/test_gpu_box_repair.py.  Two levels:

- ``repair_table``: cells + sizes -> everything repair_boxes_* returns, in plain Python (CPython's json, float()).
- ``repair_arrays``: what K11 computes from the scanned arrays (box4, row_off, class ids, W, H, size status), in numpy.
"""
import json
import math

import numpy as np

from box_audit_ref import boxes_of, fnum, fval, size_status

ACTIONS = ("keep", "clip", "no_size", "bad_coords", "degenerate", "outside", "low_visibility", "small")
REMOVED = ("bad_coords", "degenerate", "outside", "low_visibility", "small")


def decide(box, st, W, H, min_visibility=0.0, min_size=0.0):
    """-> (action, clipped corners or None) of one box (its raw min x, min y, max x, max y)"""
    if st != "ok":
        return "no_size", None
    c = [fnum(v) for v in box]
    if any(v is None for v in c):
        return "bad_coords", None
    x1, y1, x2, y2 = c
    if max(x2 - x1, 0.0) <= 0 or max(y2 - y1, 0.0) <= 0:
        return "degenerate", None
    cx1 = 0.0 if x1 < 0 else x1
    cy1 = 0.0 if y1 < 0 else y1
    cx2 = W if x2 > W else x2
    cy2 = H if y2 > H else y2
    bw, bh = max(cx2 - cx1, 0.0), max(cy2 - cy1, 0.0)
    clipped = x1 < 0 or y1 < 0 or x2 > W or y2 > H
    if bw <= 0 or bh <= 0:
        return "outside", None
    if bw * bh < min_visibility * ((x2 - x1) * (y2 - y1)):
        return "low_visibility", None
    if bw < min_size or bh < min_size:
        return "small", None
    if clipped:
        return "clip", (cx1, cy1, cx2, cy2)
    return "keep", None


def repair_table(cells, widths, heights, min_visibility=0.0, min_size=0.0):
    """-> {"cells": the output cells, "changes": [(row, object, name, action, x1, y1, x2, y2, nx1, ny1, nx2, ny2)],
    "counts": {class: {action: n}}, "classes": sorted str names, "totals": {...}}"""
    n = len(cells)
    if widths is None:
        widths = heights = [None] * n
    out, changes, counts = [], [], {}
    totals = {"rows": n, "rows_changed": 0, "boxes": 0, "boxes_clipped": 0, "boxes_removed": 0, "rows_no_size": 0}
    for i in range(n):
        st, W, H = size_status(widths[i], heights[i])
        totals["rows_no_size"] += st != "ok"
        bx = boxes_of(cells[i])
        totals["boxes"] += len(bx)
        clips, removed = {}, set()
        for k, name, *box in bx:
            act, cbox = decide(box, st, W, H, min_visibility, min_size)
            if isinstance(name, str):
                counts.setdefault(name, dict.fromkeys(ACTIONS, 0))[act] += 1
            if act == "clip":
                clips[k] = cbox
                changes.append((i, k, name, act, *[fval(v) for v in box], *cbox))
            elif act in REMOVED:
                removed.add(k)
                changes.append((i, k, name, act, *[fval(v) for v in box], math.nan, math.nan, math.nan, math.nan))
        totals["boxes_clipped"] += len(clips)
        totals["boxes_removed"] += len(removed)
        if not clips and not removed:
            out.append(cells[i])
            continue
        doc = json.loads(cells[i])
        objs = doc["objects"]
        for k, (a, b, c, d) in clips.items():
            objs[k]["polygon"]["ptList"] = [{"x": float(a), "y": float(b)}, {"x": float(c), "y": float(d)}]
        doc["objects"] = [o for k, o in enumerate(objs) if k not in removed]
        out.append(json.dumps(doc, ensure_ascii=False))
        totals["rows_changed"] += 1
    return {"cells": out, "changes": changes, "counts": counts, "classes": sorted(counts), "totals": totals}


def check_repair(res, ref, cells=None, stats=None):
    """assert that repair_boxes_cells' (cells, changes, per_class) equals repair_table's answer; unchanged cells must be the
    input objects themselves"""
    out, changes, per_class = res
    assert len(out) == len(ref["cells"])
    for k, (a, b) in enumerate(zip(out, ref["cells"])):
        assert a == b or (a != a and b != b), k
        if cells is not None and not any(c[0] == k for c in ref["changes"]):
            assert a is cells[k], k
    assert per_class["class"].tolist() == ref["classes"]
    for act in ACTIONS:
        assert per_class[act].tolist() == [ref["counts"][c][act] for c in ref["classes"]], act
    assert (per_class["boxes"] == per_class[list(ACTIONS)].sum(axis=1)).all()
    assert list(changes.columns[-12:]) == ["row", "object", "name", "action", "x1", "y1", "x2", "y2", "nx1", "ny1", "nx2", "ny2"]
    got = list(zip(changes["row"].tolist(), changes["object"].tolist(), changes["name"].tolist(), changes["action"].tolist()))
    assert got == [c[:4] for c in ref["changes"]]
    for j, col in enumerate(("x1", "y1", "x2", "y2", "nx1", "ny1", "nx2", "ny2")):
        want = np.asarray([c[4 + j] for c in ref["changes"]], np.float64)
        assert np.array_equal(changes[col].to_numpy(np.float64), want, equal_nan=True), col
    if stats is not None:
        for k, v in ref["totals"].items():
            assert stats[k] == v, k


def repair_arrays(box4, row_off, cls, W, H, status, n_classes, min_visibility=0.0, min_size=0.0):
    """K11 restated in numpy -> (action [B] u8, box4 [B,4] f64, row_counts [N,8] i32, class_counts [C,8] i64)"""
    box4 = np.asarray(box4, np.float64).reshape(-1, 4)
    row_off = np.asarray(row_off, np.int64)
    cls = np.asarray(cls, np.int64)
    n = len(row_off) - 1
    C = int(n_classes)
    row = np.repeat(np.arange(n), np.diff(row_off))
    x1, y1, x2, y2 = box4.T
    st = np.asarray(status)[row]
    w = np.asarray(W, np.float64)[row]
    h = np.asarray(H, np.float64)[row]
    unm = (cls < 0) | (cls >= C)
    mv, ms = float(min_visibility), float(min_size)
    with np.errstate(all="ignore"):
        finite = np.isfinite(box4).all(axis=1)
        bw, bh = x2 - x1, y2 - y1
        deg = (np.where(0.0 > bw, 0.0, bw) <= 0) | (np.where(0.0 > bh, 0.0, bh) <= 0)
        cx1, cy1 = np.where(x1 < 0, 0.0, x1), np.where(y1 < 0, 0.0, y1)
        cx2, cy2 = np.where(x2 > w, w, x2), np.where(y2 > h, h, y2)
        dx, dy = cx2 - cx1, cy2 - cy1
        cw, ch = np.where(0.0 > dx, 0.0, dx), np.where(0.0 > dy, 0.0, dy)
        clipped = (x1 < 0) | (y1 < 0) | (x2 > w) | (y2 > h)
        act = np.select([st != 0, ~finite, deg, (cw <= 0) | (ch <= 0), cw * ch < mv * (bw * bh), (cw < ms) | (ch < ms), clipped],
                        [2, 3, 4, 5, 6, 7, 1], 0).astype(np.int64)
    out = box4.copy()
    c1 = act == 1
    out[c1] = np.stack([cx1, cy1, cx2, cy2], axis=1)[c1]
    action = (act | np.where(unm, 0x80, 0)).astype(np.uint8)
    rows = np.bincount(row * 8 + act, minlength=8 * n).reshape(n, 8) if n else np.zeros((0, 8), np.int64)
    cc = (np.bincount((cls * 8 + act)[~unm], minlength=8 * C).reshape(C, 8) if C else np.zeros((0, 8), np.int64))
    return action, out, rows.astype(np.int32), cc.astype(np.int64)
