"""The polygon simplification restated from its definition (include/dyd.h, K19), for
tests/test_polygon_simplify_cpu.py and tests/test_gpu_polygon_simplify.py.  Three levels:

- ``simplify``: one polygon, pure Python, recursive (``simplify_rounds``: the same rule in rounds over all current segments).
- ``simplify_arrays``: what K19 computes from the scanned arrays (xy, pt_off), the ABI's shape.
- ``simplify_table``: cells -> everything simplify_polygons_* returns, via json.loads.
"""
import json
import math
import sys

import numpy as np

from box_audit_ref import boxes_of, fval

ACTIONS = ("kept", "simplified", "bad_coords", "too_few_points")
LIMIT = 2.0 ** 43
LAST_ROUNDS = 0                        # the rounds simplify_rounds' last call took below the roots


def dist2(P, Q, v):
    """s(k; i, j): the squared distance of v from the segment (P, Q), operation by operation as the definition writes it"""
    dx, dy = Q[0] - P[0], Q[1] - P[1]
    ex, ey = v[0] - P[0], v[1] - P[1]
    L2 = dx * dx + dy * dy
    t = dx * ex + dy * ey
    if L2 == 0.0 or t <= 0.0:
        return ex * ex + ey * ey
    if t >= L2:
        fx, fy = v[0] - Q[0], v[1] - Q[1]
        return fx * fx + fy * fy
    c = dx * ey - dy * ex
    return (c * c) / L2


def farthest(V, i, j):
    """(s*, k*) of the segment (i, j), j == len(V) standing for vertex 0; (None, None) without interior vertices"""
    P, Q = V[i], V[j % len(V)]
    best, arg = None, None
    for k in range(i + 1, j):
        s = dist2(P, Q, V[k])
        if best is None or s > best:
            best, arg = s, k
    return best, arg


def _untouched(V):
    m = len(V)
    if any(not (math.isfinite(c) and abs(c) < LIMIT) for p in V for c in p):
        return 2
    if m < 4:
        return 3
    return None


def _anchor(V):
    x0, y0 = V[0]
    best, b = 0.0, 0
    for k, (x, y) in enumerate(V):
        d = (x - x0) * (x - x0) + (y - y0) * (y - y0)
        if d > best:
            best, b = d, k
    return best, b


def _roots(V, b, e2):
    """the root segments that split: [(i, j, k*)], and the s* of those that do not"""
    m = len(V)
    s0, k0 = farthest(V, 0, b)
    s1, k1 = farthest(V, b, m)
    split0, split1 = s0 is not None and s0 > e2, s1 is not None and s1 > e2
    if not split0 and not split1:
        if s0 is not None and (s1 is None or s0 >= s1):
            split0 = True
        else:
            split1 = True
    splits, ended = [], []
    for split, s, k, (i, j) in ((split0, s0, k0, (0, b)), (split1, s1, k1, (b, m))):
        if split:
            splits.append((i, j, k))
        elif s is not None:
            ended.append(s)
    return splits, ended


def simplify(V, tol):
    """-> (keep list of 0 / 1, action code, kept, dev2) of one polygon V = [(x, y)] of floats, recursive"""
    m = len(V)
    act = _untouched(V)
    if act is not None:
        return [1] * m, act, m, 0.0
    best, b = _anchor(V)
    if best == 0.0:
        return [1] * m, 0, m, 0.0
    e2 = tol * tol
    keep = [0] * m
    keep[0] = keep[b] = 1
    ended = []

    def rec(i, j):
        s, k = farthest(V, i, j)
        if s is None:
            return
        if s > e2:
            keep[k] = 1
            rec(i, k)
            rec(k, j)
        else:
            ended.append(s)

    splits, root_ended = _roots(V, b, e2)
    ended += root_ended
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 2 * m + 200))
    try:
        for i, j, k in splits:
            keep[k] = 1
            rec(i, k)
            rec(k, j)
    finally:
        sys.setrecursionlimit(old)
    kept = sum(keep)
    return keep, (1 if kept < m else 0), kept, (max(ended) if ended else 0.0)


def simplify_rounds(V, tol):
    """simplify in rounds: every current segment is split at once"""
    m = len(V)
    act = _untouched(V)
    if act is not None:
        return [1] * m, act, m, 0.0
    best, b = _anchor(V)
    if best == 0.0:
        return [1] * m, 0, m, 0.0
    e2 = tol * tol
    keep = [0] * m
    keep[0] = keep[b] = 1
    splits, ended = _roots(V, b, e2)
    global LAST_ROUNDS
    LAST_ROUNDS = 0
    cur = []
    for i, j, k in splits:
        keep[k] = 1
        cur += [(i, k), (k, j)]
    while cur:
        LAST_ROUNDS += 1
        nxt = []
        for i, j in cur:
            s, k = farthest(V, i, j)
            if s is None:
                continue
            if s > e2:
                keep[k] = 1
                nxt += [(i, k), (k, j)]
            else:
                ended.append(s)
        cur = nxt
    kept = sum(keep)
    return keep, (1 if kept < m else 0), kept, (max(ended) if ended else 0.0)


def simplify_arrays(xy, pt_off, tolerance=1.0):
    """K19 restated -> (keep u8 [P], action u8 [B], kept i32 [B], dev2 f64 [B])"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pt_off = np.asarray(pt_off, np.int64)
    nb = len(pt_off) - 1
    keep = np.ones(len(xy), np.uint8)
    action, kept, dev2 = np.zeros(nb, np.uint8), np.zeros(nb, np.int32), np.zeros(nb, np.float64)
    tol = float(tolerance)
    for p in range(nb):
        a, b = int(pt_off[p]), int(pt_off[p + 1])
        V = [tuple(v) for v in xy[a:b].tolist()]
        k, action[p], kept[p], dev2[p] = simplify(V, tol)
        keep[a:b] = k
    return keep, action, kept, dev2


def polygons_of(cell):
    """the audit's polygons of one cell: [(object, name, [(x, y) as floats, NaN for a non-number])]"""
    bx = boxes_of(cell)
    if not bx:
        return []
    objs = json.loads(cell)["objects"]
    out = []
    for k, name, *_ in bx:
        pts = objs[k]["polygon"]["ptList"]
        out.append((k, name, [(fval(p["x"]), fval(p["y"])) for p in pts if isinstance(p, dict) and "x" in p and "y" in p]))
    return out


def simplify_table(cells, tolerance=1.0):
    """-> {"cells": the output cells, "changes": [(row, object, name, points, kept, max_deviation)],
    "counts": {class: {action..., points_in, points_out}}, "classes": sorted str names, "totals": {...}}"""
    tol = float(tolerance)
    out, changes, counts = [], [], {}
    totals = {"rows": len(cells), "rows_changed": 0, "polygons": 0, "polygons_simplified": 0, "points": 0, "points_removed": 0,
              "tolerance": tol}
    for i, c in enumerate(cells):
        dec = {}
        for k, name, V in polygons_of(c):
            keep, act, kept, dev2 = simplify(V, tol)
            totals["polygons"] += 1
            totals["points"] += len(V)
            if isinstance(name, str):
                cc = counts.setdefault(name, dict.fromkeys((*ACTIONS, "points_in", "points_out"), 0))
                cc[ACTIONS[act]] += 1
                cc["points_in"] += len(V)
                cc["points_out"] += kept
            if act == 1:
                dec[k] = keep
                changes.append((i, k, name, len(V), kept, math.sqrt(dev2)))
                totals["polygons_simplified"] += 1
                totals["points_removed"] += len(V) - kept
        if not dec:
            out.append(c)
            continue
        doc = json.loads(c)
        for k, keep in dec.items():
            poly = doc["objects"][k]["polygon"]
            flags = iter(keep)
            poly["ptList"] = [p for p in poly["ptList"] if not (isinstance(p, dict) and "x" in p and "y" in p) or next(flags)]
        out.append(json.dumps(doc, ensure_ascii=False))
        totals["rows_changed"] += 1
    return {"cells": out, "changes": changes, "counts": counts, "classes": sorted(counts), "totals": totals}


def check_simplify(res, ref, cells=None, stats=None):
    """assert that simplify_polygons_cells' (cells, changes, per_class) equals simplify_table's answer; unchanged cells must be
    the input objects themselves"""
    out, changes, per_class = res
    assert len(out) == len(ref["cells"])
    changed_rows = {c[0] for c in ref["changes"]}
    for k, (a, b) in enumerate(zip(out, ref["cells"])):
        assert a == b or (a != a and b != b), k
        if cells is not None and k not in changed_rows:
            assert a is cells[k], k
    assert per_class["class"].tolist() == ref["classes"]
    for col in (*ACTIONS, "points_in", "points_out"):
        assert per_class[col].tolist() == [ref["counts"][c][col] for c in ref["classes"]], col
    assert (per_class["polygons"] == per_class[list(ACTIONS)].sum(axis=1)).all()
    assert list(per_class.columns) == ["class", "polygons", *ACTIONS, "points_in", "points_out"]
    assert list(changes.columns[-6:]) == ["row", "object", "name", "points", "kept", "max_deviation"]
    got = list(zip(changes["row"].tolist(), changes["object"].tolist(), changes["name"].tolist(), changes["points"].tolist(),
                   changes["kept"].tolist()))
    assert got == [c[:5] for c in ref["changes"]]
    want = np.asarray([c[5] for c in ref["changes"]], np.float64)
    assert np.array_equal(changes["max_deviation"].to_numpy(np.float64).view(np.uint64), want.view(np.uint64))
    if stats is not None:
        for k, v in ref["totals"].items():
            assert stats[k] == v, k
