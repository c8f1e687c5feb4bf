"""The polygon audit (K14) restated from its definition (include/dyd.h), for tests/test_polygon_audit_cpu.py
and tests/test_gpu_polygon_audit.py.  The category is K13's action as yolo_seg_ref computes it; the defects work on any
number type with exact == and sign tests, so Fraction coordinates give the exact answer.

- ``defects(V, C, min_area)``: the defect bits of a written or clipped polygon (V as drawn, C its clipped vertices);
- ``polygon(raw, W, H, min_area)``: (category code, defect bits, area) of one polygon, W / H usable sizes or None;
- ``audit_arrays``: what K14 computes from the arrays -> (category, defects, area, class_counts, hist_vertices).
"""
import math

import numpy as np

import yolo_seg_ref as S

DUP, SELFX, TINY = 1, 2, 4
DEFECTS = ("duplicate_vertices", "self_intersecting", "tiny_area")
UNMATCHABLE = 255
HIST_EDGES = (2, 3, 4, 8, 16, 32, 64, 128, 256, 1024)
CLASS_COLS = ("polygons", "images", *S.ACTIONS, *DEFECTS, "small", "medium", "large")


def o(p, q, r):
    return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def on_box(p, q, r):
    return min(p[0], q[0]) <= r[0] <= max(p[0], q[0]) and min(p[1], q[1]) <= r[1] <= max(p[1], q[1])


def segments_meet(a, b, c, d):
    d1, d2, d3, d4 = o(c, d, a), o(c, d, b), o(a, b, c), o(a, b, d)
    if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
        return True
    return ((d1 == 0 and on_box(c, d, a)) or (d2 == 0 and on_box(c, d, b)) or (d3 == 0 and on_box(a, b, c))
            or (d4 == 0 and on_box(a, b, d)))


def without_repeats(V):
    """V without cyclically consecutive duplicates (one vertex when all are equal)"""
    U = [p for k, p in enumerate(V) if p != V[k - 1]]
    return U if U else list(V[:1])


def self_intersecting(V):
    if len(V) < 3:
        return False
    U = without_repeats(V)
    m = len(U)
    if m < 3:
        return False
    for k in range(m):
        a, b, c = U[k], U[(k + 1) % m], U[(k + 2) % m]
        if o(a, b, c) == 0 and (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1]) < 0:
            return True
    for i in range(m):
        for j in range(i + 2, m):
            if i == 0 and j == m - 1:
                continue
            if segments_meet(U[i], U[(i + 1) % m], U[j], U[(j + 1) % m]):
                return True
    return False


def area(C):
    s = 0.0
    for k in range(len(C)):
        s += C[k][0] * C[(k + 1) % len(C)][1] - C[(k + 1) % len(C)][0] * C[k][1]
    return abs(s) * 0.5


def defects(V, C, min_area):
    bits = 0
    if len(V) >= 3 and any(V[k] == V[k - 1] for k in range(len(V))):
        bits |= DUP
    if self_intersecting(V):
        bits |= SELFX
    if area(C) < min_area:
        bits |= TINY
    return bits


def clipped(V, W, H):
    if len(V) == 2:
        x1, x2 = min(V[0][0], V[1][0]), max(V[0][0], V[1][0])
        y1, y2 = min(V[0][1], V[1][1]), max(V[0][1], V[1][1])
        V = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    return S.clip(V, W, H)


def polygon(raw, W, H, min_area=1.0):
    """raw: [(x, y)] floats as K13 reads them -> (category code, defect bits, area or NaN)"""
    act, _ = S.polygon(raw, W, H, 0)
    code = S.ACTIONS.index(act)
    if act not in ("written", "clipped"):
        return code, 0, math.nan
    V = [(float(x), float(y)) for x, y in raw]
    C = clipped(V, W, H)
    return code, defects(V, C, min_area), area(C)


def hist_bin(n):
    for k, e in enumerate(HIST_EDGES):
        if n <= e:
            return k
    return len(HIST_EDGES)


def audit_arrays(xy, pt_off, row_off, cls, width, height, status, n_classes, min_area=1.0):
    xy = np.asarray(xy, np.float64).reshape(-1)
    n, nb = len(row_off) - 1, int(row_off[-1]) if len(row_off) > 1 else 0
    cat, dfc, ar = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), np.full(nb, np.nan)
    cc = np.zeros((n_classes, len(CLASS_COLS)), np.int64)
    hist = np.zeros((n_classes, len(HIST_EDGES) + 1), np.int64)
    for i in range(n):
        ok = int(status[i]) == 0
        W, H = (S.size_of(float(width[i])), S.size_of(float(height[i]))) if ok else (None, None)
        seen = set()
        for p in range(int(row_off[i]), int(row_off[i + 1])):
            c = int(cls[p])
            if c < 0:
                cat[p] = UNMATCHABLE
                continue
            raw = [(float(xy[2 * k]), float(xy[2 * k + 1])) for k in range(int(pt_off[p]), int(pt_off[p + 1]))]
            code, bits, a = polygon(raw, W, H, min_area)
            cat[p], dfc[p], ar[p] = code, bits, a
            cc[c, 0] += 1
            if c not in seen:
                cc[c, 1] += 1
                seen.add(c)
            cc[c, 2 + code] += 1
            for k in range(3):
                cc[c, 8 + k] += bits >> k & 1
            if code <= 1:
                cc[c, 11 + (0 if a < 1024.0 else (1 if a < 9216.0 else 2))] += 1
            hist[c, hist_bin(len(raw))] += 1
    return cat, dfc, ar, cc, hist
