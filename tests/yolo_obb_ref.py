"""The YOLO oriented-box labels (K17) restated from their definition, for tests/test_yolo_obb_cpu.py and
tests/test_gpu_yolo_obb.py.  Polygons, checks, clip and number handling are K13's (tests/yolo_seg_ref.py); the new part is the
minimum-area enclosing rectangle of the clipped vertices.  Two levels:

- ``obb_row``: one split-sheet row (cell, label, class id, width, height) -> (text, reason, actions);
- ``obb_arrays``: what K17 computes from the arrays -> (text_off, flag, action, text, clamped, corners).
"""
import numpy as np

import yolo_seg_ref as S

ACTIONS = S.ACTIONS + ("flat",)


def rectangle(C):
    """the walk over the clipped vertices C = [(x, y) floats] -> (kept area or None, its four corners or None)"""
    m = len(C)
    s = C[0]
    lx = hx = s[0]
    ly = hy = s[1]
    for x, y in C[1:]:
        if y < s[1] or (y == s[1] and x < s[0]):
            s = (x, y)
        if x < lx:
            lx = x
        if x > hx:
            hx = x
        if y < ly:
            ly = y
        if y > hy:
            hy = y
    cx, cy = s
    kept_area, kept = None, None
    for _ in range(m):
        best, bd = None, 0.0
        for kx, ky in C:
            if kx == cx and ky == cy:
                continue
            d = (kx - cx) * (kx - cx) + (ky - cy) * (ky - cy)
            if best is None:
                best, bd = (kx, ky), d
                continue
            cr = (best[0] - cx) * (ky - cy) - (best[1] - cy) * (kx - cx)
            if cr < 0 or (cr == 0 and d > bd):
                best, bd = (kx, ky), d
        if best is None:
            break
        dx, dy = best[0] - cx, best[1] - cy
        if dx == 0 or dy == 0:
            area = (hx - lx) * (hy - ly)
            corners = [(lx, ly), (hx, ly), (hx, hy), (lx, hy)]
        else:
            a = b = e = f = None
            for x, y in C:
                u = (x - cx) * dx + (y - cy) * dy
                v = (y - cy) * dx - (x - cx) * dy
                if a is None:
                    a = b = u
                    e = f = v
                    continue
                if u < a:
                    a = u
                if u > b:
                    b = u
                if v < e:
                    e = v
                if v > f:
                    f = v
            L = dx * dx + dy * dy
            area = ((b - a) * (f - e)) / L
            corners = [(cx + (u * dx - v * dy) / L, cy + (u * dy + v * dx) / L) for u, v in ((a, e), (b, e), (b, f), (a, f))]
        if kept_area is None or area < kept_area:
            kept_area, kept = area, corners
        cx, cy = best
        if cx == s[0] and cy == s[1]:
            break
    return kept_area, kept


def polygon(raw, W, H, cid):
    """-> (action, line or None, clamped, corners or None) of one matched polygon; W, H usable sizes (floats) or None"""
    act, line = S.polygon(raw, W, H, cid)
    if line is None:
        return act, None, 0, None
    V = [(S.coord(x), S.coord(y)) for x, y in raw]
    if len(V) == 2:
        x1, x2 = min(V[0][0], V[1][0]), max(V[0][0], V[1][0])
        y1, y2 = min(V[0][1], V[1][1]), max(V[0][1], V[1][1])
        V = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    area, corners = rectangle(S.clip(V, W, H))
    if area is None or not area > 0:
        return "flat", None, 0, None
    clamped = int(any(x < 0 or x > W or y < 0 or y > H for x, y in corners))
    return act, f"{cid}" + "".join(f" {S.norm(x / W):.6f} {S.norm(y / H):.6f}" for x, y in corners), clamped, corners


def obb_row(cell, label, cid, w, h):
    """-> (text or None, reason or None, [action per matched polygon])"""
    polys = S.matched_polygons(cell, label)
    if not polys:
        return None, S.NO_MATCH, []
    if not w or not h:
        return None, S.NO_SIZE, []
    W, H = S.size_of(w), S.size_of(h)
    res = [polygon(p, W, H, cid) for p in polys]
    lines = [r[1] for r in res if r[1] is not None]
    acts = [r[0] for r in res]
    return ("\n".join(lines), None, acts) if lines else (None, S.NO_LINE, acts)


def obb_arrays(xy, pt_off, row_off, sel, width, height, class_id):
    """K17 on arrays -> (text_off int64 [n+1], flag u8 [n], action u8 [B], text bytes, clamped u8 [B], corners f64 [B, 8],
    NaN where the polygon has no line)"""
    xy = np.asarray(xy, np.float64).reshape(-1)
    n = len(row_off) - 1
    nb = int(row_off[-1]) if n else 0
    off, flag = np.zeros(n + 1, np.int64), np.zeros(n, np.uint8)
    action = np.full(nb, 255, np.uint8)
    clamped = np.zeros(nb, np.uint8)
    corners = np.full((nb, 8), np.nan)
    parts = []
    for i in range(n):
        W, H, cid = float(width[i]), float(height[i]), int(class_id[i])
        Wok, Hok = S.size_of(W), S.size_of(H)
        lines = []
        for b in range(int(row_off[i]), int(row_off[i + 1])):
            if sel is not None and not sel[b]:
                continue
            raw = [(float(xy[2 * k]), float(xy[2 * k + 1])) for k in range(int(pt_off[b]), int(pt_off[b + 1]))]
            act, line, cl, cs = polygon(raw, Wok, Hok, cid)
            action[b] = ACTIONS.index(act)
            if line is not None:
                lines.append(line)
                clamped[b] = cl
                corners[b] = [v for c in cs for v in c]
        if W == 0.0 or H == 0.0 or cid < 0:
            flag[i] = 2
            text = ""
        else:
            flag[i] = 0 if lines else 1
            text = "\n".join(lines)
        parts.append(text)
        off[i + 1] = off[i] + len(text)
    return off, flag, action, "".join(parts).encode("ascii"), clamped, corners
