"""The YOLO segmentation labels (K13) restated from their definition, for tests/test_yolo_seg_cpu.py and
tests/test_gpu_yolo_seg.py.  Two levels:

- ``seg_row``: one split-sheet row (cell, label, class id, width, height) -> (text, reason, actions), CPython's json and float();
- ``seg_arrays``: what K13 computes from the arrays (xy, pt_off, row_off, sel, W, H, class ids) -> (text_off, flag, action, text).
"""
import json
import math

import numpy as np

NUMBER = (int, float, np.integer, np.floating)
LIMIT = float(2 ** 43)
ACTIONS = ("written", "clipped", "bad_coords", "too_few_points", "empty", "no_size")
NO_MATCH, NO_SIZE, NO_LINE = "无匹配标签框", "缺少图像尺寸", "标注框无效"


def matched_polygons(cell, label):
    """the detect step's objects (utils._extract_boxes_with_labels: prefix kept on any exception) whose name is the label ->
    [[(x, y) as read for every ptList dict holding both]]"""
    out = []
    if not isinstance(cell, str):
        return out
    try:
        for obj in json.loads(cell).get("objects", []):
            if not isinstance(obj, dict):
                continue
            name = obj.get("name")
            if not name:
                continue
            points = obj.get("polygon", {}).get("ptList", [])
            if not points:
                continue
            dpts = [p for p in points if isinstance(p, dict)]
            xs = [p.get("x") for p in dpts if "x" in p]
            ys = [p.get("y") for p in dpts if "y" in p]
            if xs and ys:
                min(xs), min(ys), max(xs), max(ys)          # raises where the detect step does
                if name == label:
                    out.append([(p["x"], p["y"]) for p in dpts if "x" in p and "y" in p])
    except Exception:                                       # noqa: BLE001
        pass
    return out


def size_of(v):
    if not isinstance(v, NUMBER):
        return None
    try:
        f = float(v)
    except OverflowError:
        return None
    return f if math.isfinite(f) and 0.0 < f < LIMIT else None


def coord(v):
    if not isinstance(v, NUMBER):
        return None
    try:
        f = float(v)
    except OverflowError:
        return None
    return f if math.isfinite(f) and abs(f) < LIMIT else None


def clip(V, W, H):
    for inside, axis, c in ((lambda p: p[0] >= 0.0, 0, 0.0), (lambda p: p[0] <= W, 0, W),
                            (lambda p: p[1] >= 0.0, 1, 0.0), (lambda p: p[1] <= H, 1, H)):
        out, n = [], len(V)
        for k in range(n):
            p, q = V[k], V[(k + 1) % n]
            if inside(p):
                out.append(p)
            if inside(p) != inside(q):
                if axis == 0:
                    t = (c - p[0]) / (q[0] - p[0])
                    out.append((c, p[1] + t * (q[1] - p[1])))
                else:
                    t = (c - p[1]) / (q[1] - p[1])
                    out.append((p[0] + t * (q[0] - p[0]), c))
        V = out
    return V


def norm(v):
    return 0.0 if v <= 0.0 else (1.0 if v >= 1.0 else v)


def polygon(raw, W, H, cid):
    """-> (action, line or None) of one matched polygon; W, H usable sizes (floats) or None"""
    if W is None or H is None:
        return "no_size", None
    V = [(coord(x), coord(y)) for x, y in raw]
    if any(v is None for p in V for v in p):
        return "bad_coords", None
    if len(V) < 2:
        return "too_few_points", None
    if len(V) == 2:
        x1, x2 = min(V[0][0], V[1][0]), max(V[0][0], V[1][0])
        y1, y2 = min(V[0][1], V[1][1]), max(V[0][1], V[1][1])
        V = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    out = clip(V, W, H)
    if len(out) < 3 or max(p[0] for p in out) - min(p[0] for p in out) <= 0 or max(p[1] for p in out) - min(p[1] for p in out) <= 0:
        return "empty", None
    act = "clipped" if any(not (x >= 0.0 and x <= W and y >= 0.0 and y <= H) for x, y in V) else "written"
    return act, f"{cid}" + "".join(f" {norm(x / W):.6f} {norm(y / H):.6f}" for x, y in out)


def seg_row(cell, label, cid, w, h):
    """-> (text or None, reason or None, [action per matched polygon])"""
    polys = matched_polygons(cell, label)
    if not polys:
        return None, NO_MATCH, []
    if not w or not h:
        return None, NO_SIZE, []
    W, H = size_of(w), size_of(h)
    res = [polygon(p, W, H, cid) for p in polys]
    lines = [line for _, line in res if line is not None]
    acts = [a for a, _ in res]
    return ("\n".join(lines), None, acts) if lines else (None, NO_LINE, acts)


def seg_arrays(xy, pt_off, row_off, sel, width, height, class_id):
    """K13 on arrays -> (text_off int64 [n+1], flag u8 [n], action u8 [B], text bytes)"""
    xy = np.asarray(xy, np.float64).reshape(-1)
    n = len(row_off) - 1
    off, flag = np.zeros(n + 1, np.int64), np.zeros(n, np.uint8)
    action = np.full(int(row_off[-1]) if n else 0, 255, np.uint8)
    parts = []
    for i in range(n):
        W, H, cid = float(width[i]), float(height[i]), int(class_id[i])
        Wok, Hok = size_of(W), size_of(H)
        lines = []
        for b in range(int(row_off[i]), int(row_off[i + 1])):
            if sel is not None and not sel[b]:
                continue
            raw = [(float(xy[2 * k]), float(xy[2 * k + 1])) for k in range(int(pt_off[b]), int(pt_off[b + 1]))]
            act, line = polygon(raw, Wok, Hok, cid)
            action[b] = ACTIONS.index(act)
            if line is not None:
                lines.append(line)
        if W == 0.0 or H == 0.0 or cid < 0:
            flag[i] = 2
            text = ""
        else:
            flag[i] = 0 if lines else 1
            text = "\n".join(lines)
        parts.append(text)
        off[i + 1] = off[i] + len(text)
    return off, flag, action, "".join(parts).encode("ascii")
