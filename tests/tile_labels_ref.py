"""The tiled YOLO labels (K20) restated from their definition (include/dyd.h, the K20 block), for
tests/test_tile_labels_cpu.py and tests/test_gpu_tile_labels.py.  Plain Python floats and ints, operation by operation:

- ``axis`` / ``row_grid``: the grid of one image row;
- ``tile_polygon``: one polygon seen from one tile -> None (no part), or (written, cut, line);
- ``tile_arrays``: what K20 computes from the arrays -> (row_status, tile_off, tile_line_count, text_off, action,
  tiles_written, tiles_cut, tiles_dropped, text).
"""
import numpy as np

import polygon_audit_ref as A
import yolo_seg_ref as S

STATUS = ("tiled", "no_size", "fractional_size", "too_many_tiles")
MAX_TILE = 1 << 20


def check_params(tile_w, tile_h, step_x, step_y, min_visibility, mode, max_tiles_per_row):
    for t, s in ((tile_w, step_x), (tile_h, step_y)):
        if not (isinstance(t, int) and isinstance(s, int) and 1 <= s <= t <= MAX_TILE):
            raise ValueError("need integers 1 <= step <= tile <= 2^20")
    if not (0.0 <= min_visibility <= 1.0):
        raise ValueError("min_visibility must lie in [0, 1]")
    if mode not in (0, 1) or not 1 <= max_tiles_per_row <= MAX_TILE:
        raise ValueError("mode is 0 or 1, max_tiles_per_row in 1..2^20")


def axis(L, T, S):
    """-> [(origin, extent)] of the tiles of one axis of length L"""
    if L <= T:
        return [(0, L)]
    n = -((T - L) // S) + 1                              # ceil((L - T) / S) + 1
    return [(min(j * S, L - T), T) for j in range(n)]


def row_grid(W, H, tile_w, tile_h, step_x, step_y, max_tiles_per_row):
    """-> (status, [(ox, oy, tw, th)] in the order ty * nx + tx)"""
    if S.size_of(W) is None or S.size_of(H) is None:
        return 1, []
    if W != int(W) or H != int(H):
        return 2, []
    xs, ys = axis(int(W), tile_w, step_x), axis(int(H), tile_h, step_y)
    if len(xs) * len(ys) > max_tiles_per_row:
        return 3, []
    return 0, [(ox, oy, tw, th) for oy, th in ys for ox, tw in xs]


def vertices(raw):
    """K13's vertex list of a polygon that passed its checks"""
    V = [(float(x), float(y)) for x, y in raw]
    if len(V) == 2:
        x1, x2 = min(V[0][0], V[1][0]), max(V[0][0], V[1][0])
        y1, y2 = min(V[0][1], V[1][1]), max(V[0][1], V[1][1])
        V = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    return V


def is_empty(C):
    return len(C) < 3 or not (max(p[0] for p in C) - min(p[0] for p in C) > 0) or not (max(p[1] for p in C) - min(p[1] for p in C) > 0)


def tile_polygon(V, a_img, cid, ox, oy, tw, th, min_visibility, mode):
    """V: vertices(); a_img: the image-clipped area -> None, or (written, cut, line or None)"""
    ox, oy, tw, th = float(ox), float(oy), float(tw), float(th)
    M = [(x - ox, y - oy) for x, y in V]
    C = S.clip(M, tw, th)
    if is_empty(C):
        return None
    if not A.area(C) >= min_visibility * a_img:
        return False, False, None
    cut = any(not (x >= 0.0 and x <= tw and y >= 0.0 and y <= th) for x, y in M)
    if mode == 0:
        line = f"{cid}" + "".join(f" {S.norm(x / tw):.6f} {S.norm(y / th):.6f}" for x, y in C)
    else:
        x1, x2 = min(p[0] for p in C), max(p[0] for p in C)
        y1, y2 = min(p[1] for p in C), max(p[1] for p in C)
        line = f"{cid} {(x1 + x2) / 2 / tw:.6f} {(y1 + y2) / 2 / th:.6f} {(x2 - x1) / tw:.6f} {(y2 - y1) / th:.6f}"
    return True, cut, line


def tile_arrays(xy, pt_off, row_off, cls, width, height, tile_w, tile_h, step_x, step_y, min_visibility=0.1, mode=0,
                max_tiles_per_row=4096):
    check_params(tile_w, tile_h, step_x, step_y, min_visibility, mode, max_tiles_per_row)
    xy = np.asarray(xy, np.float64).reshape(-1)
    n = len(row_off) - 1
    nb = int(row_off[-1]) if n else 0
    status, tile_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    action = np.full(nb, 255, np.uint8)
    written, cut, dropped = np.zeros(nb, np.int32), np.zeros(nb, np.int32), np.zeros(nb, np.int32)
    line_count, sizes, parts = [], [], []
    for i in range(n):
        W, H = float(width[i]), float(height[i])
        status[i], tiles = row_grid(W, H, tile_w, tile_h, step_x, step_y, max_tiles_per_row)
        tile_off[i + 1] = tile_off[i] + len(tiles)
        live = []                                        # (polygon, class id, V, A_img) of the written and clipped ones
        for b in range(int(row_off[i]), int(row_off[i + 1])):
            if cls[b] < 0:
                continue
            raw = [(float(xy[2 * k]), float(xy[2 * k + 1])) for k in range(int(pt_off[b]), int(pt_off[b + 1]))]
            act, _ = S.polygon(raw, S.size_of(W), S.size_of(H), 0)
            action[b] = S.ACTIONS.index(act)
            if action[b] <= 1:
                live.append((b, int(cls[b]), vertices(raw), A.area(A.clipped(vertices(raw), W, H))))
        for ox, oy, tw, th in tiles:
            lines = []
            for b, cid, V, a_img in live:
                res = tile_polygon(V, a_img, cid, ox, oy, tw, th, min_visibility, mode)
                if res is None:
                    continue
                if res[0]:
                    written[b] += 1
                    cut[b] += res[1]
                    lines.append(res[2])
                else:
                    dropped[b] += 1
            text = "\n".join(lines)
            line_count.append(len(lines))
            sizes.append(len(text))
            parts.append(text)
    text_off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=text_off[1:])
    return (status, tile_off, np.asarray(line_count, np.int32), text_off, action, written, cut, dropped,
            "".join(parts).encode("ascii"))


def tile_boxes(width, height, status, tile_w, tile_h, step_x, step_y, max_tiles_per_row=4096):
    """-> [(row, tile, x0, y0, w, h)] of every tile in order"""
    out = []
    for i in range(len(status)):
        st, tiles = row_grid(float(width[i]), float(height[i]), tile_w, tile_h, step_x, step_y, max_tiles_per_row)
        assert st == status[i]
        out += [(i, k, *t) for k, t in enumerate(tiles)]
    return out
