"""The K23 rule (include/dyd.h: COCO run-length masks from the annotation polygons) restated in numpy.  Coverage is K21's rule
(polygon_raster_ref: vertices, canonical, the same f64 operations), evaluated over the polygon's own box of columns and lines
only, so that an image of 2^30 pixels costs what its polygons cover; runs are the differences of the transition indices in
column-major order; the string is COCO's rleToString, written here once more, with its inverse.  It produces every output of
the entry; the GPU tests and the fake backend of the CPU tests compare against it."""
import math

import numpy as np

from polygon_raster_ref import ACT_BAD, ACT_DONE, ACT_FEW, ACT_NO_RASTER, ACT_UNSELECTED, LIMIT, canonical, row_size, vertices


# ---- the string -------------------------------------------------------------------------------------------------------
def enc(runs) -> bytes:
    """COCO's rleToString"""
    runs = [int(v) for v in runs]
    out = bytearray()
    for i, c in enumerate(runs):
        x = c - runs[i - 2] if i > 2 else c
        while True:
            b = x & 0x1f
            x >>= 5
            more = (x != -1) if (b & 0x10) else (x != 0)
            if more:
                b |= 0x20
            out.append(b + 48)
            if not more:
                break
    return bytes(out)


def dec(text) -> list:
    """COCO's rleFrString"""
    text = text.encode("ascii") if isinstance(text, str) else bytes(text)
    runs, at = [], 0
    while at < len(text):
        x, k = 0, 0
        while True:
            c = text[at] - 48
            x |= (c & 0x1f) << (5 * k)
            at += 1
            k += 1
            if not c & 0x20:
                if c & 0x10:
                    x |= -1 << (5 * k)
                break
        if len(runs) > 2:
            x += runs[-2]
        runs.append(x)
    return runs


def decode(runs, w, h) -> np.ndarray:
    """runs -> bool [h, w]"""
    runs = np.asarray(runs, np.int64)
    assert int(runs.sum()) == w * h and (runs >= 0).all()
    return np.repeat((np.arange(len(runs)) & 1).astype(bool), runs).reshape(w, h).T


# ---- coverage over the box ----------------------------------------------------------------------------------------------
def box_cover(pts, w, h):
    """-> (x0, y0, sub): sub (bool [lines, columns]) holds the rule's coverage of the columns x0.. and lines y0.. that the box
    of the points can reach; every pixel of the image outside of it is not covered.  No edge crosses a line unless min y <= yc <
    max y, and every crossing lies within [min x, max x] up to rounding, so a column a whole pixel outside has parity 0 (to the
    right no crossing exceeds xc; to the left all do, and their number is even)."""
    V = vertices(pts)
    bx1, by1, bx2, by2 = V[:, 0].min(), V[:, 1].min(), V[:, 0].max(), V[:, 1].max()
    x0, x1 = int(min(max(math.floor(bx1) - 1, 0), w)), int(min(max(math.ceil(bx2) + 1, 0), w))
    y0, y1 = int(min(max(math.floor(by1) - 1, 0), h)), int(min(max(math.ceil(by2) + 1, 0), h))
    if x1 <= x0 or y1 <= y0:
        return 0, 0, np.zeros((0, 0), bool)
    xc, yc = np.arange(x0, x1, dtype=np.float64) + 0.5, np.arange(y0, y1, dtype=np.float64) + 0.5
    par = np.zeros((len(yc), len(xc)), bool)
    for k in range(len(V)):
        P, Q = canonical(V[k], V[(k + 1) % len(V)])
        if P[1] == Q[1]:
            continue
        rows = np.flatnonzero((P[1] <= yc) & (yc < Q[1]))
        if not len(rows):
            continue
        t = yc[rows] - P[1]
        d = Q[0] - P[0]
        n = t * d
        q = n / (Q[1] - P[1])
        xs = P[0] + q
        par[rows] ^= xs[:, None] > xc[None, :]
    return x0, y0, par


def box_cover_full(pts, w, h) -> np.ndarray:
    """box_cover placed into the whole image (small images only)"""
    x0, y0, sub = box_cover(pts, w, h)
    full = np.zeros((h, w), bool)
    full[y0:y0 + sub.shape[0], x0:x0 + sub.shape[1]] = sub
    return full


def polygon_runs(pts, w, h):
    """-> (runs [int], area, (x, y, bw, bh)) of one polygon of action 0.  Per box column the stretches of covered lines are
    intervals of the column-major index k = i * h + j; an interval that ends where the next begins (the bottom of one column,
    the top of the next) is the same run; the bounds of the merged intervals are the transitions, but for the image's end."""
    x0, y0, sub = box_cover(pts, w, h)
    bounds = []                                            # the merged intervals' bounds, flat and ascending
    for c in range(sub.shape[1]):
        col = np.concatenate([[False], sub[:, c], [False]]).astype(np.int8)
        edges = np.flatnonzero(np.diff(col) != 0) + (x0 + c) * h + y0      # begin, end, begin, end ...
        for a, b in zip(edges[0::2].tolist(), edges[1::2].tolist()):
            if bounds and bounds[-1] == a:
                bounds[-1] = b
            else:
                bounds += [a, b]
    if bounds and bounds[-1] == w * h:
        bounds.pop()
    runs = np.diff(np.asarray([0] + bounds + [w * h], np.int64)).tolist()
    ys, xs = np.nonzero(sub)
    area = int(sub.sum())
    box = (int(x0 + xs.min()), int(y0 + ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)) if area else (0, 0, 0, 0)
    return runs, area, box


def rle_arrays(xy, pt_off, row_off, sel, width, height, max_pixels_per_row=1 << 26):
    """-> (row_status u8 [n], action u8 [B], area i64 [B], bbox i32 [B, 4], run_off i64 [B+1], runs u32, text_off i64 [B+1],
    text bytes)"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pt_off, row_off, sel = np.asarray(pt_off, np.int64), np.asarray(row_off, np.int64), np.asarray(sel, np.int64)
    W, H = np.asarray(width, np.float64), np.asarray(height, np.float64)
    n, nb = len(W), len(sel)
    status = np.zeros(n, np.uint8)
    action = np.full(nb, ACT_UNSELECTED, np.uint8)
    area, bbox = np.zeros(nb, np.int64), np.zeros((nb, 4), np.int32)
    run_off, text_off = np.zeros(nb + 1, np.int64), np.zeros(nb + 1, np.int64)
    all_runs, texts = [], []
    for i in range(n):
        status[i], w, h = row_size(W[i], H[i], max_pixels_per_row)
        for p in range(row_off[i], row_off[i + 1]):
            pts = xy[pt_off[p]:pt_off[p + 1]]
            runs, text = [], b""
            if sel[p] < 0:
                pass
            elif status[i] != 0:
                action[p] = ACT_NO_RASTER
            elif not (np.abs(pts) < LIMIT).all():          # NaN and inf fail too
                action[p] = ACT_BAD
            elif len(pts) < 2:
                action[p] = ACT_FEW
            else:
                action[p] = ACT_DONE
                runs, area[p], bbox[p] = polygon_runs(pts, w, h)
                text = enc(runs)
            all_runs.extend(runs)
            texts.append(text)
            run_off[p + 1] = run_off[p] + len(runs)
            text_off[p + 1] = text_off[p] + len(text)
    return status, action, area, bbox, run_off, np.asarray(all_runs, np.uint32), text_off, b"".join(texts)


def runs_by_items(pts, w, h, strip=1024, capacity=256, band=64):
    """The runs of one polygon of action 0 by K23's mapping instead of by the rule: the reach [c0, c1) x [j0, j1) from
    the box of the points, items of `strip` columns by `band` lines, every item walked top to bottom after the line before it,
    crossings through a list of `capacity` entries, the transitions counted per column and band, a column's top judged
    afterwards against the bottom of the column to its left (nothing before the reach), a column's transitions placed band
    after band.  It shows that the reach, the strips, the bands, the list and the continuation change nothing; it is not
    another definition."""
    V = vertices(pts)
    P = np.asarray(pts, np.float64).reshape(-1, 2)
    bx1, by1, bx2, by2 = P[:, 0].min(), P[:, 1].min(), P[:, 0].max(), P[:, 1].max()
    clamp = lambda v, hi: int(min(max(v, 0), hi))          # noqa: E731
    c0, c1 = clamp(math.floor(bx1 - 1.5) + 1, w), clamp(math.ceil(bx2 + 0.5) + 1, w)
    j0, j1 = clamp(math.ceil(by1 - 0.5), h), clamp(math.ceil(by2 - 0.5), h)

    def line(j, xc):
        yc, par, listed = j + 0.5, np.zeros(len(xc), bool), []
        for k in range(len(V)):
            A, B = canonical(V[k], V[(k + 1) % len(V)])
            if A[1] != B[1] and A[1] <= yc < B[1]:
                listed.append(A[0] + ((yc - A[1]) * (B[0] - A[0])) / (B[1] - A[1]))
                if len(listed) == capacity:
                    for xs in listed:
                        par ^= xs > xc
                    listed = []
        for xs in listed:
            par ^= xs > xc
        return par

    trans = []
    if c1 > c0 and j1 > j0:
        cols = c1 - c0
        top, bot = np.zeros(cols, bool), np.zeros(cols, bool)
        found = [[] for _ in range(cols)]                   # per column, band after band
        for x0 in range(c0, c1, strip):
            npx = min(strip, c1 - x0)
            xc = x0 + np.arange(npx) + 0.5
            for ja in range(j0, j1, band):
                jb, first, last = min(ja + band, j1), ja == j0, ja + band >= j1
                prev = np.zeros(npx, bool) if first else line(ja - 1, xc)
                for j in range(ja, jb):
                    cur = line(j, xc)
                    if j == 0:
                        top[x0 - c0:x0 - c0 + npx] = cur
                    else:
                        for lane in np.flatnonzero(cur != prev).tolist():
                            found[x0 - c0 + lane].append((x0 + lane) * h + j)
                    prev = cur
                if last and j1 < h:
                    for lane in np.flatnonzero(prev).tolist():
                        found[x0 - c0 + lane].append((x0 + lane) * h + j1)
                if last and j1 == h:
                    bot[x0 - c0:x0 - c0 + npx] = prev
        for ci in range(cols):
            left = bot[ci - 1] if ci else False
            trans += ([(c0 + ci) * h] if left != top[ci] else []) + found[ci]
    return np.diff(np.asarray([0] + trans + [w * h], np.int64)).tolist()
