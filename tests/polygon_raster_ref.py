"""The K21 rule (include/dyd.h: label masks from the annotation polygons) restated in numpy, per polygon and edge over the whole
pixel grid, in the same f64 operations (numpy does not contract them).  It produces every output of the entry; the GPU tests and
the fake backend of the CPU tests compare against it.  exact_cover is the same rule in fractions.Fraction, for the tests of the
rule itself."""
from fractions import Fraction

import numpy as np

LIMIT = float(1 << 43)
ACT_DONE, ACT_BAD, ACT_FEW, ACT_NO_RASTER, ACT_UNSELECTED = 0, 2, 3, 5, 255


def row_size(W, H, max_pixels):
    """-> (status, width, height) of one row, the sizes as ints (0 unless status is 0)"""
    if not (0.0 < W < LIMIT) or not (0.0 < H < LIMIT):
        return 1, 0, 0
    if W != np.floor(W) or H != np.floor(H):
        return 2, 0, 0
    w, h = int(W), int(H)
    if w > max_pixels or h > max_pixels or w * h > max_pixels:
        return 3, 0, 0
    return 0, w, h


def vertices(pts):
    """K13's vertex list: the points, or for exactly two points the four corners of their box"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    if len(pts) == 2:
        x1, y1, x2, y2 = pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()
        return np.array([(x1, y1), (x2, y1), (x2, y2), (x1, y2)])
    return pts


def canonical(A, B):
    return (B, A) if A[1] > B[1] or (A[1] == B[1] and A[0] > B[0]) else (A, B)


def cover(pts, w, h):
    """bool [h, w]: the pixels the polygon of these points covers"""
    V = vertices(pts)
    xc, yc = np.arange(w, dtype=np.float64) + 0.5, np.arange(h, dtype=np.float64) + 0.5
    par = np.zeros((h, w), bool)
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
    return par


def exact_cover(pts, w, h):
    """cover() in exact rational arithmetic (coordinates must be exactly representable, which every float is)"""
    V = [(Fraction(float(x)), Fraction(float(y))) for x, y in vertices(pts)]
    par = np.zeros((h, w), bool)
    half = Fraction(1, 2)
    for k in range(len(V)):
        P, Q = canonical(V[k], V[(k + 1) % len(V)])
        if P[1] == Q[1]:
            continue
        for j in range(h):
            yc = j + half
            if P[1] <= yc < Q[1]:
                xs = P[0] + (yc - P[1]) * (Q[0] - P[0]) / (Q[1] - P[1])
                for i in range(w):
                    if xs > i + half:
                        par[j, i] ^= True
    return par


def raster_arrays(xy, pt_off, row_off, val, width, height, background=0, max_pixels_per_row=1 << 26):
    """-> (row_status u8 [n], pix_off i64 [n+1], action u8 [B], covered i64 [B], owned i64 [B], pixels u8 [total])"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pt_off, row_off, val = np.asarray(pt_off, np.int64), np.asarray(row_off, np.int64), np.asarray(val, np.int64)
    W, H = np.asarray(width, np.float64), np.asarray(height, np.float64)
    n, nb = len(W), len(val)
    status, pix_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    action = np.full(nb, ACT_UNSELECTED, np.uint8)
    covered, owned = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    masks = []
    for i in range(n):
        status[i], w, h = row_size(W[i], H[i], max_pixels_per_row)
        pix_off[i + 1] = pix_off[i] + w * h
        own = np.full((h, w), -1, np.int64)
        for p in range(row_off[i], row_off[i + 1]):
            pts = xy[pt_off[p]:pt_off[p + 1]]
            if val[p] < 0:
                continue
            if status[i] != 0:
                action[p] = ACT_NO_RASTER
            elif not (np.abs(pts) < LIMIT).all():          # NaN and inf fail too
                action[p] = ACT_BAD
            elif len(pts) < 2:
                action[p] = ACT_FEW
            else:
                action[p] = ACT_DONE
                c = cover(pts, w, h)
                covered[p] = int(c.sum())
                own[c] = p
        if w * h:
            painted = own >= 0
            owned += np.bincount(own[painted], minlength=nb)[:nb] if nb else 0
            masks.append(np.where(painted, val[np.maximum(own, 0)] if nb else 0, background).astype(np.uint8).reshape(-1))
    pixels = np.concatenate(masks) if masks else np.zeros(0, np.uint8)
    return status, pix_off, action, covered, owned, pixels


def paint_by_items(xy, pt_off, row_off, val, width, height, background=0, max_pixels_per_row=1 << 26, strip=1024, capacity=256):
    """The same outputs by K21's mapping instead of by the rule: items of (row, scanline, strip), per item the row's
    polygons in order culled by their box, edges in chunks of 64 whose crossings go through a list of `capacity` entries that is
    applied and emptied when full, ownership handed over per polygon with the counters adjusted.  It shows that the strips, the
    cull and the list change nothing; it is not another definition."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pt_off, row_off, val = np.asarray(pt_off, np.int64), np.asarray(row_off, np.int64), np.asarray(val, np.int64)
    status, pix_off, action, _, _, _ = raster_arrays(xy, pt_off, row_off, np.where(val < 0, -1, 0), width, height, 0, max_pixels_per_row)
    action = np.where(val < 0, ACT_UNSELECTED, action).astype(np.uint8)
    nb = len(val)
    covered, owned = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    pixels = np.zeros(pix_off[-1], np.uint8)
    for r in np.flatnonzero(status == 0):
        w, h = int(width[r]), int(height[r])
        for j in range(h):
            for x0 in range(0, w, strip):
                npx = min(strip, w - x0)
                xc = x0 + np.arange(npx, dtype=np.float64) + 0.5
                yc = j + 0.5
                owner, parity = np.full(npx, -1, np.int64), np.zeros(npx, bool)
                for p in range(row_off[r], row_off[r + 1]):
                    if action[p] != ACT_DONE:
                        continue
                    pts = xy[pt_off[p]:pt_off[p + 1]]
                    bx1, by1, bx2, by2 = pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()
                    if not by1 <= yc or not yc < by2 or xc[0] >= bx2 + 1.0 or xc[-1] <= bx1 - 1.0:
                        continue
                    V = vertices(pts)
                    listed = []
                    for k0 in range(0, len(V), 64):
                        for k in range(k0, min(k0 + 64, len(V))):
                            P, Q = canonical(V[k], V[(k + 1) % len(V)])
                            if P[1] != Q[1] and P[1] <= yc < Q[1]:
                                listed.append(P[0] + ((yc - P[1]) * (Q[0] - P[0])) / (Q[1] - P[1]))
                                if len(listed) == capacity:
                                    for xs in listed:
                                        parity ^= xs > xc
                                    listed = []
                    for xs in listed:
                        parity ^= xs > xc
                    old = owner[parity]
                    np.subtract.at(owned, old[old >= 0], 1)
                    covered[p] += parity.sum()
                    owned[p] += parity.sum()
                    owner[parity] = p
                    parity[:] = False
                at = pix_off[r] + j * w + x0
                pixels[at:at + npx] = np.where(owner >= 0, val[np.maximum(owner, 0)] if nb else 0, background)
    return status, pix_off, action, covered, owned, pixels
