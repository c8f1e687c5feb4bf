"""Table builders shared by tests/test_polygon_compare_cpu.py and tests/test_gpu_polygon_compare.py: the ten input arrays of K22 from
rows written out by hand, small shapes, and the random table both files compare on, with its expected outputs computed once."""
import functools
import math

import numpy as np

import polygon_compare_ref as R


def table(rows):
    """rows = [(W, H, [(cls, [(x, y)])] of A, the same of B)] -> the ten input arrays of the entries"""
    sides = []
    for k in (2, 3):
        xy, pt_off, row_off, cls = [], [0], [0], []
        for row in rows:
            for c, pts in row[k]:
                xy += [v for p in pts for v in p]
                pt_off.append(pt_off[-1] + len(pts))
                cls.append(c)
            row_off.append(len(cls))
        sides += [np.asarray(xy, np.float64), np.asarray(pt_off, np.int32), np.asarray(row_off, np.int32), np.asarray(cls, np.int32)]
    return (*sides, np.asarray([r[0] for r in rows], np.float64), np.asarray([r[1] for r in rows], np.float64))


def blob(rng, cx, cy, r, m):
    a = np.sort(rng.uniform(0, 2 * math.pi, m))
    rad = rng.uniform(0.4 * r, r, m)
    return [(cx + rr * math.cos(t), cy + rr * math.sin(t)) for t, rr in zip(a.tolist(), rad.tolist())]


def random_rows(seed, n_rows=40, max_polys=8, max_size=96, n_classes=3):
    """A as the raster test draws its rows; B from A: polygons dropped, jittered, relabelled, reordered and added"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n_rows):
        w, h = int(rng.integers(1, max_size + 1)), int(rng.integers(1, max_size + 1))
        wide = rng.random() < 0.2
        a = []
        for _ in range(int(rng.integers(0, max_polys + 1))):
            m = int(rng.integers(1, 46)) if rng.random() < 0.3 else int(rng.integers(2, 9))
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            r = rng.choice([4.0, 20.0, 90.0])
            pts = np.stack([cx + rng.uniform(-r, r, m), cy + rng.uniform(-r, r, m)], axis=1)
            if not wide:
                pts = np.clip(pts, 0, [w, h])
            kind = rng.random()
            if kind < 0.3:
                pts = np.round(pts)
            elif kind < 0.5:
                pts = np.round(pts) + 0.5
            if rng.random() < 0.03:
                pts[rng.integers(0, m), rng.integers(0, 2)] = rng.choice([np.nan, np.inf, 2.0 ** 43])
            if rng.random() < 0.04:
                pts = pts[:1]                                                 # too few points
            c = -1 if rng.random() < 0.1 else int(rng.integers(0, n_classes))
            a.append((c, [tuple(p) for p in pts.tolist()]))
        b = []
        for c, pts in a:
            u = rng.random()
            if u < 0.15:
                continue                                                      # dropped
            if u < 0.45:
                pts = [(x + rng.uniform(-1.5, 1.5), y + rng.uniform(-1.5, 1.5)) for x, y in pts]
            if u > 0.85 and c >= 0:
                c = (c + 1) % n_classes                                       # relabelled
            b.append((c, pts))
        if rng.random() < 0.3:
            b.append((int(rng.integers(0, n_classes)), blob(rng, rng.uniform(0, w), rng.uniform(0, h), 12, 6)))
        if rng.random() < 0.3:
            b = b[::-1]
        if i % 9 == 4:
            w = [0.0, w + 0.5, math.nan, 5000.0][(i // 9) % 4]                # rows of status 1, 2, 1, 3
        rows.append((w, h, a, b))
    return rows


@functools.lru_cache(maxsize=None)
def random_table(seed=5):
    return table(random_rows(seed))


RANDOM = dict(n_classes=3, max_pixels_per_row=96 * 96, max_pairs_per_row=48)


@functools.lru_cache(maxsize=None)
def random_want(thr=0.5, by_label=False):
    return R.compare_arrays(*random_table(), thr=thr, by_label=by_label, **RANDOM)


def box(x1, y1, x2, y2):
    return [(float(x1), float(y1)), (float(x2), float(y2))]
