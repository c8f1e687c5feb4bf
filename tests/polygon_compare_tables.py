"""Table builders shared by tests/test_polygon_compare_cpu.py and tests/test_gpu_polygon_compare.py: the ten input arrays of K22 from
rows written out by hand, small shapes, and the random table both files compare on, with its expected outputs computed once; and
the identities that tie K22's outputs to K21's masks of the same two tables, with the table both files check them on."""
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


def strip_rows(widths, h=5):
    rng = np.random.default_rng(31)
    rows = []
    for w in widths:
        a = [(0, blob(rng, w / 2, h / 2, w / 2 + 1, 9)), (1, box(w - 3, 0, w, h)), (2, box(-5, 1, w + 5, 2.2))]
        b = [(0, blob(rng, w / 2 + 1, h / 2, w / 2, 7)), (2, box(w - 4, 1, w - 1, h)), (1, box(0, 0, w, 1.7)), (1, box(60, 1, 70, 4))]
        rows.append((w, h, a, b))
    return rows


def comb(n_teeth):
    pts = [(0.0, 0.0)]
    for k in range(n_teeth):
        pts += [(3.0 * k + 0.5, 10.0), (3.0 * k + 1.5, 1.0), (3.0 * k + 2.5, 10.0)]
    return pts + [(3.0 * n_teeth + 5.0, 0.0)]


# ----------------------------------------------------------------------------------------------- K21 and K22 on the same tables
def shared_rows():
    """The smallest table that reaches what K21 and K22 share (csrc/k21_cover.h): strip edges at and around a wave with boxes
    that overhang the image; about 80 crossings per scanline; a two-point polygon per side (the synthetic corners); polygons of
    65 points (a second chunk of edges); unselected polygons; a row of fractional size between painted rows."""
    rng = np.random.default_rng(34)
    rows = strip_rows((63, 64, 65, 130))
    shifted = [(x + 1.0, y) for x, y in comb(40)]
    rows.append((125, 12, [(0, comb(40)), (1, box(3, 2, 90, 7))], [(0, shifted), (1, box(100, 9, 4, 1))]))
    rows.append((40.5, 30, [(2, box(0, 0, 5, 5))], [(2, box(0, 0, 5, 5))]))
    rows.append((40, 30, [(2, blob(rng, 20, 15, 18, 65)), (-1, box(0, 0, 40, 30)), (1, box(30, 2, 38, 20))],
                 [(2, blob(rng, 21, 15, 18, 65)), (1, box(29, 2, 38, 21)), (-1, blob(rng, 10, 10, 9, 5))]))
    return rows


@functools.lru_cache(maxsize=None)
def shared_table():
    return table(shared_rows())


@functools.lru_cache(maxsize=None)
def shared_want():
    """the restatements over shared_table(): K21's outputs over side A and over side B, K22's over both (3 classes)"""
    import polygon_raster_ref as RR

    t = shared_table()
    return RR.raster_arrays(*raster_side(t, 0)), RR.raster_arrays(*raster_side(t, 1)), R.compare_arrays(*t, 3)


def raster_side(t, k):
    """side k (0: A, 1: B) of a comparison as K21's six inputs, with val = cls + 1 (background 0) and unselected polygons kept
    unselected"""
    xy, pt_off, row_off, cls = t[4 * k:4 * k + 4]
    assert cls.max(initial=0) <= 254, "val must fit a byte"
    return xy, pt_off, row_off, np.where(cls >= 0, cls + 1, -1).astype(np.int32), t[8], t[9]


def assert_same_cover(t, mask_a, mask_b, cmp):
    """mask_a / mask_b: K21's six outputs over raster_side(t, 0 / 1) with background 0; cmp: K22's outputs over t, under the same
    max_pixels_per_row.  A row of pair status 4 is rasterised and not compared, so nothing is said about it."""
    status, row_pixels = cmp[0], cmp[14]
    rows = status != R.STATUS_PAIRS
    for mask, row_off, action, pixels in ((mask_a, t[2], cmp[2], cmp[4]), (mask_b, t[6], cmp[3], cmp[5])):
        polys = np.repeat(rows, np.diff(row_off))
        assert np.array_equal(mask[0][rows], status[rows]), "row_status"
        assert np.array_equal(mask[2][polys], action[polys]), "action"
        assert mask[3].dtype == pixels.dtype and np.array_equal(mask[3][polys], pixels[polys]), "covered against a_pixels / b_pixels"
    pix_off = mask_a[1]
    assert np.array_equal(pix_off, mask_b[1])
    want = np.zeros((len(status), 2), np.int64)
    for r in np.flatnonzero(status == 0):
        ma, mb = mask_a[5][pix_off[r]:pix_off[r + 1]], mask_b[5][pix_off[r]:pix_off[r + 1]]
        want[r] = ((ma == mb) & (ma != 0)).sum(), ((ma != 0) | (mb != 0)).sum()
    assert row_pixels.dtype == want.dtype and np.array_equal(row_pixels, want), "row_pixels"
