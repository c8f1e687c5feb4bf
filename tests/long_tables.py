"""A long sparse polygon table for the steps that share the polygon-table path (csrc/poly_table.h, k13_poly.h, k13_scan.h): K13,
K14, K16, K17, K20 and K21.  Thousands of rows, most without a polygon, one with hundreds, the last polygon behind about 2,000
empty rows: more than two parts of the scan over rows and over polygons, 256-polygon blocks that lie inside one row and blocks
that start after a long run of equal row_off entries, print windows that touch more than a thousand rows.
tests/test_long_tables_cpu.py holds the properties as assertions, tests/test_gpu_long_tables.py runs the steps.  No GPU."""
import functools

import numpy as np

import coco_ref
import polygon_audit_ref
import polygon_raster_ref
import tile_labels_ref
import yolo_obb_ref
import yolo_seg_ref

LENGTHS = (2, 3, 4, 7)


@functools.lru_cache(maxsize=None)
def long_sparse(seed=0, n=6000):
    """-> (xy f64 [2P], pt_off i32 [B+1], row_off i32 [n+1], W f64 [n], H f64 [n]); cached: the callers leave the arrays unchanged"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    W, H = 3.0 + i % 6, 2.0 + i % 5
    cw, ch = W.copy(), H.copy()                              # the polygons are placed by the sizes before they are spoilt
    W[5::97] = 0.0
    W[7::101] += 0.5
    H[11::103] = np.nan
    count = np.zeros(n, np.int64)
    count[1000:2000] = 2
    count[2003:4000:7] = 1
    count[2500] = 700
    count[n - 1] = 1
    row_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    nb = int(row_off[-1])
    row = np.repeat(i, count)
    lengths = np.asarray(LENGTHS)[np.arange(nb) % len(LENGTHS)]
    pt_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    owner = np.repeat(np.arange(nb), lengths)                # the polygon of every point
    centre = rng.uniform(0.0, 1.0, (nb, 2)) * np.stack([cw[row], ch[row]], axis=1)
    pts = centre[owner] + rng.uniform(-2.5, 2.5, (len(owner), 2))
    whole = owner % 3 == 0                                   # vertices on pixel corners and tile edges, repeated vertices
    pts[whole] = np.round(pts[whole])
    return pts.reshape(-1), pt_off, row_off, W, H


def size_status(W, H):
    """the size_status K14 and K16 take, as the size check of the audit steps reads numeric columns: 1 for a zero, 2 for another
    value that is no size"""
    missing = (W == 0) | (H == 0)
    ok = ~missing & np.isfinite(W) & np.isfinite(H) & (W > 0) & (H > 0)
    return np.where(missing, 1, np.where(ok, 0, 2)).astype(np.uint8)


# ---- the steps' columns on that table (polygon p, row i) ----------------------------------------------------------
def class_ids(n):
    return (np.arange(n) % 1200).astype(np.int32)            # one to four digits


def k13_sel(nb):
    return (np.arange(nb) % 5 != 0).astype(np.uint8)


def k14_cls(nb):
    return (np.arange(nb) % 5 - 1).astype(np.int32)          # -1: not matched; n_classes = 4


def k16_cat(nb):
    return np.maximum(np.arange(nb) % 5 - 1, 0).astype(np.int32)


def k21_val(nb):
    p = np.arange(nb)
    return np.where(p % 5 == 0, -1, 1 + p % 200).astype(np.int32)


def k20_cls(nb):
    p = np.arange(nb)
    return np.where(p % 5 == 0, -1, np.asarray((0, 10, 100))[p % 3]).astype(np.int32)


# ---- the steps' tables and the references' outputs on them, computed once ------------------------------------------
def k13_table(sel=False):
    xy, pt_off, row_off, W, H = long_sparse()
    return xy, pt_off, row_off, k13_sel(len(pt_off) - 1) if sel else None, W, H, class_ids(len(W))


def k14_table():
    xy, pt_off, row_off, W, H = long_sparse()
    return xy, pt_off, row_off, k14_cls(len(pt_off) - 1), W, H, size_status(W, H), 4


def k16_table():
    xy, pt_off, row_off, W, H = long_sparse()
    return xy, pt_off, row_off, k16_cat(len(pt_off) - 1), W, H, size_status(W, H)


def k20_table():
    xy, pt_off, row_off, W, H = long_sparse()
    return xy, pt_off, row_off, k20_cls(len(pt_off) - 1), W, H


def k20_params(mode=0, max_tiles_per_row=4096):
    return 2, 2, 1, 1, 0.1, mode, max_tiles_per_row          # tile 2 x 2, step 1 x 1: up to 7 x 5 tiles per row


def k21_table():
    xy, pt_off, row_off, W, H = long_sparse()
    return xy, pt_off, row_off, k21_val(len(pt_off) - 1), W, H


@functools.lru_cache(maxsize=None)
def k13_want(sel=False):
    return yolo_seg_ref.seg_arrays(*k13_table(sel))


@functools.lru_cache(maxsize=None)
def k17_want(sel=False):
    return yolo_obb_ref.obb_arrays(*k13_table(sel))


@functools.lru_cache(maxsize=None)
def k14_want():
    return polygon_audit_ref.audit_arrays(*k14_table())


@functools.lru_cache(maxsize=None)
def k16_want(flags=1):
    return coco_ref.coco_arrays(*k16_table(), 1, 1, flags)


@functools.lru_cache(maxsize=None)
def k20_want(mode=0, max_tiles_per_row=4096):
    return tile_labels_ref.tile_arrays(*k20_table(), *k20_params(mode, max_tiles_per_row))


@functools.lru_cache(maxsize=None)
def k21_want(max_pixels=1 << 20):
    return polygon_raster_ref.raster_arrays(*k21_table(), 9, max_pixels)
