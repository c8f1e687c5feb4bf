"""The COCO annotation objects (K16) restated from their definition (include/dyd.h), for tests/test_coco_cpu.py
and tests/test_gpu_coco.py.  The action is K13's as yolo_seg_ref computes it, the clipped vertices and the area are
polygon_audit_ref's; every number is Python's own "%.2f".

- ``fix2(v)``: the definition's rounding rule, step by step (math.fma where Python has it, else exact integers);
- ``polygon(raw, W, H, ann, img, cat, segmentation)``: (action code, text or None, area) of one selected polygon;
- ``coco_arrays``: what K16 computes from the arrays -> (action, area, row_kept, text).
"""
import math
from fractions import Fraction

import numpy as np

import polygon_audit_ref as R
import yolo_seg_ref as S

ACTIONS = (*S.ACTIONS, "too_large")
TOO_LARGE = 6
UNSELECTED = 255
LIMIT = float(2 ** 43)
SEGMENTATION = 1
ID_LIMIT = 2 ** 53


def fix2(v):
    """the definition's computation of "%.2f" % v for 0 <= v < 2^43 (e = fma(v, 100, -t), here from exact integers)"""
    t = v * 100.0
    e = Fraction(v) * 100 - Fraction(t)                     # what fma(v, 100.0, -t) returns: the product's rounding error, exact
    n = int(t)
    f = t - float(n)
    if f > 0.5 or (f == 0.5 and (e > 0 or (e == 0 and n % 2 == 1))):
        n += 1
    return f"{n // 100}.{n % 100:02d}"


def clamp(v, hi):
    return 0.0 if not v > 0.0 else (hi if v > hi else v)


def polygon(raw, W, H, ann, img, cat, segmentation=True):
    """raw: [(x, y)] floats as K13 reads them; W, H usable sizes or None -> (action code, text or None, area or NaN)"""
    act, _ = S.polygon(raw, W, H, 0)
    code = S.ACTIONS.index(act)
    if code > 1:
        return code, None, math.nan
    C = R.clipped([(float(x), float(y)) for x, y in raw], W, H)
    area = R.area(C)
    if not area < LIMIT:
        return TOO_LARGE, None, math.nan
    Pc = [(clamp(x, W), clamp(y, H)) for x, y in C]
    bx, by = min(p[0] for p in Pc), min(p[1] for p in Pc)
    bw, bh = max(p[0] for p in Pc) - bx, max(p[1] for p in Pc) - by
    seg = "[" + ",".join("%.2f,%.2f" % p for p in Pc) + "]" if segmentation else ""
    text = ('{"id":%d,"image_id":%d,"category_id":%d,"bbox":[%.2f,%.2f,%.2f,%.2f],"area":%.2f,"iscrowd":0,"segmentation":[%s]}'
            % (ann, img, cat, bx, by, bw, bh, area, seg))
    return code, text, area


def coco_arrays(xy, pt_off, row_off, cat_id, width, height, status, image_id_base=1, ann_id_base=1, flags=SEGMENTATION):
    """K16 on arrays -> (action u8 [B], area f64 [B], row_kept i32 [n], text bytes)"""
    if image_id_base < 0 or ann_id_base < 0:
        raise ValueError("negative id base")
    xy = np.asarray(xy, np.float64).reshape(-1)
    n, nb = len(row_off) - 1, int(row_off[-1]) if len(row_off) > 1 else 0
    if image_id_base + n >= ID_LIMIT or ann_id_base + nb >= ID_LIMIT:
        raise ValueError("ids reach 2^53")
    action, area = np.full(nb, UNSELECTED, np.uint8), np.full(nb, np.nan)
    kept = np.zeros(n, np.int32)
    parts = []
    for i in range(n):
        ok = int(status[i]) == 0
        W, H = (S.size_of(float(width[i])), S.size_of(float(height[i]))) if ok else (None, None)
        for p in range(int(row_off[i]), int(row_off[i + 1])):
            cat = int(cat_id[p])
            if cat <= 0:
                continue
            raw = [(float(xy[2 * k]), float(xy[2 * k + 1])) for k in range(int(pt_off[p]), int(pt_off[p + 1]))]
            code, text, a = polygon(raw, W, H, ann_id_base + p, image_id_base + i, cat, bool(flags & SEGMENTATION))
            action[p], area[p] = code, a
            if text is not None:
                parts.append(text)
                kept[i] += 1
    return action, area, kept, ",".join(parts).encode("ascii")
