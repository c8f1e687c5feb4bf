"""Restatement of the box comparison (K18, core/processor.py: compare_boxes_*) for the tests.

- ``compare_rows``: the seven outputs of the kernel from two box tables, numpy, vectorised over the A boxes per B box, with
  np.where compare / selects in the reference's operand order (reference core/processor.py:328-339, :359-362).
- ``compare_rows_py``: the same in scalar pure Python on plain floats (the builtins max / min, as the reference calls them).
- ``expected_comparison``: cells -> everything compare_boxes_cells returns, through CPython's json and
  utils._extract_boxes_with_labels.
"""
import json

import numpy as np
import pandas as pd

from deal_yolo_daya_amd.core.utils import _extract_boxes_with_labels

HIST_BINS = 20
NONE = "(none)"
KINDS = ("missing", "extra", "relabelled")


def _normalise(box4):
    """extract_boxes :359-362: min / max of the two stored points, first argument unless the second is strictly better"""
    b = np.asarray(box4, np.float64).reshape(-1, 4)
    p1x, p1y, p2x, p2y = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([np.where(p2x < p1x, p2x, p1x), np.where(p2y < p1y, p2y, p1y),
                     np.where(p2x > p1x, p2x, p1x), np.where(p2y > p1y, p2y, p1y)], axis=1)


def _iou_block(a, b):
    """calculate_iou(a_i, b_j) for the normalised boxes a [na, 4] and b [nb, 4] -> [na, nb]"""
    a, b = a[:, None, :], b[None, :, :]
    with np.errstate(all="ignore"):
        ix1 = np.where(b[..., 0] > a[..., 0], b[..., 0], a[..., 0])
        iy1 = np.where(b[..., 1] > a[..., 1], b[..., 1], a[..., 1])
        ix2 = np.where(b[..., 2] < a[..., 2], b[..., 2], a[..., 2])
        iy2 = np.where(b[..., 3] < a[..., 3], b[..., 3], a[..., 3])
        w, h = ix2 - ix1, iy2 - iy1
        w, h = np.where(w > 0, w, 0.0), np.where(h > 0, h, 0.0)
        inter = w * h
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        uni = area_a + area_b - inter
        return np.where(inter == 0, 0.0, np.where(uni != 0, inter / np.where(uni != 0, uni, 1.0), 0.0))


_BLOCK = 1 << 20          # IoUs held at a time: a long row is taken in blocks of B boxes


def compare_rows(a_box4, a_off, a_cls, b_box4, b_off, b_cls, n_classes, thr, by_label):
    """-> (a_match i32, b_match i32, b_iou f64, a_best f64, b_best f64, row_counts [N, 4] i32, confusion [C+1, C+1] u64).
    Per row the IoUs come from np.where compare / selects over all A boxes at once; the B boxes are then taken one by one."""
    A, B = _normalise(a_box4), _normalise(b_box4)
    a_off, b_off = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
    a_cls, b_cls = np.asarray(a_cls, np.int64), np.asarray(b_cls, np.int64)
    n, C = len(a_off) - 1, int(n_classes)
    a_match, a_best = np.full(len(A), -1, np.int32), np.zeros(len(A))
    b_match, b_iou, b_best = np.full(len(B), -1, np.int32), np.zeros(len(B)), np.zeros(len(B))
    for r in range(n):
        a0, a1, b0, b1 = a_off[r], a_off[r + 1], b_off[r], b_off[r + 1]
        if a1 == a0 or b1 == b0:
            continue
        a, ac = A[a0:a1], a_cls[a0:a1]
        free = np.ones(a1 - a0, bool)
        step = max(1, _BLOCK // (a1 - a0))
        for j0 in range(b0, b1, step):
            j1 = min(b1, j0 + step)
            iou = _iou_block(a, B[j0:j1])
            with np.errstate(invalid="ignore"):
                pos = np.where(iou > 0, iou, 0.0)            # `iou > best` from 0.0: a NaN never raises the maximum
                ok = iou >= thr
            a_best[a0:a1] = np.where(pos.max(axis=1) > a_best[a0:a1], pos.max(axis=1), a_best[a0:a1])
            b_best[j0:j1] = pos.max(axis=0)
            if by_label:
                ok &= ac[:, None] == b_cls[None, j0:j1]
            for j in range(j0, j1):
                idx = np.flatnonzero(free & ok[:, j - j0])
                if len(idx):
                    i = idx[np.argmax(iou[idx, j - j0])]     # the first of equal maxima: the lowest index
                    free[i] = False
                    a_match[a0 + i] = j - b0
                    b_match[j], b_iou[j] = i, iou[i, j - j0]
    row_a = np.repeat(np.arange(n), np.diff(a_off))
    row_b = np.repeat(np.arange(n), np.diff(b_off))
    hit = np.flatnonzero(b_match >= 0)
    hit_a = a_off[row_b[hit]] + b_match[hit]
    same = a_cls[hit_a] == b_cls[hit]
    rows = np.zeros((n, 4), np.int64)
    np.add.at(rows[:, 0], row_b[hit[same]], 1)
    np.add.at(rows[:, 1], row_b[hit[~same]], 1)
    np.add.at(rows[:, 2], row_a[a_match < 0], 1)
    np.add.at(rows[:, 3], row_b[b_match < 0], 1)
    conf = np.zeros((C + 1, C + 1), np.int64)
    np.add.at(conf, (a_cls[hit_a], b_cls[hit]), 1)
    np.add.at(conf, (a_cls[a_match < 0], C), 1)
    np.add.at(conf, (C, b_cls[b_match < 0]), 1)
    return a_match, b_match, b_iou, a_best, b_best, rows.astype(np.int32), conf.astype(np.uint64)


def _iou_py(box1, box2):
    """reference core/processor.py:328-339, word for word"""
    x1_inter = max(box1[0], box2[0])
    y1_inter = max(box1[1], box2[1])
    x2_inter = min(box1[2], box2[2])
    y2_inter = min(box1[3], box2[3])
    intersection = max(0, x2_inter - x1_inter) * max(0, y2_inter - y1_inter)
    if intersection == 0:
        return 0.0
    area1 = (box1[2] - box1[0]) * (box1[3] - box1[1])
    area2 = (box2[2] - box2[0]) * (box2[3] - box2[1])
    union = area1 + area2 - intersection
    return intersection / union if union != 0 else 0.0


def _normalise_py(b):
    return (min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3]))


def compare_rows_py(a_box4, a_off, a_cls, b_box4, b_off, b_cls, n_classes, thr, by_label):
    """compare_rows in scalar Python on plain floats -> the same seven outputs as lists (confusion as a list of rows)"""
    A = [_normalise_py([float(v) for v in b]) for b in np.asarray(a_box4, np.float64).reshape(-1, 4).tolist()]
    B = [_normalise_py([float(v) for v in b]) for b in np.asarray(b_box4, np.float64).reshape(-1, 4).tolist()]
    a_off, b_off = [int(v) for v in a_off], [int(v) for v in b_off]
    a_cls, b_cls = [int(v) for v in a_cls], [int(v) for v in b_cls]
    C, thr = int(n_classes), float(thr)
    a_match, a_best = [-1] * len(A), [0.0] * len(A)
    b_match, b_iou, b_best = [-1] * len(B), [0.0] * len(B), [0.0] * len(B)
    rows, conf = [], [[0] * (C + 1) for _ in range(C + 1)]
    for r in range(len(a_off) - 1):
        a0, a1, b0, b1 = a_off[r], a_off[r + 1], b_off[r], b_off[r + 1]
        taken = set()
        counts = [0, 0, 0, 0]
        for j in range(b0, b1):
            pick, pick_iou = -1, 0.0
            for i in range(a0, a1):
                iou = _iou_py(A[i], B[j])
                if iou > a_best[i]:
                    a_best[i] = iou
                if iou > b_best[j]:
                    b_best[j] = iou
                if i in taken or (by_label and a_cls[i] != b_cls[j]) or not iou >= thr:
                    continue
                if pick < 0 or iou > pick_iou:
                    pick, pick_iou = i, iou
            if pick >= 0:
                taken.add(pick)
                b_match[j], b_iou[j], a_match[pick] = pick - a0, pick_iou, j - b0
                conf[a_cls[pick]][b_cls[j]] += 1
                counts[0 if a_cls[pick] == b_cls[j] else 1] += 1
            else:
                conf[C][b_cls[j]] += 1
                counts[3] += 1
        for i in range(a0, a1):
            if i not in taken:
                conf[a_cls[i]][C] += 1
                counts[2] += 1
        rows.append(counts)
    return a_match, b_match, b_iou, a_best, b_best, rows, conf


def same_outputs(got, want, what=""):
    """the seven outputs equal, floats bit for bit up to the sign of a zero (all are integers or exact f64)"""
    names = ("a_match", "b_match", "b_iou", "a_best", "b_best", "row_counts", "confusion")
    for nm, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.size == w.size, f"{what} {nm}: {g.shape} against {w.shape}"
        if g.size:
            bad = np.flatnonzero(~(g.reshape(-1) == w.reshape(g.shape).reshape(-1)))
            assert len(bad) == 0, f"{what} {nm}: {len(bad)} differ, first at {bad[0]}: {g.reshape(-1)[bad[0]]} != {w.reshape(-1)[bad[0]]}"


# ------------------------------------------------------------------------------------------------ cells -> BoxComparison
def _number(v):
    if isinstance(v, bool) or isinstance(v, (int, float)):
        try:
            return float(v)
        except OverflowError:
            return float("inf")
    return float("nan")


def _cell_boxes(cell):
    """[(object index, name, x1, y1, x2, y2 as floats)] of one cell: utils._extract_boxes_with_labels with the index of each
    box's object, found by the same walk over json.loads(cell)"""
    boxes = _extract_boxes_with_labels(cell)
    if not boxes:
        return []
    idx = []
    for k, obj in enumerate(json.loads(cell).get("objects", [])):
        if len(idx) == len(boxes):
            break
        if not isinstance(obj, dict) or not obj.get("name"):
            continue
        points = obj.get("polygon", {}).get("ptList", [])
        if not points:
            continue
        dict_points = [pt for pt in points if isinstance(pt, dict)]
        if [pt for pt in dict_points if "x" in pt] and [pt for pt in dict_points if "y" in pt]:
            idx.append(k)
    assert len(idx) == len(boxes)
    return [(k, b[0], *(_number(v) for v in b[1:])) for k, b in zip(idx, boxes)]


def expected_comparison(cells_a, cells_b, iou_threshold=0.5, by_label=False, sources=None):
    """-> dict(classes, confusion, per_class, hist_iou, per_row, differences, totals) as compare_boxes_cells builds them"""
    n = len(cells_a)
    assert len(cells_b) == n
    rows_a, rows_b = [_cell_boxes(c) for c in cells_a], [_cell_boxes(c) for c in cells_b]
    names = {b[1] for row in rows_a + rows_b for b in row if isinstance(b[1], str)}
    odd = any(not isinstance(b[1], str) for row in rows_a + rows_b for b in row)
    classes = sorted(names) + ([None] if odd else [])
    cid = {c: k for k, c in enumerate(classes)}
    C = len(classes)

    def table(rows):
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        flat = [b for r in rows for b in r]
        return (np.asarray([b[2:] for b in flat], np.float64).reshape(-1, 4), off,
                np.asarray([cid[b[1] if isinstance(b[1], str) else None] for b in flat], np.int64), flat)

    box_a, off_a, cls_a, flat_a = table(rows_a)
    box_b, off_b, cls_b, flat_b = table(rows_b)
    a_match, b_match, b_iou, a_best, b_best, rc, conf = compare_rows(box_a, off_a, cls_a, box_b, off_b, cls_b, C, iou_threshold,
                                                                     by_label)
    conf = conf.astype(np.int64)
    hist = np.zeros((C, HIST_BINS), np.int64)
    diffs = []
    nan4 = [float("nan")] * 4
    for r in range(n):
        lines = []
        for i in range(off_a[r], off_a[r + 1]):
            if a_match[i] < 0:
                lines.append((0, i - off_a[r], flat_a[i][0], -1, flat_a[i][1], None, 0.0, a_best[i], *box_a[i], *nan4))
        for j in range(off_b[r], off_b[r + 1]):
            if b_match[j] < 0:
                lines.append((1, j - off_b[r], -1, flat_b[j][0], None, flat_b[j][1], 0.0, b_best[j], *nan4, *box_b[j]))
                continue
            i = off_a[r] + b_match[j]
            if cls_a[i] == cls_b[j]:
                hist[cls_b[j], min(int(b_iou[j] * HIST_BINS), HIST_BINS - 1)] += 1
            else:
                lines.append((2, b_match[j], flat_a[i][0], flat_b[j][0], flat_a[i][1], flat_b[j][1], b_iou[j], b_iou[j],
                              *box_a[i], *box_b[j]))
        for kind, _, *rest in sorted(lines, key=lambda t: t[:2]):
            diffs.append((r, *((sources[r],) if sources is not None else ()), KINDS[kind], *rest))
    cols = ["row", *(("source",) if sources is not None else ()), "kind", "a_object", "b_object", "a_name", "b_name", "iou",
            "best_iou", "ax1", "ay1", "ax2", "ay2", "bx1", "by1", "bx2", "by2"]
    differences = pd.DataFrame(diffs, columns=cols)
    labels = classes + [NONE]
    pairs = conf[:C, :C]
    agree = np.diagonal(pairs)
    per_class = pd.DataFrame({"class": pd.Series(classes, dtype=object), "a_boxes": conf[:C].sum(axis=1),
                              "b_boxes": conf[:, :C].sum(axis=0), "agree": agree, "relabelled_to_other": pairs.sum(axis=1) - agree,
                              "relabelled_from_other": pairs.sum(axis=0) - agree, "missing": conf[:C, C], "extra": conf[C, :C]})
    pr = {"row": np.arange(n, dtype=np.int64)}
    if sources is not None:
        pr["source"] = np.asarray(sources, object)
    pr.update({"a_boxes": np.diff(off_a), "b_boxes": np.diff(off_b), "agree": rc[:, 0], "relabelled": rc[:, 1],
               "missing": rc[:, 2], "extra": rc[:, 3]})
    totals = {"rows": n, "a_boxes": len(flat_a), "b_boxes": len(flat_b), "matched": int(rc[:, :2].sum()),
              "agree": int(rc[:, 0].sum()), "relabelled": int(rc[:, 1].sum()), "missing": int(rc[:, 2].sum()),
              "extra": int(rc[:, 3].sum()), "iou_threshold": float(iou_threshold), "by_label": bool(by_label)}
    return {"classes": classes, "confusion": pd.DataFrame(conf, index=pd.Index(labels, dtype=object),
                                                          columns=pd.Index(labels, dtype=object)),
            "per_class": per_class, "hist_iou": hist, "per_row": pd.DataFrame(pr), "differences": differences, "totals": totals}


def records(frame):
    """rows of a frame as tuples in which every NaN equals every NaN and ints equal their numpy twins"""
    out = []
    for rec in frame.itertuples(index=False, name=None):
        out.append(tuple("nan" if isinstance(v, (float, np.floating)) and v != v else
                         (v.item() if isinstance(v, np.generic) else v) for v in rec))
    return out


def check_comparison(got, want):
    """assert that a BoxComparison equals expected_comparison's answer (python_cells and the unpaired rows aside)"""
    assert got.classes == want["classes"]
    assert list(got.confusion.index) == list(want["confusion"].index) == list(got.confusion.columns)
    assert got.confusion.to_numpy().dtype == np.int64
    assert np.array_equal(got.confusion.to_numpy(), want["confusion"].to_numpy())
    for nm in ("per_class", "per_row", "differences"):
        g, w = getattr(got, nm), want[nm]
        assert list(g.columns) == list(w.columns), nm
        assert records(g) == records(w), nm
    assert got.hist_iou.dtype == np.int64 and np.array_equal(got.hist_iou, want["hist_iou"])
    for k, v in want["totals"].items():
        gv = got.totals[k]
        assert gv == v or (isinstance(v, float) and v != v and gv != gv), (k, gv, v)
