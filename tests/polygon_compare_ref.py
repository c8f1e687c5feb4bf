"""The K22 rule (include/dyd.h: polygon comparison by mask IoU) restated in numpy on top of polygon_raster_ref.cover and row_size.
It produces every output of the entries, the pair table included; the GPU tests and the fake backend of the CPU tests compare
against it.  A definition: whole images per polygon, no strips, no chunks."""
import numpy as np

from polygon_raster_ref import LIMIT, cover, row_size

ACT_DONE, ACT_BAD, ACT_FEW, ACT_NO_ROW, ACT_UNSELECTED = 0, 2, 3, 5, 255
STATUS_PAIRS = 4
NAMES = ("row_status", "pair_off", "a_action", "b_action", "a_pixels", "b_pixels", "a_match", "b_match", "b_iou", "a_best", "b_best",
         "row_counts", "confusion", "pixel_confusion", "row_pixels", "pairs")


def _actions(xy, pt_off, lo, hi, cls, compared):
    act = np.full(hi - lo, ACT_UNSELECTED, np.uint8)
    for k, p in enumerate(range(lo, hi)):
        pts = xy[pt_off[p]:pt_off[p + 1]]
        if cls[p] < 0:
            continue
        if not compared:
            act[k] = ACT_NO_ROW
        elif not (np.abs(pts) < LIMIT).all():               # NaN and inf fail too
            act[k] = ACT_BAD
        elif len(pts) < 2:
            act[k] = ACT_FEW
        else:
            act[k] = ACT_DONE
    return act


def compare_arrays(a_xy, a_pt_off, a_row_off, a_cls, b_xy, b_pt_off, b_row_off, b_cls, width, height, n_classes, thr=0.5,
                   by_label=False, max_pixels_per_row=1 << 26, max_pairs_per_row=1 << 20):
    """-> the sixteen arrays of NAMES, in that order"""
    a_xy, b_xy = (np.asarray(v, np.float64).reshape(-1, 2) for v in (a_xy, b_xy))
    a_pt_off, a_row_off, a_cls, b_pt_off, b_row_off, b_cls = (np.asarray(v, np.int64) for v in
                                                             (a_pt_off, a_row_off, a_cls, b_pt_off, b_row_off, b_cls))
    W, H = np.asarray(width, np.float64), np.asarray(height, np.float64)
    n, C, thr = len(W), int(n_classes), float(thr)
    NA, NB = len(a_cls), len(b_cls)
    status, pair_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    a_act, b_act = np.full(NA, ACT_UNSELECTED, np.uint8), np.full(NB, ACT_UNSELECTED, np.uint8)
    a_pix, b_pix = np.zeros(NA, np.int64), np.zeros(NB, np.int64)
    a_match, b_match = np.full(NA, -1, np.int32), np.full(NB, -1, np.int32)
    b_iou, a_best, b_best = np.zeros(NB), np.zeros(NA), np.zeros(NB)
    rows, conf = np.zeros((n, 4), np.int32), np.zeros((C + 1, C + 1), np.uint64)
    pconf, row_pixels = np.zeros((C + 1, C + 1), np.uint64), np.zeros((n, 2), np.int64)
    pairs = []
    for r in range(n):
        a0, a1, b0, b1 = a_row_off[r], a_row_off[r + 1], b_row_off[r], b_row_off[r + 1]
        na, nb = a1 - a0, b1 - b0
        status[r], w, h = row_size(W[r], H[r], max_pixels_per_row)
        if status[r] == 0 and na * nb > max_pairs_per_row:
            status[r] = STATUS_PAIRS
        ok = status[r] == 0
        pair_off[r + 1] = pair_off[r] + (na * nb if ok else 0)
        a_act[a0:a1] = _actions(a_xy, a_pt_off, a0, a1, a_cls, ok)
        b_act[b0:b1] = _actions(b_xy, b_pt_off, b0, b1, b_cls, ok)
        if not ok:
            continue
        cov_a = [cover(a_xy[a_pt_off[p]:a_pt_off[p + 1]], w, h) if a_act[p] == 0 else None for p in range(a0, a1)]
        cov_b = [cover(b_xy[b_pt_off[p]:b_pt_off[p + 1]], w, h) if b_act[p] == 0 else None for p in range(b0, b1)]
        own = []                                            # the class per pixel on either side, C = background
        for covs, cls, lo, pix in ((cov_a, a_cls, a0, a_pix), (cov_b, b_cls, b0, b_pix)):
            o = np.full((h, w), C, np.int64)
            for k, c in enumerate(covs):
                if c is not None:
                    pix[lo + k] = int(c.sum())
                    o[c] = cls[lo + k]
            own.append(o)
        np.add.at(pconf, (own[0].reshape(-1), own[1].reshape(-1)), np.uint64(1))
        row_pixels[r, 0] = int(((own[0] == own[1]) & (own[0] < C)).sum())
        row_pixels[r, 1] = int(((own[0] < C) | (own[1] < C)).sum())
        flat = [np.stack([np.zeros(w * h, np.int64) if c is None else c.reshape(-1).astype(np.int64) for c in covs])
                if covs else np.zeros((0, w * h), np.int64) for covs in (cov_a, cov_b)]
        inter = (flat[0] @ flat[1].T).astype(np.uint32)     # |cover(a) & cover(b)| per pair; 0 with a polygon that is not compared
        pairs.append(inter.reshape(-1))
        pa, pb = a_pix[a0:a1], b_pix[b0:b1]
        uni = pa[:, None] + pb[None, :] - inter
        iou = np.where(inter > 0, inter / np.maximum(uni, 1).astype(np.float64), 0.0)
        a_ok, b_ok = a_act[a0:a1] == 0, b_act[b0:b1] == 0
        if na and nb:
            a_best[a0:a1] = iou.max(axis=1)
            b_best[b0:b1] = iou.max(axis=0)
        free = a_ok.copy()
        for j in np.flatnonzero(b_ok):
            cand = free & (inter[:, j] > 0) & (iou[:, j] >= thr)
            if by_label:
                cand &= a_cls[a0:a1] == b_cls[b0 + j]
            idx = np.flatnonzero(cand)
            if len(idx):
                i = idx[np.argmax(iou[idx, j])]             # the first of equal maxima: the lowest index
                free[i] = False
                a_match[a0 + i], b_match[b0 + j], b_iou[b0 + j] = j, i, iou[i, j]
                ca, cb = a_cls[a0 + i], b_cls[b0 + j]
                rows[r, 0 if ca == cb else 1] += 1
                conf[ca, cb] += np.uint64(1)
            else:
                rows[r, 3] += 1
                conf[C, b_cls[b0 + j]] += np.uint64(1)
        for i in np.flatnonzero(free):
            rows[r, 2] += 1
            conf[a_cls[a0 + i], C] += np.uint64(1)
    pairs = np.concatenate(pairs).astype(np.uint32) if pairs else np.zeros(0, np.uint32)
    return (status, pair_off, a_act, b_act, a_pix, b_pix, a_match, b_match, b_iou, a_best, b_best, rows, conf, pconf, row_pixels,
            pairs)
