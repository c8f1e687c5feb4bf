"""The box audit restated from its definition, for tests/test_box_audit_cpu.py and
tests/test_gpu_box_audit.py.  Two levels:

- ``audit_table``: cells + sizes -> everything audit_boxes_* returns, in plain Python (CPython's json, float()).
- ``audit_arrays``: what K10 computes from the scanned arrays (box4, row_off, class ids, W, H, size status), in numpy.
"""
import json
import math

import numpy as np

NB_BPI = 257
CLASS_COLS = ("no_size", "bad_coords", "degenerate", "writable", "out_of_image", "small", "medium", "large", "images")
ROW_COLS = ("unmatchable", "no_size", "bad_coords", "degenerate", "writable", "out_of_image")
NUMBER = (int, float, np.integer, np.floating)


def boxes_of(cell):
    """utils._extract_boxes_with_labels' walk with the object index: [(object, name, x1, y1, x2, y2)]"""
    out = []
    if not isinstance(cell, str):
        return out
    try:
        for k, obj in enumerate(json.loads(cell).get("objects", [])):
            if not isinstance(obj, dict):
                continue
            name = obj.get("name")
            if not name:
                continue
            pts = obj.get("polygon", {}).get("ptList", [])
            if not pts:
                continue
            dp = [p for p in pts if isinstance(p, dict)]
            xs = [p.get("x") for p in dp if "x" in p]
            ys = [p.get("y") for p in dp if "y" in p]
            if xs and ys:
                out.append((k, name, min(xs), min(ys), max(xs), max(ys)))
    except Exception:
        pass
    return out


def size_status(w, h):
    """-> ("ok" | "missing" | "invalid", W, H)"""
    try:
        if not w or not h:
            return "missing", None, None
    except Exception:
        return "invalid", None, None
    vals = []
    for v in (w, h):
        if not isinstance(v, NUMBER):
            return "invalid", None, None
        try:
            f = float(v)
        except OverflowError:
            return "invalid", None, None
        if not math.isfinite(f) or f <= 0:
            return "invalid", None, None
        vals.append(f)
    return "ok", vals[0], vals[1]


def fnum(v):
    if not isinstance(v, NUMBER):
        return None
    try:
        f = float(v)
    except OverflowError:
        return None
    return f if math.isfinite(f) else None


def fval(v):
    """the coordinate as the problems table shows it: float(v) (inf when it overflows), NaN for a non-number"""
    if not isinstance(v, NUMBER):
        return math.nan
    try:
        return float(v)
    except OverflowError:
        return math.inf


def bin_of(v, nb):
    f = math.floor(v * nb) if math.isfinite(v * nb) else (math.inf if v * nb > 0 else -math.inf)
    return int(min(max(f, 0), nb - 1))


def classify(box, st, W, H, nb):
    """-> (category, out_of_image, area bucket, (bin wn, bin hn), (bin xc, bin yc)) of a class-keyed box"""
    if st != "ok":
        return "no_size", False, None, None, None
    c = [fnum(v) for v in box]
    if any(v is None for v in c):
        return "bad_coords", False, None, None, None
    x1, y1, x2, y2 = c
    bw = max(x2 - x1, 0.0)
    bh = max(y2 - y1, 0.0)
    if bw <= 0 or bh <= 0:
        return "degenerate", False, None, None, None
    ooi = x1 < 0 or y1 < 0 or x2 > W or y2 > H
    xc = (x1 + x2) / 2 / W
    yc = (y1 + y2) / 2 / H
    wn = bw / W
    hn = bh / H
    a = bw * bh
    area = "small" if a < 1024 else "medium" if a < 9216 else "large"
    return "writable", ooi, area, (bin_of(wn, nb), bin_of(hn, nb)), (bin_of(xc, nb), bin_of(yc, nb))


def audit_table(cells, widths, heights, nbins=16):
    n = len(cells)
    if widths is None:
        widths = heights = [None] * n
    per_box, rows = [], []
    names = set()
    for i in range(n):
        st, W, H = size_status(widths[i], heights[i])
        bx = boxes_of(cells[i])
        rc = dict.fromkeys(ROW_COLS, 0)
        for k, name, *box in bx:
            if not isinstance(name, str):
                rc["unmatchable"] += 1
                continue
            names.add(name)
            cat, ooi, area, bwh, bxy = classify(box, st, W, H, nbins)
            rc[cat] += 1
            rc["out_of_image"] += ooi
            per_box.append((i, k, name, cat, ooi, area, bwh, bxy, box))
        rows.append({"size_status": st, "n_boxes": len(bx), **rc})
    classes = sorted(names)
    cid = {c: j for j, c in enumerate(classes)}
    C = len(classes)
    counts = {c: dict.fromkeys(CLASS_COLS, 0) for c in classes}
    seen = set()
    wh = np.zeros((C, nbins, nbins), np.int64)
    xy = np.zeros((C, nbins, nbins), np.int64)
    problems = []
    for i, k, name, cat, ooi, area, bwh, bxy, box in per_box:
        d = counts[name]
        d[cat] += 1
        d["out_of_image"] += ooi
        if area:
            d[area] += 1
            wh[cid[name]][bwh] += 1
            xy[cid[name]][bxy] += 1
        if (i, name) not in seen:
            seen.add((i, name))
            d["images"] += 1
        issue = cat if cat in ("bad_coords", "degenerate") else "out_of_image" if ooi else None
        if issue:
            problems.append((i, k, name, issue, *[fval(v) for v in box]))
    bpi = np.zeros(NB_BPI, np.int64)
    for r in rows:
        bpi[min(r["n_boxes"], 256)] += 1
    return {"classes": classes, "counts": counts, "hist_wh": wh, "hist_xy": xy, "bpi": bpi, "rows": rows,
            "problems": problems}


def check_audit(a, ref):
    """assert that a BoxAudit equals audit_table's answer"""
    assert a.classes == ref["classes"]
    pc = a.per_class
    assert pc["class"].tolist() == ref["classes"]
    for col in CLASS_COLS:
        assert pc[col].tolist() == [ref["counts"][c][col] for c in ref["classes"]], col
    assert (pc["boxes"] == pc["no_size"] + pc["bad_coords"] + pc["degenerate"] + pc["writable"]).all()
    assert (pc["small"] + pc["medium"] + pc["large"] == pc["writable"]).all()
    assert (pc["out_of_image"] <= pc["writable"]).all()
    assert np.array_equal(a.hist_wh, ref["hist_wh"]) and np.array_equal(a.hist_xy, ref["hist_xy"])
    assert a.hist_wh.dtype == np.int64 and a.hist_xy.dtype == np.int64
    assert np.array_equal(a.boxes_per_image, ref["bpi"])
    pr = a.per_row
    assert pr["row"].tolist() == list(range(len(ref["rows"])))
    for col in ("size_status", "n_boxes") + ROW_COLS:
        assert pr[col].tolist() == [r[col] for r in ref["rows"]], col
    got = list(zip(a.problems["row"].tolist(), a.problems["object"].tolist(), a.problems["name"].tolist(),
                   a.problems["issue"].tolist()))
    assert got == [p[:4] for p in ref["problems"]]
    for col, j in (("x1", 4), ("y1", 5), ("x2", 6), ("y2", 7)):
        want = [p[j] for p in ref["problems"]]
        assert np.array_equal(a.problems[col].to_numpy(np.float64), np.asarray(want, np.float64), equal_nan=True), col
    t = a.totals
    assert t["boxes"] == sum(r["n_boxes"] for r in ref["rows"])
    assert t["unmatchable_name_boxes"] == sum(r["unmatchable"] for r in ref["rows"])
    for st in ("ok", "missing", "invalid"):
        assert t["rows_" + st] == sum(r["size_status"] == st for r in ref["rows"])


def audit_arrays(box4, row_off, cls, W, H, status, n_classes, nb):
    """K10 restated in numpy -> (flag, row_counts [N,6] i32, class_counts [C,9] i64, hist_wh, hist_xy, bpi)"""
    box4 = np.asarray(box4, np.float64).reshape(-1, 4)
    row_off = np.asarray(row_off, np.int64)
    cls = np.asarray(cls, np.int64)
    n = len(row_off) - 1
    B = len(cls)
    C = int(n_classes)
    row = np.repeat(np.arange(n), np.diff(row_off))
    x1, y1, x2, y2 = box4.T
    st = np.asarray(status)[row]
    w = np.asarray(W, np.float64)[row]
    h = np.asarray(H, np.float64)[row]
    unm = (cls < 0) | (cls >= C)
    with np.errstate(all="ignore"):
        finite = np.isfinite(box4).all(axis=1)
        dx, dy = x2 - x1, y2 - y1
        bw = np.where(0.0 > dx, 0.0, dx)
        bh = np.where(0.0 > dy, 0.0, dy)
        cat = np.where(st != 0, 0, np.where(~finite, 1, np.where((bw <= 0) | (bh <= 0), 2, 3)))
        wr = (cat == 3) & ~unm
        ooi = wr & ((x1 < 0) | (y1 < 0) | (x2 > w) | (y2 > h))
        a = bw * bh
        area = np.where(a < 1024, 0, np.where(a < 9216, 1, 2))

        def binv(v):
            f = np.floor(v * float(nb))
            f = np.where(f < 0.0, 0.0, f)
            f = np.where(f > nb - 1, float(nb - 1), f)
            return np.where(wr, f, 0.0).astype(np.int64)

        bx, by = binv((x1 + x2) / 2 / w), binv((y1 + y2) / 2 / h)
        bwb, bhb = binv(bw / w), binv(bh / h)
    flag = np.where(unm, 0x80, cat | (ooi.astype(np.int64) << 2) | np.where(wr, area << 3, 0)).astype(np.uint8)
    rows = np.zeros((n, 6), np.int64)
    rows[:, 0] = np.bincount(row[unm], minlength=n)
    for k in range(4):
        rows[:, 1 + k] = np.bincount(row[~unm & (cat == k)], minlength=n)
    rows[:, 5] = np.bincount(row[ooi], minlength=n)
    c = np.where(unm, 0, cls)
    cc = np.zeros((C, 9), np.int64)
    for k in range(4):
        cc[:, k] = np.bincount(c[~unm & (cat == k)], minlength=C)[:C]
    cc[:, 4] = np.bincount(c[ooi], minlength=C)[:C]
    for k in range(3):
        cc[:, 5 + k] = np.bincount(c[wr & (area == k)], minlength=C)[:C]
    if B and C:
        pairs = np.unique(row[~unm] * C + c[~unm])
        cc[:, 8] = np.bincount(pairs % C, minlength=C)[:C]
    hw = np.bincount(((c * nb + bwb) * nb + bhb)[wr], minlength=C * nb * nb).reshape(C, nb, nb) if C else np.zeros((0, nb, nb), np.int64)
    hx = np.bincount(((c * nb + bx) * nb + by)[wr], minlength=C * nb * nb).reshape(C, nb, nb) if C else np.zeros((0, nb, nb), np.int64)
    bpi = np.bincount(np.minimum(np.diff(row_off), 256), minlength=NB_BPI).astype(np.int64)
    return flag, rows.astype(np.int32), cc, hw.astype(np.int64), hx.astype(np.int64), bpi
