"""Flatten: DataFrame cells -> the SoA buffers the device stage consumes, and back (emit).

Host-side work of the drop-in steps.  The structure walk below follows the reference's own
accessors step by step (``doc.get("objects", [])``, ``obj.get("polygon", {}).get("ptList", [])``,
the ``"x" in p and "y" in p`` guard ...) so that every malformed structure raises the same
exception type, at the same row, as ``core/processor.py:262-281`` / ``:341-366`` do.

Only coordinates that an IEEE double represents exactly go to the device: floats, bools and
ints of magnitude <= 2**53 (K1) / <= 2**25 (K2, where products of differences must also stay
exact).  Anything else in a coordinate slot (None, str, list, huge int) cannot be laid out as
f64 and is resolved right here with the same builtin ``min``/``max``/arithmetic the reference
applies to it, which is also what makes it raise TypeError exactly when the reference does.
``stats`` counts such boxes/rows so callers and tests can assert the device did the work.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field

import numpy as np
import pandas as pd

_K1_INT_LIMIT = 2 ** 53
_K2_INT_LIMIT = 2 ** 25


def _f64_or_none(v, int_limit):
    t = type(v)
    if t is float:
        return v
    if t is int:
        return float(v) if -int_limit <= v <= int_limit else None
    if t is bool:
        return 1.0 if v else 0.0
    return None


# ------------------------------------------------------------------------------------------
# a3  polygon ptList -> bbox  (reference core/processor.py:262-281)
# ------------------------------------------------------------------------------------------
@dataclass
class PolygonBatch:
    docs: list                     # per cell: parsed document, or None when the cell yields None
    objs: list                     # per cell: list of the dict objects of the document (in order)
    box_pts: list                  # per box: its valid points (dicts) — the tokens emit re-uses
    host_boxes: dict               # box index -> ptList computed on the host (non-f64 coordinates)
    xy: np.ndarray                 # [P,2] f64
    pt_off: np.ndarray             # [B+1] i32
    cell_box_off: np.ndarray       # [n_cells+1] i32 first box of each cell
    stats: dict = field(default_factory=dict)


def _host_bbox(points):
    """get_bbox_points (:254-260) on the host for coordinates that are not f64-representable."""
    lo_x = min(p["x"] for p in points)
    hi_x = max(p["x"] for p in points)
    lo_y = min(p["y"] for p in points)
    hi_y = max(p["y"] for p in points)
    return [{"x": lo_x, "y": lo_y}, {"x": hi_x, "y": hi_y}]


def flatten_polygons(cells) -> PolygonBatch:
    docs, objs_per_cell, box_pts, host_boxes = [], [], [], {}
    xs, npts, cell_boxes = [], [], [0]
    n_host = 0
    for cell in cells:
        doc, dict_objs = None, []
        if isinstance(cell, str):                     # :264 — NaN / non-str cells give None
            try:
                doc = json.loads(cell)
            except json.JSONDecodeError:              # :280-281
                doc = None
            else:
                for obj in doc.get("objects", []):    # AttributeError / TypeError propagate like the reference
                    if not isinstance(obj, dict):     # :270 non-dict objects are dropped
                        continue
                    pts = [p for p in obj.get("polygon", {}).get("ptList", [])
                           if isinstance(p, dict) and "x" in p and "y" in p]   # :253
                    flat, ok = [], True
                    for p in pts:
                        x = _f64_or_none(p["x"], _K1_INT_LIMIT)
                        y = _f64_or_none(p["y"], _K1_INT_LIMIT)
                        if x is None or y is None:
                            ok = False
                            break
                        flat.append(x)
                        flat.append(y)
                    if not ok:                         # resolve with builtin min/max, raising as CPython does
                        host_boxes[len(box_pts)] = _host_bbox(pts)
                        n_host += 1
                        flat = []
                    xs.extend(flat)
                    npts.append(len(flat) // 2)
                    box_pts.append(pts)
                    dict_objs.append(obj)
        docs.append(doc)
        objs_per_cell.append(dict_objs)
        cell_boxes.append(len(box_pts))
    pt_off = np.zeros(len(npts) + 1, np.int64)
    np.cumsum(np.asarray(npts, np.int64), out=pt_off[1:])
    if pt_off[-1] >= 2 ** 31:
        raise OverflowError("more than 2^31 points in one batch: split the table into chunks")
    xy = np.asarray(xs, np.float64).reshape(-1, 2)
    return PolygonBatch(docs, objs_per_cell, box_pts, host_boxes, xy, pt_off.astype(np.int32),
                        np.asarray(cell_boxes, np.int32),
                        {"cells": len(docs), "boxes": len(box_pts), "points": int(pt_off[-1]),
                         "host_boxes": n_host})


def emit_polygons(batch: PolygonBatch, arg4: np.ndarray) -> list:
    """Re-serialise every document with each ptList replaced by its two corner points.

    ``arg4[b] = (argmin_x, argmin_y, argmax_x, argmax_y)`` from K1; the emitted coordinate is
    the ORIGINAL Python object at that index (so ``10`` stays ``10`` and ``10.0`` stays ``10.0``,
    processor.py:256-260), -1 marks a box without valid points (:254-255)."""
    out = []
    arg = np.asarray(arg4).tolist()
    for ci, doc in enumerate(batch.docs):
        if doc is None:
            out.append(None)
            continue
        b = int(batch.cell_box_off[ci])
        rewritten = []
        for obj in batch.objs[ci]:
            if b in batch.host_boxes:
                corners = batch.host_boxes[b]
            else:
                pts = batch.box_pts[b]
                a = arg[b]
                if not pts:
                    corners = [{"x": None, "y": None}, {"x": None, "y": None}]
                else:
                    corners = [{"x": pts[a[0]]["x"], "y": pts[a[1]]["y"]},
                               {"x": pts[a[2]]["x"], "y": pts[a[3]]["y"]}]
            new_obj = obj.copy()                      # :271
            if "polygon" not in new_obj:              # :274-275
                new_obj["polygon"] = {}
            new_obj["polygon"]["ptList"] = corners    # :276
            rewritten.append(new_obj)
            b += 1
        doc["objects"] = rewritten                    # :278
        out.append(json.dumps(doc, ensure_ascii=False))   # :279
    return out


# ------------------------------------------------------------------------------------------
# a4  two-point boxes per image row  (reference core/processor.py:341-366)
# ------------------------------------------------------------------------------------------
@dataclass
class BoxBatch:
    box4: np.ndarray               # [B,4] f64 (p1x,p1y,p2x,p2y) as stored; K2 normalises corners
    row_off: np.ndarray            # [n_rows+1] i32
    host_rows: dict                # row -> list of (x1,y1,x2,y2) Python tuples for non-f64 rows
    stats: dict = field(default_factory=dict)


def flatten_boxes(cells) -> BoxBatch:
    flat, counts, host_rows = [], [], {}
    for ri, cell in enumerate(cells):
        row_vals, tuples, device_ok = [], [], True
        try:                                           # :343 — any exception keeps the prefix
            if isinstance(cell, str):                  # :344
                doc = json.loads(cell)
                for obj in doc.get("objects", []):
                    if not isinstance(obj, dict):
                        continue
                    pts = obj.get("polygon", {}).get("ptList", [])
                    if len(pts) != 2:
                        continue
                    a, b = pts
                    if not (isinstance(a, dict) and isinstance(b, dict) and "x" in a and "y" in a
                            and "x" in b and "y" in b):
                        continue
                    raw = (a["x"], a["y"], b["x"], b["y"])
                    # :359-362 — evaluated here only to raise (None vs number ...) exactly where the
                    # reference's min()/max() would; the device redoes the normalisation in f64
                    tuples.append((min(raw[0], raw[2]), min(raw[1], raw[3]),
                                   max(raw[0], raw[2]), max(raw[1], raw[3])))
                    vals = [_f64_or_none(v, _K2_INT_LIMIT) for v in raw]
                    if device_ok and None not in vals:
                        row_vals.extend(vals)
                    else:
                        device_ok = False
        except Exception:                               # noqa: BLE001 (:364-365)
            pass
        if device_ok:
            flat.extend(row_vals)
            counts.append(len(row_vals) // 4)
        else:
            host_rows[ri] = tuples
            counts.append(0)
    row_off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=row_off[1:])
    if row_off[-1] >= 2 ** 31:
        raise OverflowError("more than 2^31 boxes in one batch: split the table into chunks")
    return BoxBatch(np.asarray(flat, np.float64).reshape(-1, 4), row_off.astype(np.int32), host_rows,
                    {"rows": len(counts), "boxes": int(row_off[-1]), "host_rows": len(host_rows)})


def host_row_is_high(boxes, min_boxes, thr) -> bool:
    """meet_conditions / calculate_iou (:328-339, :368-376) for rows whose coordinates are not
    f64-representable (huge ints, strings): CPython arithmetic, raising as the reference does."""
    if len(boxes) < min_boxes:
        return False
    for i in range(len(boxes)):
        p = boxes[i]
        for j in range(i + 1, len(boxes)):
            q = boxes[j]
            inter = (max(0, min(p[2], q[2]) - max(p[0], q[0]))
                     * max(0, min(p[3], q[3]) - max(p[1], q[1])))
            if inter == 0:
                iou = 0.0
            else:
                union = (p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter
                iou = inter / union if union != 0 else 0.0
            if iou >= thr:
                return True
    return False



def pair_iou(p, q):
    """calculate_iou (:328-339) of (earlier, later) corner tuples in CPython arithmetic: exact ints, IEEE doubles,
    first-wins max / min — so a NaN corner behaves as in the reference and strings raise where it raises."""
    ix1 = max(p[0], q[0])
    iy1 = max(p[1], q[1])
    ix2 = min(p[2], q[2])
    iy2 = min(p[3], q[3])
    inter = max(0, ix2 - ix1) * max(0, iy2 - iy1)
    if inter == 0:
        return 0.0
    union = (p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter
    return inter / union if union != 0 else 0.0


def suppress_cell(cell, thr, by_label):
    """Duplicate-box suppression of one cell on the host, for the cells the native scanner leaves to Python (huge ints,
    string coordinates, repeated keys, odd names ...): -> (cell or its re-spelled document, [(object, kept_object, iou)]).

    The boxes are extract_boxes' (:341-366, prefix on exception) with the index of their object and their name; a box is
    dropped when an earlier kept box (of the same name when ``by_label``) reaches pair_iou >= thr with it.  Exceptions of
    pair_iou propagate, as in meet_conditions.  A cell that loses nothing is returned as the same object."""
    if not isinstance(cell, str):
        return cell, []
    boxes = []
    try:
        doc = json.loads(cell)
        for k, obj in enumerate(doc.get("objects", [])):
            if not isinstance(obj, dict):
                continue
            pts = obj.get("polygon", {}).get("ptList", [])
            if len(pts) != 2:
                continue
            a, b = pts
            if not (isinstance(a, dict) and isinstance(b, dict) and "x" in a and "y" in a and "x" in b and "y" in b):
                continue
            boxes.append((k, (min(a["x"], b["x"]), min(a["y"], b["y"]), max(a["x"], b["x"]), max(a["y"], b["y"])),
                          obj.get("name")))
    except Exception:                                   # noqa: BLE001 (:364-365) keep the prefix
        pass
    kept, removed = [], []
    for k, box, name in boxes:
        for kk, kbox, kname in kept:
            if not by_label or kname == name:
                iou = pair_iou(kbox, box)
                if iou >= thr:
                    removed.append((k, kk, iou))
                    break
        else:
            kept.append((k, box, name))
    if not removed:
        return cell, []
    drop = {k for k, _, _ in removed}
    doc["objects"] = [o for k, o in enumerate(doc["objects"]) if k not in drop]
    return json.dumps(doc, ensure_ascii=False), removed


def audit_cell_boxes(cell) -> list:
    """The box audit's boxes of one cell on the host, for the cells the native scanner leaves to Python (numbers, true or
    containers as "name", string or huge-int coordinates, repeated keys ...): utils._extract_boxes_with_labels' walk
    (reference utils.py:681-710: named objects with a non-empty ptList, first-wins min / max, the prefix kept on any
    exception) -> [(index of the object in "objects", name, min x, min y, max x, max y)]."""
    collected = []
    if not isinstance(cell, str):
        return collected
    try:
        for k, obj in enumerate(json.loads(cell).get("objects", [])):
            if not isinstance(obj, dict):
                continue
            name = obj.get("name")
            if not name:
                continue
            points = obj.get("polygon", {}).get("ptList", [])
            if not points:
                continue
            dict_points = [pt for pt in points if isinstance(pt, dict)]
            xs = [pt.get("x") for pt in dict_points if "x" in pt]
            ys = [pt.get("y") for pt in dict_points if "y" in pt]
            if xs and ys:
                collected.append((k, name, min(xs), min(ys), max(xs), max(ys)))
    except Exception:                                   # noqa: BLE001 (utils.py:708-709) keep the prefix
        pass
    return collected


def seg_cell_polygons(cell) -> list:
    """The segmentation step's polygons of one cell on the host, for the cells the native scanner leaves to Python: the
    objects of audit_cell_boxes (the YOLO step's objects, the prefix kept on any exception) with their points ->
    [(index of the object in "objects", name, [(x, y) of every ptList dict holding both "x" and "y", as read])]."""
    boxes = audit_cell_boxes(cell)
    if not boxes:
        return []
    objs = json.loads(cell)["objects"]                  # the walk above got this far without an exception
    out = []
    for k, name, *_ in boxes:
        pts = objs[k]["polygon"]["ptList"]
        out.append((k, name, [(pt["x"], pt["y"]) for pt in pts if isinstance(pt, dict) and "x" in pt and "y" in pt]))
    return out


def repair_cell(cell, decisions) -> str:
    """One cell re-spelled by the box repair step from decisions already made (K11): ``decisions`` maps the index of an object
    in "objects" to None (the object is left out) or to the clipped corners (x1', y1', x2', y2'), which replace its
    polygon.ptList by the replace step's two-point shape (reference processor.py:260) with float values.  Every other object
    stays as json.loads read it.  -> json.dumps(doc, ensure_ascii=False)"""
    doc = json.loads(cell)
    objs = doc["objects"]
    for k, box in decisions.items():
        if box is not None:
            x1, y1, x2, y2 = (float(v) for v in box)
            objs[k]["polygon"]["ptList"] = [{"x": x1, "y": y1}, {"x": x2, "y": y2}]
    doc["objects"] = [o for k, o in enumerate(objs) if k not in decisions or decisions[k] is not None]
    return json.dumps(doc, ensure_ascii=False)


def simplify_cell(cell, decisions) -> str:
    """One cell re-spelled by the polygon simplify step from decisions already made (K19): ``decisions`` maps the index of an
    object in "objects" to its keep list, one flag per vertex (the ptList dicts holding both "x" and "y", in order).  The ptList
    entries of the vertices whose flag is 0 are left out; every other entry and every other object stays as json.loads read it.
    -> json.dumps(doc, ensure_ascii=False)"""
    doc = json.loads(cell)
    objs = doc["objects"]
    for k, keep in decisions.items():
        poly = objs[k]["polygon"]
        flags = iter(keep)
        poly["ptList"] = [pt for pt in poly["ptList"]
                          if not (isinstance(pt, dict) and "x" in pt and "y" in pt) or next(flags)]
    return json.dumps(doc, ensure_ascii=False)


# ------------------------------------------------------------------------------------------
# a1 / a2  key column -> flat bytes + offsets for K3
# ------------------------------------------------------------------------------------------
NA_KEY = np.array([0x6e616e5f6b65795f, 0x5f5f6e615f5f6b79], np.uint64)   # key given to missing cells


def _strings_to_bytes(values) -> tuple:
    """list of str -> (uint8 buffer, int64 offsets)."""
    try:
        import pyarrow as pa
        arr = pa.array(values, type=pa.large_string())
        bufs = arr.buffers()
        off = np.frombuffer(bufs[1], dtype=np.int64, count=len(arr) + 1)
        data = np.frombuffer(bufs[2], dtype=np.uint8, count=int(off[-1])) if bufs[2] is not None else np.zeros(0, np.uint8)
        return data, off
    except ImportError:
        enc = [v.encode("utf-8") for v in values]
        off = np.zeros(len(enc) + 1, np.int64)
        np.cumsum([len(e) for e in enc], out=off[1:])
        return np.frombuffer(b"".join(enc), dtype=np.uint8), off


def column_key_bytes(col: pd.Series) -> tuple:
    """Canonical bytes of a key column for drop_duplicates-style equality (processor.py:140).

    -> (bytes u8, offsets i64, na_mask bool).  Equality classes match pandas': strings by value,
    all missing cells equal to each other (the caller overwrites their hash with NA_KEY), numeric
    columns by value with -0.0 == 0.0."""
    from . import pycells
    kind = col.dtype.kind
    if kind == "O" and pycells.available() and pycells.all_str(col.to_numpy()):
        na = np.zeros(len(col), bool)                       # every cell is a str (parallel header walk): no isna pass (60 ms per 1M cells)
    else:
        na = col.isna().to_numpy()
    if kind in "iub":
        raw = np.ascontiguousarray(col.to_numpy().astype(np.int64)).view(np.uint8)
        return raw, np.arange(len(col) + 1, dtype=np.int64) * 8, na
    if kind == "f":
        v = col.to_numpy().astype(np.float64) + 0.0          # -0.0 + 0.0 == +0.0
        v[na] = 0.0
        raw = np.ascontiguousarray(v).view(np.uint8)
        return raw, np.arange(len(col) + 1, dtype=np.int64) * 8, na
    # object column.  The usual case — every present cell is a str (URLs) — needs no per-cell Python: the str objects' UTF-8
    # buffers are gathered by worker threads (pycells), or pyarrow walks the objects in C; missing cells come out empty (the
    # caller gives them NA_KEY).
    if pycells.available() and col.dtype == object:
        try:
            flat = pycells.flat_utf8(col.to_numpy(), na)
        except UnicodeEncodeError:
            flat = None
        if flat is not None:
            return flat[0], flat[1], na
    try:
        import pyarrow as pa
        arr = pa.array(col.to_numpy(), type=pa.large_string(), from_pandas=True)
        bufs = arr.buffers()
        off = np.frombuffer(bufs[1], dtype=np.int64, count=len(arr) + 1)
        data = np.frombuffer(bufs[2], dtype=np.uint8, count=int(off[-1])) if bufs[2] is not None else np.zeros(0, np.uint8)
        return data, off, na
    except ImportError:
        pass
    except Exception:  # noqa: BLE001 - pa.ArrowInvalid / ArrowTypeError: some cell is not a str -> the tagged spelling below
        pass
    # Mixed column.  A str keeps its plain utf-8 bytes (the same key as on the fast path above — shards of one table must
    # agree); every other value is tagged with a 0xFF byte, which no utf-8 text contains, so "1.0" the string and 1.0 the
    # number stay apart.
    vals = col.tolist()
    plain = all(m or type(v) is str or isinstance(v, (bool, int, float)) for v, m in zip(vals, na.tolist()))
    ids = {}                 # any other hashable: one id per equality class, by Python's own hash / == (what pandas' object
    cells = []               # table uses, so 1 == 1.0 == Decimal(1) fall together); an unhashable cell raises TypeError like pandas
    for v, missing in zip(vals, na.tolist()):
        if missing:
            cells.append(b"")
        elif type(v) is str:
            cells.append(v.encode("utf-8"))
        elif plain:
            # 1 == 1.0 == True hash alike in pandas' object table; an int that no float equals keeps its own spelling
            try:
                as_float = float(v)
                exact = not isinstance(v, int) or int(as_float) == v
            except OverflowError:
                exact = False
            cells.append((b"\xffn" + repr(as_float).encode()) if exact else (b"\xffi" + repr(int(v)).encode()))
        else:
            cells.append(b"\xffo%d" % ids.setdefault(v, len(ids)))
    off = np.zeros(len(cells) + 1, np.int64)
    np.cumsum([len(c) for c in cells], out=off[1:])
    blob = b"".join(cells)
    return (np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(0, np.uint8)), off, na


def column_str_bytes(col: pd.Series, drop_na: bool = False) -> tuple:
    """``col.astype(str)`` (after ``dropna`` when asked) as flat bytes (processor.py:194, :198)."""
    from . import pycells
    every_cell_str = col.dtype == object and pycells.available() and pycells.all_str(col.to_numpy())
    if drop_na and not every_cell_str:
        col = col.dropna()
    if pycells.available() and col.dtype == object:      # an all-str column: astype(str) changes nothing but the missing cells (NaN -> "nan", None -> "None")
        try:
            na = np.zeros(len(col), bool) if every_cell_str else col.isna().to_numpy()
            flat = pycells.flat_utf8(col.to_numpy(), na, na_as_text=True)
        except UnicodeEncodeError:
            flat = None
        if flat is not None:
            return flat
    data, off = _strings_to_bytes(col.astype(str).tolist())
    return data, off


# ---- the tile step's grid (K20; include/dyd.h has the rule) -------------------------------------------------------
TILE_STATUS = ("tiled", "no_size", "fractional_size", "too_many_tiles")   # K20 row status codes 0..3
_TILE_LIMIT = float(1 << 43)


def tile_grid(width, height, tile_w: int, tile_h: int, step_x: int, step_y: int, max_tiles_per_row: int = 4096) -> tuple:
    """K20's grid from the same integer rule as the kernel -> (status u8 [n], nx int64 [n], ny int64 [n]); nx = ny = 0 for a
    row that is not tiled"""
    W, H = np.asarray(width, np.float64), np.asarray(height, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (W > 0) & (W < _TILE_LIMIT) & (H > 0) & (H < _TILE_LIMIT)
        whole = ok & (W == np.floor(W)) & (H == np.floor(H))
    Lx, Ly = np.where(whole, W, 0).astype(np.int64), np.where(whole, H, 0).astype(np.int64)
    nx = np.where(Lx <= tile_w, 1, -((tile_w - Lx) // step_x) + 1)
    ny = np.where(Ly <= tile_h, 1, -((tile_h - Ly) // step_y) + 1)
    cap = max_tiles_per_row + 1                          # the product of the clipped counts stays below 2^42
    many = whole & (np.minimum(nx, cap) * np.minimum(ny, cap) > max_tiles_per_row)
    status = np.where(~ok, 1, np.where(~whole, 2, np.where(many, 3, 0))).astype(np.uint8)
    tiled = status == 0
    return status, np.where(tiled, nx, 0).astype(np.int64), np.where(tiled, ny, 0).astype(np.int64)


def tile_boxes(width, height, nx, ny, tile_w: int, tile_h: int, step_x: int, step_y: int) -> tuple:
    """the tiles of tile_grid's rows in K20's order (row by row, ty * nx + tx) -> (row, tile, x0, y0, w, h), int64 each"""
    nx, ny = np.asarray(nx, np.int64), np.asarray(ny, np.int64)
    count = nx * ny
    row = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    tile = np.arange(int(count.sum()), dtype=np.int64) - first[row]
    Lx, Ly = np.asarray(width, np.float64)[row].astype(np.int64), np.asarray(height, np.float64)[row].astype(np.int64)
    tx, ty = tile % np.maximum(nx[row], 1), tile // np.maximum(nx[row], 1)
    x0 = np.where(Lx <= tile_w, 0, np.minimum(tx * step_x, Lx - tile_w))
    y0 = np.where(Ly <= tile_h, 0, np.minimum(ty * step_y, Ly - tile_h))
    return row, tile, x0, y0, np.minimum(Lx, tile_w), np.minimum(Ly, tile_h)


# ---- the mask step's rows, order and batches (K21; include/dyd.h has the rule) ------------------------------------
MASK_STATUS = ("rasterised", "no_size", "fractional_size", "too_large")   # K21 row status codes 0..3


def mask_rows(width, height, max_pixels_per_row: int = 1 << 26) -> tuple:
    """K21's row rule from the same tests as the kernel -> (status u8 [n], pixels int64 [n]); pixels = W * H for a row that is
    rasterised, else 0"""
    W, H = np.asarray(width, np.float64), np.asarray(height, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (W > 0) & (W < _TILE_LIMIT) & (H > 0) & (H < _TILE_LIMIT)
        whole = ok & (W == np.floor(W)) & (H == np.floor(H))
    w, h = np.where(whole, W, 0).astype(np.int64), np.where(whole, H, 0).astype(np.int64)
    cap = max_pixels_per_row + 1                         # the product of the clipped sizes stays below 2^62
    large = whole & (np.minimum(w, cap) * np.minimum(h, cap) > max_pixels_per_row)
    status = np.where(~ok, 1, np.where(~whole, 2, np.where(large, 3, 0))).astype(np.uint8)
    return status, np.where(status == 0, w * h, 0).astype(np.int64)


def mask_batches(pixels, batch_pixels: int) -> list:
    """consecutive row ranges [(a, b)] whose pixel totals stay within batch_pixels; a single larger row goes alone"""
    out, a, total = [], 0, 0
    for i, v in enumerate(np.asarray(pixels, np.int64).tolist()):
        if i > a and total + v > batch_pixels:
            out.append((a, i))
            a, total = i, 0
        total += v
    if len(pixels) > a:
        out.append((a, len(pixels)))
    return out


def large_first_order(xy, pt_off, row_off) -> np.ndarray:
    """the polygons of a table, within each row stably sorted by decreasing (max x - min x) * (max y - min y) of their points
    (NaN and a polygon without points sort as 0) -> perm int64 [B]: the polygon at new position k is the old perm[k]"""
    pt_off, row_off = np.asarray(pt_off, np.int64), np.asarray(row_off, np.int64)
    nb = len(pt_off) - 1
    pts = np.asarray(xy, np.float64).reshape(-1, 2)
    area = np.zeros(nb)
    full = np.flatnonzero(np.diff(pt_off) > 0)
    if len(full):
        first = pt_off[:-1][full]                        # polygons without points own no entry, so these delimit the others'
        with np.errstate(invalid="ignore", over="ignore"):
            ext = [np.maximum.reduceat(pts[:, c], first) - np.minimum.reduceat(pts[:, c], first) for c in (0, 1)]
            area[full] = np.nan_to_num(ext[0] * ext[1], nan=0.0)
    row = np.repeat(np.arange(len(row_off) - 1, dtype=np.int64), np.diff(row_off))
    return np.lexsort((-area, row)).astype(np.int64)     # lexsort is stable


def permute_polygons(xy, pt_off, perm) -> tuple:
    """-> (xy, pt_off int32) of the table whose polygon k is the given table's polygon perm[k]"""
    pt_off, perm = np.asarray(pt_off, np.int64), np.asarray(perm, np.int64)
    count = np.diff(pt_off)[perm]
    new_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    src = np.repeat(pt_off[:-1][perm] - new_off[:-1], count) + np.arange(int(new_off[-1]), dtype=np.int64)
    return np.asarray(xy, np.float64).reshape(-1, 2)[src].reshape(-1), new_off.astype(np.int32)


# ---- the polygon comparison's rows and batches (K22; include/dyd.h has the rule) ----------------------------------
COMPARE_STATUS = ("compared", *MASK_STATUS[1:], "too_many_pairs")   # K22 row status codes 0..4


def compare_rows(width, height, n_a, n_b, max_pixels_per_row: int = 1 << 26, max_pairs_per_row: int = 1 << 20) -> tuple:
    """K22's row rule: K21's sizes (mask_rows), then 4 for a row of more than max_pairs_per_row pairs of polygons -> (status u8
    [n], pixels int64 [n], pairs int64 [n]); pixels = W * H and pairs = n_a * n_b for a row that is compared, else 0"""
    status, pixels = mask_rows(width, height, max_pixels_per_row)
    pairs = np.asarray(n_a, np.int64) * np.asarray(n_b, np.int64)
    status = np.where((status == 0) & (pairs > max_pairs_per_row), 4, status).astype(np.uint8)
    return status, np.where(status == 0, pixels, 0).astype(np.int64), np.where(status == 0, pairs, 0).astype(np.int64)


def compare_batches(pixels, pairs, batch_pixels: int, batch_pairs: int) -> list:
    """consecutive row ranges [(a, b)] whose pixel totals stay within batch_pixels and whose pair totals within batch_pairs; a
    single larger row goes alone"""
    out, a, tot_px, tot_pr = [], 0, 0, 0
    for i, (v, w) in enumerate(zip(np.asarray(pixels, np.int64).tolist(), np.asarray(pairs, np.int64).tolist())):
        if i > a and (tot_px + v > batch_pixels or tot_pr + w > batch_pairs):
            out.append((a, i))
            a, tot_px, tot_pr = i, 0, 0
        tot_px += v
        tot_pr += w
    if len(pixels) > a:
        out.append((a, len(pixels)))
    return out
