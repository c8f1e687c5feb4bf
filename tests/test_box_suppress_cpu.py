"""Duplicate-box suppression (core/processor.py: suppress_duplicate_boxes_*), host side: the native scan of boxes with their
object index and name id, the native emit that drops objects, and the three step functions driven by a test backend whose
device stage is the Python restatement below.  No GPU."""
import io
import json
import os
import random

import numpy as np
import pandas as pd
import pytest

from helpers import OracleBackend
from oracle.steps import pair_iou

from deal_yolo_daya_amd import native_json as nj
from deal_yolo_daya_amd.core import processor as P

COL = P.BBOX_COL


# ----------------------------------------------------------------------------------------------- the definition
def suppress_cell(cell, thr, by_label):
    """What the step computes for one cell: the earlier kept box wins; a cell that loses nothing keeps its text."""
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
    except Exception:
        pass
    kept, removed = [], []
    for k, box, name in boxes:
        for kk, kbox, kname in kept:
            if (not by_label or kname == name):
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


def suppress_rows(box4, row_off, thr, name=None):
    """The device stage restated: (keep, partner) per box of the scanned arrays."""
    box4 = np.asarray(box4, np.float64).reshape(-1, 4).tolist()
    row_off = np.asarray(row_off).tolist()
    name = None if name is None else np.asarray(name).tolist()
    keep = np.ones(len(box4), np.uint8)
    partner = np.full(len(box4), -1, np.int32)
    for r in range(len(row_off) - 1):
        s, e = row_off[r], row_off[r + 1]
        kept = []
        for j in range(s, e):
            x1, y1, x2, y2 = box4[j]
            me = (min(x1, x2), min(y1, y2), max(x1, x2), max(y1, y2))
            for kj, kb in kept:
                if name is not None and name[kj] != name[j]:
                    continue
                if pair_iou(kb, me) >= thr:
                    keep[j] = 0
                    partner[j] = kj - s
                    break
            else:
                kept.append((j, me))
    return keep, partner


def expected_cells(cells, thr, by_label):
    out, removed = [], []
    for i, c in enumerate(cells):
        t, rem = suppress_cell(c, thr, by_label)
        out.append(t)
        removed += [(i, k, kk, iou) for k, kk, iou in rem]
    return out, removed


class SuppressBackend(OracleBackend):
    def suppress_boxes(self, box4, row_off, thr, name=None):
        return suppress_rows(box4, row_off, thr, name)


@pytest.fixture(scope="module")
def be():
    return SuppressBackend()


# ----------------------------------------------------------------------------------------------- known answers
def box(x1, y1, x2, y2, name=None, **extra):
    o = {"polygon": {"ptList": [{"x": x1, "y": y1}, {"x": x2, "y": y2}]}}
    if name is not None:
        o["name"] = name
    o.update(extra)
    return o


def doc(*objs, **top):
    d = {"width": 640, "height": 480}
    d.update(top)
    d["objects"] = list(objs)
    return json.dumps(d, ensure_ascii=False)


BIG = 2 ** 40
KNOWN = {
    "exact_tie": doc(box(0, 0, 100, 100), box(0, 0, 100, 98)),
    "just_under": doc(box(0, 0, 100, 100), box(0, 0, 100, 97.99)),
    "chain": doc(box(0, 0, 100, 100), box(1, 0, 101, 100), box(2, 0, 102, 100)),
    "labels_differ": doc(box(0, 0, 100, 100, "猫"), box(0, 0, 100, 100, "狗")),
    "missing_vs_null": '{"objects": [' + json.dumps(box(0, 0, 10, 10)) + ', {"name": null, "polygon": {"ptList": '
                       '[{"x": 0, "y": 0}, {"x": 10, "y": 10}]}}]}',
    "nan_first": '{"objects": [{"polygon": {"ptList": [{"x": NaN, "y": 0}, {"x": 10, "y": 10}]}}, '
                 '{"polygon": {"ptList": [{"x": 0, "y": 0}, {"x": 10, "y": 10}]}}]}',
    "nan_second": '{"objects": [{"polygon": {"ptList": [{"x": 0, "y": 0}, {"x": 10, "y": 10}]}}, '
                  '{"polygon": {"ptList": [{"x": NaN, "y": 0}, {"x": 10, "y": 10}]}}]}',
    "disjoint": doc(box(0, 0, 10, 10), box(50, 50, 60, 60)),
    "undecodable": '{"objects": [',
    "list_doc": "[1, 2]",
    "interleaved": doc({"name": "poly", "polygon": {"ptList": [{"x": 0, "y": 0}, {"x": 1, "y": 0}, {"x": 1, "y": 1}]}},
                       box(0, 0, 100, 100), "not a dict", box(0, 0, 100, 100), {"name": "kept"}, box(0, 0, 100, 99)),
    "prefix": '{"objects": [' + json.dumps(box(0, 0, 10, 10)) + ', ' + json.dumps(box(0, 0, 10, 10)) +
              ', {"polygon": null}, ' + json.dumps(box(0, 0, 10, 10)) + ']}',
    "big_ints": doc(box(0, 0, BIG, BIG), box(0, 0, BIG, BIG - (BIG // 50) + 1)),
    "big_ints_tie": doc(box(0, 0, BIG + 1, BIG), box(0, 0, BIG, BIG)),
    "non_ascii": doc(box(0, 0, 10, 10, "行人"), box(0, 0, 10, 10, "行人"), note="标注 é中", url="a/b\\c"),
    "escaped": '{"note": "\\u4e2d\\n\\"q\\"", "objects": [' + json.dumps(box(0.5, 0, 1e3, 10)) + ', ' +
               json.dumps(box(0.5, 0, 1e3, 10)) + '], "v": 1E+2}',
    "repeated_key": '{"objects": [], "objects": [' + json.dumps(box(0, 0, 10, 10)) + ', ' + json.dumps(box(0, 0, 10, 10)) + ']}',
    "repeated_name": '{"objects": [{"name": "a", "name": "b", "polygon": {"ptList": [{"x": 0, "y": 0}, {"x": 9, "y": 9}]}}, '
                     + json.dumps(box(0, 0, 9, 9, "b")) + ']}',
    "numeric_name": doc(box(0, 0, 10, 10, 3), box(0, 0, 10, 10, 3)),
    "inf_and_negzero": '{"objects": [{"polygon": {"ptList": [{"x": -0.0, "y": 0}, {"x": Infinity, "y": 10}]}}, '
                       '{"polygon": {"ptList": [{"x": 0, "y": 0}, {"x": Infinity, "y": 10}]}}]}',
    "empty_objects": '{"objects": []}',
    "no_objects": '{"width": 1}',
}


def _known_cells():
    return list(KNOWN.values()) + [float("nan"), None, 7]


@pytest.mark.parametrize("thr", [0.98, 0.5, 0.0, -1.0, 1.0, float("nan")])
@pytest.mark.parametrize("by_label", [False, True])
def test_known_cells(be, thr, by_label):
    cells = _known_cells()
    out, removed = P.suppress_duplicate_boxes_cells(cells, thr, by_label, backend=be)
    want, want_removed = expected_cells(cells, thr, by_label)
    assert [type(c) for c in out] == [type(c) for c in want]
    assert [c if isinstance(c, str) else repr(c) for c in out] == [c if isinstance(c, str) else repr(c) for c in want]
    assert removed == want_removed
    for a, b, w in zip(out, cells, want):
        if w is b:
            assert a is b                                  # untouched cells are the same objects


def test_known_answers_spelled_out(be):
    cells = list(KNOWN.values())
    out, removed = P.suppress_duplicate_boxes_cells(cells, 0.98, False, backend=be)
    got = dict(zip(KNOWN, out))
    rem = {}
    for c, k, kk, iou in removed:
        rem.setdefault(list(KNOWN)[c], []).append((k, kk, iou))
    assert rem["exact_tie"] == [(1, 0, 0.98)]
    assert "just_under" not in rem
    assert rem["chain"] == [(1, 0, pair_iou((0, 0, 100, 100), (1, 0, 101, 100)))]     # A~B, B~C, not A~C: only B goes
    assert json.loads(got["chain"])["objects"] == [box(0, 0, 100, 100), box(2, 0, 102, 100)]
    assert rem["labels_differ"] == [(1, 0, 1.0)]
    assert [k for k, _, _ in rem["interleaved"]] == [3, 5]
    assert [o if not isinstance(o, dict) else o.get("name") for o in json.loads(got["interleaved"])["objects"]] == \
        ["poly", None, "not a dict", "kept"]
    assert rem["prefix"] == [(1, 0, 1.0)]                   # the box after the exception is not a box
    assert "nan_first" not in rem and "nan_second" not in rem
    at0 = P.suppress_duplicate_boxes_cells([KNOWN["nan_first"], KNOWN["nan_second"]], 0.0, backend=be)[1]
    assert at0 == [(0, 1, 0, 0.0)]                          # (NaN box, later): no intersection -> 0.0; (later NaN): NaN
    assert rem["big_ints_tie"][0][:2] == (1, 0)
    assert got["non_ascii"] == json.dumps(json.loads(KNOWN["non_ascii"]) | {"objects": [box(0, 0, 10, 10, "行人")]},
                                          ensure_ascii=False)
    assert got["escaped"] == json.dumps({"note": "中\n\"q\"", "objects": [box(0.5, 0, 1000.0, 10)], "v": 100.0},
                                        ensure_ascii=False)
    assert rem["repeated_key"] == [(1, 0, 1.0)]
    for name in ("disjoint", "undecodable", "list_doc", "empty_objects", "no_objects"):
        assert got[name] is KNOWN[name]
    by_label = P.suppress_duplicate_boxes_cells([KNOWN["labels_differ"], KNOWN["missing_vs_null"], KNOWN["repeated_name"]],
                                                0.98, True, backend=be)[1]
    assert by_label == [(1, 1, 0, 1.0), (2, 1, 0, 1.0)]     # missing == null; the last of a repeated "name" counts


def test_big_int_iou_differs_from_f64(be):
    """ints above 2^53: in f64 the two boxes are the same (IoU 1.0), CPython's exact IoU is N / (N + 1) < 1.0"""
    n = 2 ** 53
    cell = doc(box(0, 0, n + 1, 1), box(0, 0, n, 1))
    assert pair_iou((0.0, 0.0, float(n + 1), 1.0), (0.0, 0.0, float(n), 1.0)) == 1.0
    assert pair_iou((0, 0, n + 1, 1), (0, 0, n, 1)) < 1.0
    stats = {}
    assert P.suppress_duplicate_boxes_cells([cell], 1.0, backend=be, stats=stats) == ([cell], [])
    assert stats["python_cells"] == 1
    out, removed = P.suppress_duplicate_boxes_cells([cell], 0.5, backend=be)
    assert removed == [(0, 1, 0, n / (n + 1))]


def test_string_coordinates_raise(be):
    cell = doc(box("0", "0", "9", "9"), box("0", "0", "9", "9"))
    with pytest.raises(TypeError):
        suppress_cell(cell, 0.98, False)
    with pytest.raises(TypeError):
        P.suppress_duplicate_boxes_cells([doc(box(0, 0, 1, 1)), cell], 0.98, backend=be)


def test_idempotent_and_no_pair_left(be):
    cells = [c for c in _fuzz_cells(400, 3)]
    out, removed = P.suppress_duplicate_boxes_cells(cells, 0.5, backend=be)
    assert removed
    again, removed2 = P.suppress_duplicate_boxes_cells(out, 0.5, backend=be)
    assert removed2 == [] and all(a is b for a, b in zip(again, out))
    assert not P.iou_high_mask(out, 2, 0.5, backend=be).any()


def test_product_backend_is_required(be):
    with pytest.raises(TypeError):
        P.suppress_duplicate_boxes_cells([KNOWN["exact_tie"]], backend=OracleBackend())


# ----------------------------------------------------------------------------------------------- scan / emit fuzz
NAMES = ["person", "行人", "car", "a\"b", "", None, "MISSING"]


def _fuzz_obj(rng):
    r = rng.random()
    if r < 0.06:
        return rng.choice(["x", 3, None, [1, 2]])
    if r < 0.14:
        o = {"polygon": {"ptList": [{"x": rng.randint(0, 50), "y": rng.randint(0, 50)} for _ in range(rng.choice([0, 1, 3, 4]))]}}
    else:
        x, y = rng.randint(0, 40), rng.randint(0, 40)
        w, h = rng.randint(1, 30), rng.randint(1, 30)
        pts = [{"x": x, "y": y}, {"x": x + w, "y": y + h}]
        if rng.random() < 0.3:
            pts = pts[::-1]
        if rng.random() < 0.2:
            pts = [{"x": p["x"] + 0.5, "y": p["y"] * 1.0} for p in pts]
        if rng.random() < 0.02:
            pts[0]["x"] = float("nan")
        o = {"polygon": {"ptList": pts, "type": "rect"}}
    name = rng.choice(NAMES)
    if name != "MISSING":
        o["name"] = name
    if rng.random() < 0.2:
        o["attrs"] = {"occluded": rng.random() < 0.5, "note": "备注"}
    keys = list(o)
    rng.shuffle(keys)
    return {k: o[k] for k in keys}


def _fuzz_cells(n, seed):
    rng = random.Random(seed)
    cells = []
    for _ in range(n):
        objs = [_fuzz_obj(rng) for _ in range(rng.choice([0, 1, 2, 3, 5, 8, 20]))]
        base = objs[:]
        for o in base:                                      # exact and near duplicates
            if isinstance(o, dict) and rng.random() < 0.3:
                objs.insert(rng.randrange(len(objs) + 1), json.loads(json.dumps(o)))
        d = {"width": 640, "objects": objs, "height": 480}
        cells.append(json.dumps(d, ensure_ascii=rng.random() < 0.3))
    return cells


def _python_walk(cell):
    """(box corners as scanned, object index, name) per box of one cell, by §1's walk"""
    out = []
    try:
        d = json.loads(cell)
        for k, obj in enumerate(d.get("objects", [])):
            if not isinstance(obj, dict):
                continue
            pts = obj.get("polygon", {}).get("ptList", [])
            if len(pts) != 2:
                continue
            a, b = pts
            if not (isinstance(a, dict) and isinstance(b, dict) and "x" in a and "y" in a and "x" in b and "y" in b):
                continue
            min(a["x"], b["x"]), min(a["y"], b["y"])
            out.append(([a["x"], a["y"], b["x"], b["y"]], k, obj.get("name")))
    except Exception:
        pass
    return out


@pytest.mark.parametrize("views", [False, True])
def test_scan_fuzz(views):
    cells = _fuzz_cells(600, 11) + list(KNOWN.values()) + [None, float("nan")]
    if views:
        scan = nj.scan_box_objects(cells)
    else:
        data, off, missing, keep = nj.cells_to_buffers(cells)
        scan = nj.scan_box_objects_buffers(data, off, missing, keep=keep)
    try:
        irregular = {i for i in range(len(cells)) if scan.status[i] == nj.IRREGULAR}
        want_irregular = {list(KNOWN).index(k) + 600 for k in ("big_ints", "big_ints_tie", "repeated_key", "repeated_name",
                                                                "numeric_name")}
        assert want_irregular <= irregular
        assert all(i >= 600 for i in irregular)             # generated cells are regular
        for i, cell in enumerate(cells):
            s, e = scan.row_off[i], scan.row_off[i + 1]
            if i in irregular or not isinstance(cell, str):
                assert s == e
                continue
            walk = _python_walk(cell)
            assert e - s == len(walk), cell
            got = scan.box4[s:e]
            np.testing.assert_array_equal(got, np.asarray([w[0] for w in walk], np.float64).reshape(-1, 4))
            assert scan.box_object[s:e].tolist() == [w[1] for w in walk]
            ids = scan.box_name[s:e].tolist()
            names = [w[2] for w in walk]
            for a in range(len(walk)):
                assert (ids[a] == -1) == (names[a] is None)
                for b in range(len(walk)):
                    assert (ids[a] == ids[b]) == (names[a] == names[b])
    finally:
        scan.close()


def test_emit_fuzz():
    rng = np.random.default_rng(5)
    cells = _fuzz_cells(500, 23) + [KNOWN["non_ascii"], KNOWN["escaped"], KNOWN["interleaved"], KNOWN["prefix"]]
    scan = nj.scan_box_objects(cells)
    try:
        drop = (rng.random(scan.n_boxes) < 0.3).astype(np.uint8)
        changed, texts = scan.emit_dropping(drop)
        texts = iter(texts)
        for i, cell in enumerate(cells):
            s, e = scan.row_off[i], scan.row_off[i + 1]
            gone = set(scan.box_object[s:e][drop[s:e] != 0].tolist())
            if not gone:
                assert changed[i] == 0
                continue
            assert changed[i] == 1
            d = json.loads(cell)
            d["objects"] = [o for k, o in enumerate(d["objects"]) if k not in gone]
            assert next(texts) == json.dumps(d, ensure_ascii=False)
    finally:
        scan.close()


# ----------------------------------------------------------------------------------------------- step functions
def _table(n, seed):
    cells = _fuzz_cells(n, seed)
    cells[3] = float("nan")
    cells[5] = KNOWN["big_ints_tie"]
    cells[7] = KNOWN["undecodable"]
    cells[9] = KNOWN["repeated_key"]
    return pd.DataFrame({"source": [f"s{i}.jpg" for i in range(n)], P.ANNOTATION_COL: ["{}"] * n, COL: cells,
                         "width": 640, "height": 480})


@pytest.mark.parametrize("by_label", [False, True])
def test_frame(be, by_label):
    df = _table(300, 7)
    stats = {}
    out, removed = P.suppress_duplicate_boxes_frame(df, 0.7, by_label, backend=be, stats=stats)
    want, want_removed = expected_cells(df[COL].tolist(), 0.7, by_label)
    assert out.drop(columns=[COL]).equals(df.drop(columns=[COL]))
    assert [c if isinstance(c, str) else None for c in out[COL]] == [c if isinstance(c, str) else None for c in want]
    assert list(removed.columns) == ["source", "row", "object", "kept_object", "iou"]
    assert list(zip(removed["row"], removed["object"], removed["kept_object"], removed["iou"])) == want_removed
    assert removed["source"].tolist() == [f"s{r}.jpg" for r, *_ in want_removed]
    assert stats["rows"] == 300 and stats["boxes_removed"] == len(want_removed) and stats["python_cells"] >= 2
    assert stats["rows_changed"] == sum(a is not b for a, b in zip(want, df[COL].tolist()))


def test_csv_matches_pandas_route(be, tmp_path):
    df = _table(300, 8)
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    out_csv, rem_csv = tmp_path / "o" / "out.csv", tmp_path / "o" / "removed.csv"
    res = P.suppress_duplicate_boxes_csv(src, out_csv, rem_csv, 0.7, backend=be)
    assert P.LAST_IO_PATH["suppress"] == "native"
    back = pd.read_csv(src, encoding="utf-8-sig")
    want, want_removed = expected_cells(back[COL].tolist(), 0.7, False)
    back[COL] = pd.Series(want, dtype=object)
    buf = io.StringIO()
    back.to_csv(buf, index=False)
    assert out_csv.read_bytes() == b"\xef\xbb\xbf" + buf.getvalue().encode("utf-8")
    assert res == {"rows": 300, "rows_changed": sum(1 for a, b in zip(want, df[COL]) if a is not b and isinstance(a, str)
                                                    and a != b),
                   "boxes_removed": len(want_removed), "output": out_csv, "removed_output": rem_csv}
    rem = pd.read_csv(rem_csv, encoding="utf-8-sig")
    assert list(zip(rem["row"], rem["object"], rem["kept_object"])) == [r[:3] for r in want_removed]


def test_csv_errors(be, tmp_path, capsys):
    assert P.suppress_duplicate_boxes_csv(tmp_path / "nope.csv", tmp_path / "o.csv", backend=be) is None
    assert "读取失败：" in capsys.readouterr().out
    p = tmp_path / "x.csv"
    pd.DataFrame({"a": [1, 2]}).to_csv(p, index=False, encoding="utf-8-sig")
    assert P.suppress_duplicate_boxes_csv(p, tmp_path / "o.csv", backend=be) is None
    assert f"错误：缺少必要列 {COL}" in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "o.csv")
