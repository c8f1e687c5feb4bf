"""COCO export (K16) on the host: fix2 against exact arithmetic, the definition's worked answers, the file the frame / CSV /
workbook entries write, and the agreement with the polygon audit.  The device stage is a stand-in built on tests/coco_ref.py;
tests/test_gpu_coco.py checks K16 itself."""
import json
import math
import random
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import coco_ref as C
import polygon_audit_ref as R
import yolo_seg_ref as S
from helpers import OracleBackend
from test_polygon_audit_cpu import PolyBackend, _table, cell, ob
from test_yolo_host_cpu import _Sheets
from test_yolo_seg_cpu import SegBackend, _frames, fuzz_cells

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd.core import processor as P
from deal_yolo_daya_amd.core import utils as U


class CocoBackend(PolyBackend, SegBackend):
    def coco_annotations(self, xy, pt_off, row_off, cat_id, width, height, status, image_id_base=1, ann_id_base=1, flags=1):
        return C.coco_arrays(xy, pt_off, row_off, cat_id, width, height, status, image_id_base, ann_id_base, flags)


BE = CocoBackend()


# ------------------------------------------------------------------ fix2
def exact2(v):
    """ "%.2f" by exact arithmetic: round-half-even of the binary value times 100"""
    q = Fraction(v) * 100
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return f"{n // 100}.{n % 100:02d}"


def test_fix2_is_exact():
    rnd = random.Random(7)
    top = math.nextafter(2.0 ** 43, 0.0)
    vals = [0.0, C.clamp(-0.0, 5.0), 0.005, 0.015, 0.125, 0.375, 2.5, 9.994999999999999, 9.995, 9.996, 99.995, 999.995, 0.995, 0.994,
            1e-9, 0.004999999999999999, top, 2.0 ** 43 - 0.5, 2.0 ** 42 + 0.125, 1234567.125, 8796093022207.99]
    vals += [k + 0.125 for k in range(40)] + [k + 0.375 for k in range(40)] + [k / 8 for k in range(100)]     # exact ties
    for _ in range(2000):
        k = rnd.randrange(0, 10 ** rnd.randint(1, 9))
        vals.append(k * 0.005)                                                                # decimal ties, inexact in binary
        vals.append(rnd.uniform(0, 10 ** rnd.randint(0, 12)))
        vals.append(float(10 ** rnd.randint(0, 12)) - 0.005)                                  # digit boundaries
    vals += [v for b in list(vals) for v in (math.nextafter(b, 0.0), math.nextafter(b, math.inf)) if 0.0 <= v < 2.0 ** 43]
    assert str(vals[1]) == "0.0"                              # the clamp leaves no -0.0
    lengths = set()
    for v in vals:
        want = exact2(v)
        assert C.fix2(v) == want == "%.2f" % v, v
        n = int(want.replace(".", ""))
        assert len(want) == max(len(str(n)), 3) + 1
        lengths.add(len(want))
    assert {C.fix2(9.994999999999999), C.fix2(9.995), C.fix2(9.996)} == {"9.99", "10.00"}      # rounding adds a digit
    assert C.fix2(top) == "8796093022208.00" and lengths >= set(range(4, 17))


# ------------------------------------------------------------------ worked answers
HEAD = '{"id":1,"image_id":1,"category_id":1,'
WORKED = [
    ("inside", [(10, 10), (50, 10), (50, 50)], 0,
     '"bbox":[10.00,10.00,40.00,40.00],"area":800.00,"iscrowd":0,"segmentation":[[10.00,10.00,50.00,10.00,50.00,50.00]]}'),
    ("crossing", [(-10, 10), (50, 10), (50, 50)], 1,
     '"bbox":[0.00,10.00,50.00,40.00],"area":1166.67,"iscrowd":0,"segmentation":[[0.00,10.00,50.00,10.00,50.00,50.00,0.00,16.67]]}'),
    ("two_points", [(30, 60), (10, 20)], 0,
     '"bbox":[10.00,20.00,20.00,40.00],"area":800.00,"iscrowd":0,"segmentation":[[10.00,20.00,30.00,20.00,30.00,60.00,10.00,60.00]]}'),
    ("bow_tie", [(0, 0), (10, 10), (10, 0), (0, 10)], 0,
     '"bbox":[0.00,0.00,10.00,10.00],"area":0.00,"iscrowd":0,"segmentation":[[0.00,0.00,10.00,10.00,10.00,0.00,0.00,10.00]]}'),
]


@pytest.mark.parametrize("name,pts,code,tail", WORKED)
def test_worked_answers(name, pts, code, tail, tmp_path):
    raw = [(float(x), float(y)) for x, y in pts]
    got = C.polygon(raw, 100.0, 100.0, 1, 1, 1)
    assert got[:2] == (code, HEAD + tail)
    detect = C.polygon(raw, 100.0, 100.0, 1, 1, 1, segmentation=False)[1]
    assert detect == HEAD + tail[:tail.index('"segmentation"')] + '"segmentation":[]}'
    res = P.export_coco_frame(pd.DataFrame({P.ANNOTATION_COL: [cell(ob("k", pts))], "width": [100], "height": [100]}),
                              tmp_path / "w.json", backend=BE)
    doc = json.load(open(res["output"], encoding="utf-8"))
    assert doc["annotations"] == [json.loads(HEAD + tail)] and res["annotations"] == 1
    assert doc["images"] == [{"id": 1, "width": 100, "height": 100, "file_name": "0"}]
    assert doc["categories"] == [{"id": 1, "name": "k", "supercategory": ""}]


def _wound(times, side):
    return [(0.0, 0.0), (side, 0.0), (side, side), (0.0, side)] * times


def test_one_polygon_per_action(tmp_path):
    side = float(2 ** 21)
    c = cell(ob("a", [(10, 10), (50, 10), (50, 50)]),                 # written
             ob("a", [(-10, 10), (50, 10), (50, 50)]),                # clipped
             ob("b", [(10, float("inf")), (50, 10), (50, 50)]),       # bad_coords
             ob("b", [(10, 10)]),                                     # too_few_points
             ob("c", [(-200, -200), (-300, -200), (-300, -300)]),     # empty: outside the image
             ob("a", _wound(4, side)),                                # too_large: four turns round the image, 2^44
             ob("a", _wound(1, side)),                                # written: 2^42
             {"name": 7, "polygon": {"ptList": [{"x": 1, "y": 1}]}})  # unmatchable
    df = pd.DataFrame({"source": ["s0", "s1"], P.ANNOTATION_COL: [c, cell(ob("a", [(1, 1), (5, 5)]))],
                       "width": [side, None], "height": [side, 100]})
    res = P.export_coco_frame(df, tmp_path / "a.json", skipped_csv=str(tmp_path / "skipped.csv"), backend=BE)
    assert [res[a] for a in P.COCO_ACTIONS] == [2, 1, 1, 1, 1, 1, 1]
    assert (res["polygons"], res["unmatchable_name_polygons"], res["annotations"], res["rows_no_size"], res["images"]) == (9, 1, 3, 1, 1)
    assert C.polygon(_wound(4, side), side, side, 1, 1, 1)[0] == C.TOO_LARGE and R.area(_wound(4, side)) == 2.0 ** 44
    doc = json.load(open(res["output"], encoding="utf-8"))
    assert [a["id"] for a in doc["annotations"]] == [1, 2, 7] and doc["annotations"][2]["area"] == 2.0 ** 42
    assert [c["name"] for c in doc["categories"]] == ["a", "b", "c"]
    sk = pd.read_csv(res["skipped_output"], encoding="utf-8-sig")
    assert sk["action"].tolist() == ["bad_coords", "too_few_points", "empty", "too_large", "no_size"]
    assert sk["object"].tolist() == [2, 3, 4, 5, 0] and sk["row"].tolist() == [0, 0, 0, 0, 1] and sk["source"].tolist()[-1] == "s1"


# ------------------------------------------------------------------ the file against the restatement
def restate(cells, ws, hs, labels=None, classes=None, segmentation=True):
    """the annotation texts, categories and action counts of a table from CPython's json and coco_ref.polygon"""
    cat_of = {c: k + 1 for k, c in enumerate(classes)} if classes is not None else {}
    texts, counts, kept_rows, index = [], [0] * 7, set(), 0
    for i, c in enumerate(cells):
        st, W, H = P._audit_size_py(ws[i], hs[i]) if ws is not None else (1, 0.0, 0.0)
        W, H = (S.size_of(W), S.size_of(H)) if st == 0 else (None, None)
        for _, name, pts in fl.seg_cell_polygons(c):
            index += 1
            if not isinstance(name, str) or (labels is not None and name != str(labels[i])):
                continue
            if classes is not None and name not in cat_of:
                continue
            cat = cat_of.setdefault(name, len(cat_of) + 1)
            raw = [(P._audit_number(x), P._audit_number(y)) for x, y in pts]
            code, text, _ = C.polygon(raw, W, H, index, i + 1, cat, segmentation)
            counts[code] += 1
            if text is not None:
                texts.append(text)
                kept_rows.add(i)
    return texts, cat_of, counts, kept_rows


def annotations_text(path):
    data = open(path, "rb").read()
    a, b = data.index(b'"annotations":[') + 15, data.index(b'],"images":[')
    return data[a:b].decode("ascii")


def check_file(path, cells, ws, hs, **kw):
    texts, cat_of, counts, _ = restate(cells, ws, hs, **kw)
    assert annotations_text(path) == ",".join(texts)
    doc = json.load(open(path, encoding="utf-8"))
    assert set(doc) == {"info", "licenses", "annotations", "images", "categories"} and "date" not in json.dumps(doc["info"])
    ids = [a["id"] for a in doc["annotations"]]
    assert ids == sorted(set(ids))
    images = {im["id"]: im for im in doc["images"]}
    cats = {c["id"]: c["name"] for c in doc["categories"]}
    assert cats == {k: nm for nm, k in cat_of.items()} and len(images) == len(doc["images"])
    for a in doc["annotations"]:
        im = images[a["image_id"]]
        assert a["category_id"] in cats and a["iscrowd"] == 0
        x, y, w, h = a["bbox"]
        assert 0 <= x and 0 <= y and w >= 0 and h >= 0 and x + w <= im["width"] + 0.011 and y + h <= im["height"] + 0.011
        for ring in a["segmentation"]:
            assert len(ring) % 2 == 0 and len(ring) >= 6
    return doc, counts


def _fuzz_frame(n, seed):
    rnd = random.Random(seed)
    cells = fuzz_cells(n, seed)                           # irregular cells, None, lone surrogates, str and huge coordinates
    return pd.DataFrame({"source": [f"s{k}.png" for k in range(len(cells))], P.ANNOTATION_COL: np.asarray(cells, object),
                         "width": [rnd.choice([300, 300, 100, 120.5, 300, 0, None, -3, float("nan"), 2.0 ** 43]) for _ in cells],
                         "height": [rnd.choice([300, 60, 100, 300, 300, 0, float("inf")]) for _ in cells],
                         "label": [rnd.choice(["a", "a", "猫", "zz"]) for _ in cells]})


def test_frame_file_on_fuzz_cells(tmp_path):
    df = _fuzz_frame(900, 31)
    cells, ws, hs = df[P.ANNOTATION_COL].tolist(), df["width"].tolist(), df["height"].tolist()
    assert any("\ud800" in c for c in cells if isinstance(c, str))
    stats = {}
    res = P.export_coco_frame(df, tmp_path / "f.json", backend=BE, stats=stats)
    doc, counts = check_file(res["output"], cells, ws, hs)
    assert stats == res and [res[a] for a in P.COCO_ACTIONS] == counts and res["python_cells"] > 0
    assert res["annotations"] == len(doc["annotations"]) > 50 and min(counts[:6]) > 0 and counts[6] == 0
    assert any("\ud800" in c["name"] for c in doc["categories"]) and any(c["name"] == "猫" for c in doc["categories"])
    assert res["images"] == len(doc["images"]) == res["rows"] - res["rows_no_size"]
    assert {im["file_name"] for im in doc["images"]} <= set(df["source"]) and not (tmp_path / "f.json.tmp").exists()
    assert any(isinstance(im["width"], float) for im in doc["images"]) and any(isinstance(im["width"], int) for im in doc["images"])


def test_frame_options(tmp_path, monkeypatch):
    df = _fuzz_frame(400, 32)
    cells, ws, hs, labels = (df[k].tolist() for k in (P.ANNOTATION_COL, "width", "height", "label"))
    res = P.export_coco_frame(df, tmp_path / "l.json", label_col="label", backend=BE)
    doc, _ = check_file(res["output"], cells, ws, hs, labels=labels)
    assert 0 < len(doc["annotations"]) and {c["name"] for c in doc["categories"]} <= {"a", "猫"}
    res = P.export_coco_frame(df, tmp_path / "c.json", classes=["猫", "a"], backend=BE)
    doc, counts = check_file(res["output"], cells, ws, hs, classes=["猫", "a"])
    assert doc["categories"][0] == {"id": 1, "name": "猫", "supercategory": ""} and res["unknown_class"] > 0
    assert res["unknown_class"] + sum(counts) + res["unmatchable_name_polygons"] == res["polygons"]
    names = [f"img/{k:05d}.jpg" for k in range(len(df))]
    res = P.export_coco_frame(df, tmp_path / "e.json", keep_empty_images=False, file_names=names, segmentation=False, backend=BE)
    doc, _ = check_file(res["output"], cells, ws, hs, segmentation=False)
    kept_rows = restate(cells, ws, hs)[3]
    assert [im["id"] for im in doc["images"]] == [i + 1 for i in sorted(kept_rows)] and res["images"] < res["rows"] - res["rows_no_size"]
    assert all(im["file_name"] == names[im["id"] - 1] for im in doc["images"]) and all(a["segmentation"] == [] for a in doc["annotations"])
    whole = open(P.export_coco_frame(df, tmp_path / "w.json", backend=BE)["output"], "rb").read()
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 37)       # chunk edges: ids, categories and commas carry over
    assert open(P.export_coco_frame(df, tmp_path / "k.json", backend=BE)["output"], "rb").read() == whole
    with pytest.raises(ValueError):
        P.export_coco_frame(df, tmp_path / "x.json", label_col="nope", backend=BE)
    with pytest.raises(ValueError):
        P.export_coco_frame(df, tmp_path / "x.json", file_names=names[:-1], backend=BE)
    assert not (tmp_path / "x.json").exists()


def test_empty_frame_and_no_size_columns(tmp_path):
    res = P.export_coco_frame(pd.DataFrame({P.ANNOTATION_COL: [], "width": [], "height": []}), tmp_path / "e.json", backend=BE)
    doc = json.load(open(res["output"], encoding="utf-8"))
    assert (doc["annotations"], doc["images"], doc["categories"], res["rows"], res["annotations"]) == ([], [], [], 0, 0)
    res = P.export_coco_frame(pd.DataFrame({P.ANNOTATION_COL: [cell(ob("a", [(1, 1), (5, 5), (1, 5)]), ob("b", [(1, 1), (5, 5)]))]}),
                              tmp_path / "n.json", backend=BE)
    doc = json.load(open(res["output"], encoding="utf-8"))
    assert (doc["annotations"], doc["images"], res["no_size"], res["rows_no_size"]) == ([], [], 2, 1)
    assert [c["name"] for c in doc["categories"]] == ["a", "b"]


def test_backend_without_the_method(tmp_path):
    df = pd.DataFrame({P.ANNOTATION_COL: [cell(ob("a", [(1, 1), (5, 5)]))]})
    with pytest.raises(TypeError, match="coco_annotations"):
        P.export_coco_frame(df, tmp_path / "x.json", backend=PolyBackend())
    with pytest.raises(TypeError, match="coco_annotations"):
        P.export_coco_from_excels([], tmp_path, backend=OracleBackend())


def test_id_bases_are_checked():
    t = (np.zeros(0), np.zeros(1, np.int32), np.zeros(2, np.int32), np.zeros(0, np.int32), np.ones(1), np.ones(1), np.zeros(1, np.uint8))
    assert C.coco_arrays(*t, 2 ** 53 - 2, 2 ** 53 - 1)[3] == b""
    for bases in ((-1, 1), (1, -1), (2 ** 53 - 1, 1), (1, 2 ** 53)):
        with pytest.raises(ValueError):
            C.coco_arrays(*t, *bases)


# ------------------------------------------------------------------ against the polygon audit
def test_actions_and_areas_equal_the_audit():
    extra = [cell(ob("a", [(10, 10), (50, 10), (50, 50)]), ob("b", [(1, 1), (2, float("nan")), (3, 3)])), cell(ob("b", [(5, 5), (9, 50)]))]
    df = pd.concat([_table(900, 5), pd.DataFrame({"source": ["x", "y"], P.ANNOTATION_COL: extra, "width": [100, 100],
                                                  "height": [100, 100]})], ignore_index=True)
    cells = df[P.ANNOTATION_COL].to_numpy()
    status, W, H = P._audit_sizes(df["width"].to_numpy(), df["height"].to_numpy(), len(df))
    row_off, xy, pt_off, obj, cls, names, _ = P._poly_chunk(cells)
    cat, _, area, _, _ = BE.audit_polygons(xy, pt_off, row_off, cls, W, H, status, len(names))
    action, carea, kept, text = BE.coco_annotations(xy, pt_off, row_off, np.where(cls >= 0, cls + 1, 0), W, H, status)
    assert np.array_equal(action, cat) and set(action.tolist()) >= {0, 1, 2, 3, 4, 5, 255}
    assert np.array_equal(np.isnan(carea), np.isnan(area)) and np.array_equal(carea[action <= 1], area[action <= 1])
    assert kept.sum() == (action <= 1).sum() == text.count(b'{"id":')
    audit = P.audit_polygons_frame(df, backend=BE)
    res_counts = np.bincount(action[action != 255], minlength=6)
    assert [audit.totals[a] for a in P.SEG_ACTIONS] == res_counts.tolist()


# ------------------------------------------------------------------ the CSV entry
def test_csv_native_and_pandas_paths(tmp_path, monkeypatch):
    df = _table(500, 8)
    df["label"] = ["a" if k % 2 else "b" for k in range(len(df))]
    path = tmp_path / "t.csv"
    df.to_csv(path, index=False, encoding="utf-8-sig")
    a = P.export_coco_csv(str(path), tmp_path / "a.json", label_col="label", skipped_csv=str(tmp_path / "a.csv"), backend=BE)
    assert P.LAST_IO_PATH["coco_export"] == "native" and a["annotations"] > 0
    monkeypatch.setattr(P._fc, "enabled", lambda: False)
    b = P.export_coco_csv(str(path), tmp_path / "b.json", label_col="label", skipped_csv=str(tmp_path / "b.csv"), backend=BE)
    assert P.LAST_IO_PATH["coco_export"] == "pandas"
    assert open(a["output"], "rb").read() == open(b["output"], "rb").read()
    assert open(a["skipped_output"], "rb").read() == open(b["skipped_output"], "rb").read()
    drop = ("output", "skipped_output", "python_cells")
    assert {k: v for k, v in a.items() if k not in drop} == {k: v for k, v in b.items() if k not in drop}
    check_file(a["output"], df[P.ANNOTATION_COL].tolist(), df["width"].tolist(), df["height"].tolist(), labels=df["label"].tolist())
    monkeypatch.undo()
    assert P.export_coco_csv(str(path), tmp_path / "c.json", json_col="nope", backend=BE) is None
    assert P.export_coco_csv(str(tmp_path / "missing.csv"), tmp_path / "c.json", backend=BE) is None


# ------------------------------------------------------------------ the workbooks
def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file() and "annotations" not in p.parts}


@pytest.mark.parametrize("segmentation", [True, False])
def test_export_coco_from_excels(tmp_path, segmentation):
    frames = _frames(tmp_path, True)
    frames["train"].loc[3, "source"] = None                  # left out: no source
    frames["train"].loc[5, "分类标签"] = None                  # left out: its label "None" is not among the classes
    book = tmp_path / "cat.xlsx"
    book.write_bytes(b"")
    out = tmp_path / "out"
    with _Sheets(frames):
        first = P.export_coco_from_excels([str(book)], str(out), segmentation=segmentation, backend=BE)   # before any image exists
        before = {str(p): p.read_bytes() for p in first["outputs"]}
        yolo = P.generate_yolo_datasets_from_excels([str(book)], str(out), download_images=False, backend=BE,
                                                    task="segment" if segmentation else "detect")
        tree = _tree(out)
        res = P.export_coco_from_excels([str(book)], str(out), segmentation=segmentation, backend=BE)
        assert _tree(out) == tree                            # the dataset step's outputs are untouched
    ds = yolo["datasets"][0]
    assert [str(p) for p in res["outputs"]] == [str(ds / "annotations" / f"instances_{sp}.json") for sp in ("train", "val")]
    assert {str(p): p.read_bytes() for p in res["outputs"]} == before
    import yaml
    names = yaml.safe_load((ds / "data.yaml").read_text(encoding="utf-8"))["names"]
    for sp, path in zip(("train", "val"), res["outputs"]):
        doc = json.load(open(path, encoding="utf-8"))
        assert [(c["id"], c["name"]) for c in doc["categories"]] == [(k + 1, nm) for k, nm in enumerate(names)]
        written = sorted(p.name for p in (ds / "images" / sp).iterdir())
        assert sorted(im["file_name"] for im in doc["images"]) == written and len(written) > 0
        by_image = {im["id"]: im["file_name"] for im in doc["images"]}
        for a in doc["annotations"]:
            assert (a["segmentation"] != []) == segmentation
            if segmentation:                                 # K13 printed the same polygon: the label file holds the YOLO class id
                label = (ds / "labels" / sp / (by_image[a["image_id"]].rsplit(".", 1)[0] + ".txt")).read_text()
                assert {int(line.split()[0]) for line in label.splitlines()} == {a["category_id"] - 1}
        assert len(doc["annotations"]) == res["stats"]["cat"][sp]["annotations"] > 0
    assert res["stats"]["cat"]["train"]["rows_invalid_label"] == 1 and res["stats"]["cat"]["val"]["rows_invalid_label"] == 0
    assert res["stats"]["cat"]["train"]["rows_without_source"] == 1 and res["stats"]["cat"]["val"]["rows_without_source"] == 0
    assert U._safe_image_stem(str(tmp_path / "img" / "r1.jpg"), 4) == "r1_4"
    assert P._coco_image_suffix(tmp_path / "none", "x_1", "http://h/p/x.PNG?sig=a.b") == ".PNG"
    assert P._coco_image_suffix(tmp_path / "none", "x_1", "http://h/p/x") == ".jpg"
