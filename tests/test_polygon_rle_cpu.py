"""COCO run-length masks (core/processor.py: polygon_rle and export_coco_frame(segmentation="rle"); core/utils.py: rle_to_mask
and mask_to_rle), host side, and the K23 rule as restated in tests/polygon_rle_ref.py: the string codec against a known answer
of pycocotools and on its boundary values, the box-restricted coverage against the whole-image rule, the runs against the
masks, the kernel's mapping against the rule — driven by a test backend whose device stage is the restatement;
tests/test_gpu_polygon_rle.py checks K23 itself.  No GPU."""
import json
import os

import numpy as np
import pandas as pd
import pytest

import polygon_raster_ref as K21
import polygon_rle_ref as R
from helpers import OracleBackend
from test_coco_cpu import CocoBackend

from deal_yolo_daya_amd.core import processor as P
from deal_yolo_daya_amd.core import utils as U

COL = P.ANNOTATION_COL
EDGE_VALUES = (0, 1, 15, 16, 31, 32, 511, 512, 1 << 20, (1 << 30) - 1, 1 << 30)


class RleBackend(CocoBackend):
    def __init__(self):
        self.calls = 0

    def polygon_rle(self, xy, pt_off, row_off, sel, width, height, max_pixels_per_row=1 << 26):
        self.calls += 1
        return R.rle_arrays(xy, pt_off, row_off, sel, width, height, max_pixels_per_row)


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def random_polygon(rng, trial, w, h):
    m = int(rng.integers(2, 9))
    pts = rng.uniform(-4.0, max(w, h) + 4.0, (m, 2))
    if trial % 3 == 0:
        pts = np.round(pts)
    if trial % 11 == 0:
        pts = np.array([[0.0, 0.0], [w, h]]) if trial % 22 else np.array([[-3.0, -2.0], [w + 5.0, h + 1.0]])
    return pts


# ----------------------------------------------------------------------------------------------- the string
def test_known_answer_of_pycocotools():
    runs, text = [6, 1, 40, 4, 5, 4, 5, 4, 21], b"61X13mN000`0"
    assert R.enc(runs) == text and R.dec(text) == runs
    assert U.rle_runs_to_string(runs) == text and U.rle_string_to_runs(text).tolist() == runs
    mask = U.rle_to_mask(text.decode(), [9, 10])
    assert mask.shape == (9, 10) and mask.sum() == 13 and np.array_equal(mask, R.decode(runs, 10, 9))
    assert np.array_equal(U.rle_to_mask(runs, [9, 10]), mask) and np.array_equal(U.rle_to_mask(text, (9, 10)), mask)
    assert U.mask_to_rle(mask) == {"size": [9, 10], "counts": text.decode()}


def test_codec_on_its_boundary_values():
    rng = np.random.default_rng(3)
    assert len(R.enc([1 << 30])) == 7 and len(R.enc([0])) == 1 and len(R.enc([15])) == 1 and len(R.enc([16])) == 2
    assert len(R.enc([5, 1, 2, 1 << 30, 1, 0])) == 1 + 1 + 1 + 7 + 1 + 7        # the last: 0 - 2^30, a negative delta in 7 bytes
    for v in EDGE_VALUES:
        for lead in ([], [3], [3, 4], [3, 4, 5]):                               # the run with and without a delta
            runs = lead + [v]
            assert R.dec(R.enc(runs)) == runs and U.rle_runs_to_string(runs) == R.enc(runs)
    seen_negative = seen_seven = 0
    for trial in range(300):
        runs = rng.choice(EDGE_VALUES, int(rng.integers(1, 12))).tolist()
        text = R.enc(runs)
        assert R.dec(text) == runs and U.rle_string_to_runs(text).tolist() == runs and U.rle_runs_to_string(runs) == text
        assert all(48 <= b < 112 for b in text) and len(text) <= 7 * len(runs)
        deltas = [c - runs[i - 2] if i > 2 else c for i, c in enumerate(runs)]
        seen_negative += any(d < 0 for d in deltas)
        seen_seven += any(d >= 1 << 29 or d < -(1 << 29) for d in deltas)
    assert seen_negative > 50 and seen_seven > 50
    assert b"\\" in R.enc([44 + 32 * 3])                                       # the alphabet holds the backslash: JSON escapes it
    with pytest.raises(ValueError):
        U.rle_to_mask([3, 4], [2, 2])
    with pytest.raises(ValueError):
        U.rle_string_to_runs("P")                                               # a continuation byte at the end


# ----------------------------------------------------------------------------------------------- the rule
def test_the_box_holds_everything_the_rule_covers():
    rng = np.random.default_rng(5)
    for trial in range(300):
        w, h = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        pts = random_polygon(rng, trial, w, h)
        assert np.array_equal(R.box_cover_full(pts, w, h), K21.cover(pts, w, h)), trial


def test_runs_decode_to_the_cover():
    rng = np.random.default_rng(6)
    kinds = set()
    for trial in range(300):
        w, h = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        pts = random_polygon(rng, trial, w, h)
        full = K21.cover(pts, w, h)
        runs, area, box = R.polygon_runs(pts, w, h)
        assert sum(runs) == w * h and all(r > 0 for r in runs[1:]) and runs[0] >= 0
        assert np.array_equal(R.decode(runs, w, h), full) and np.array_equal(U.rle_to_mask(R.enc(runs), [h, w]), full)
        assert U.mask_to_rle(full)["counts"].encode() == R.enc(runs)
        assert area == full.sum()
        ys, xs = np.nonzero(full)
        assert box == ((xs.min(), ys.min(), np.ptp(xs) + 1, np.ptp(ys) + 1) if area else (0, 0, 0, 0))
        kinds.add("full" if full.all() else "none" if not full.any() else "first" if full[0, 0] else "some")
    assert kinds == {"full", "none", "first", "some"}


def test_column_continuation_by_hand():
    assert R.polygon_runs([(1, 0), (3, 3)], 4, 3)[0] == [3, 6, 3]               # two full columns are one run
    assert R.polygon_runs([(0, 0), (4, 3)], 4, 3)[0] == [0, 12]
    assert R.polygon_runs([(9, 9), (12, 12)], 4, 3)[0] == [12]
    assert R.polygon_runs([(1, 0), (3, 2)], 4, 3)[0] == [3, 2, 1, 2, 4]         # a line short of the bottom: two runs
    assert R.polygon_runs([(1, 1), (3, 3)], 4, 3)[0] == [4, 2, 1, 2, 3]         # bottom covered, the next top not


@pytest.mark.parametrize("strip, capacity, band", [(1024, 256, 64), (64, 256, 5), (17, 3, 2), (5, 1, 1)])
def test_the_kernels_mapping_changes_nothing(strip, capacity, band):
    rng = np.random.default_rng(8)
    for trial in range(150):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 20))
        pts = random_polygon(rng, trial, w, h)
        assert R.runs_by_items(pts, w, h, strip, capacity, band) == R.polygon_runs(pts, w, h)[0], trial
    for w in (64, 65, 130):                                                     # full-height columns across lanes 63 | 64 and strips
        for pts in ([(62, 0), (66, 3)], [(0, 0), (w, 3)], [(63, 0), (64, 3)], [(w - 1, 0), (w, 3)], [(16, 0), (18, 3)]):
            assert R.runs_by_items(pts, w, 3, strip, capacity, band) == R.polygon_runs(pts, w, 3)[0], (w, pts)


def test_every_output_of_the_restatement():
    xy = np.asarray([1, 0, 3, 3,  0, 0, 4, 3,  0, 0, 1, 1,  1, 1,  0, 0, np.inf, 1,  2, 2, 3, 3,  0, 0, 2, 2], np.float64)
    pt_off = np.asarray([0, 2, 4, 6, 7, 9, 11, 13], np.int32)
    row_off = np.asarray([0, 5, 6, 7], np.int32)
    sel = np.asarray([0, 7, -1, 0, 0, 0, 0], np.int32)
    st, act, area, bbox, run_off, runs, text_off, text = R.rle_arrays(xy, pt_off, row_off, sel, [4, 0, 4], [3, 3, 2.5])
    assert st.tolist() == [0, 1, 2] and act.tolist() == [0, 0, 255, 3, 2, 5, 5]
    assert area.tolist() == [6, 12, 0, 0, 0, 0, 0] and bbox.tolist()[:2] == [[1, 0, 2, 3], [0, 0, 4, 3]] and not bbox[2:].any()
    assert run_off.tolist() == [0, 3, 5, 5, 5, 5, 5, 5] and runs.tolist() == [3, 6, 3, 0, 12] and runs.dtype == np.uint32
    assert text == R.enc([3, 6, 3]) + R.enc([0, 12]) and text_off.tolist() == [0, 3, 5, 5, 5, 5, 5, 5]
    assert R.rle_arrays(xy, pt_off, row_off, sel, [4, 0, 4], [3, 3, 2], max_pixels_per_row=8)[0].tolist() == [3, 1, 0]


# ----------------------------------------------------------------------------------------------- the host layer
def rows():
    cells = [cell(ob("cat", [(1, 0), (3, 3)]), ob("dog", [(0, 0), (4, 3)]), ob("dog", [(0.6, 0.6), (0.9, 0.9)]), ob("cat", [(1, 1)]),
                  ob("cat", [(0, 0), (1e300, 1)]), ob(7, [(0, 0), (2, 2)])),
             cell(ob("dog", [(0, 0), (3, 3)])), cell(), cell(ob("cat", [(0, 0), (2, 2)])),
             cell(ob("cat", [(0, 0), (9, 9), (0, 9), (9, 0)]), ob("dog", [(2, 2), (4, 4)]), ob("bird", [(-5, -5), (20, 20)]))]
    return cells, [4, 0, 5, 3.5, 10], [3, 4, 2, 3, 10]


def test_polygon_rle_results():
    cells, W, H = rows()
    be = RleBackend()
    stats = {}
    res = P.polygon_rle(cells, W, H, backend=be, stats=stats, sources=[f"s{k}" for k in range(5)])
    poly = res.polygons
    assert res.rows["status"].tolist() == ["rasterised", "no_size", "rasterised", "fractional_size", "rasterised"]
    assert poly["row"].tolist() == [0] * 5 + [1, 3, 4, 4, 4] and poly["source"].tolist()[-1] == "s4"
    assert poly["action"].tolist() == ["encoded", "encoded", "encoded", "too_few_points", "bad_coords", "no_raster", "no_raster",
                                       "encoded", "encoded", "encoded"]
    assert poly["area"].tolist()[:3] == [6, 12, 0] and poly[["x", "y", "w", "h"]].to_numpy().tolist()[:2] == [[1, 0, 2, 3], [0, 0, 4, 3]]
    assert poly["runs"].tolist()[:5] == [3, 2, 1, 0, 0] and res.classes == ["cat", "dog", "bird"]
    assert res.counts[:5] == [R.enc([3, 6, 3]), R.enc([0, 12]), R.enc([12]), None, None] and res.counts[5] is None
    assert res.sizes == [[3, 4]] * 5 + [None, None] + [[10, 10]] * 3 and len(res.counts) == len(res.sizes) == len(poly)
    xy = np.asarray([(0, 0), (9, 9), (0, 9), (9, 0)], np.float64)                # the bow tie: even-odd, as the rule says
    assert np.array_equal(U.rle_to_mask(res.counts[7], res.sizes[7]), K21.cover(xy, 10, 10))
    assert U.rle_to_mask(res.counts[9], res.sizes[9]).all() and poly["area"].tolist()[9] == 100   # overlap hides nothing
    assert res.rows[["polygons", "encoded", "empty"]].to_numpy().tolist() == [[5, 2, 1], [1, 0, 0], [0, 0, 0], [1, 0, 0], [3, 3, 0]]
    assert res.per_class["class"].tolist() == ["cat", "dog", "bird"] and res.per_class["encoded"].tolist() == [2, 2, 1]
    assert res.per_class["empty"].tolist() == [0, 1, 0] and res.per_class["pixels"].tolist()[2] == 100
    t = res.totals
    assert stats == t and (t["selected"], t["encoded"], t["empty"], t["no_raster"], t["bad_coords"], t["too_few_points"]) == (10, 5, 1, 2, 1, 1)
    assert t["unmatchable_name_polygons"] == 1 and t["polygons"] == 11 and t["rows_no_size"] == 1 and t["runs"] == int(poly["runs"].sum())
    assert t["bytes"] == sum(len(c) for c in res.counts if c) and t["pixels"] == int(poly["area"].sum())
    res = P.polygon_rle(cells, W, H, classes=["dog"], labels=["dog"] * 5, backend=be)
    assert res.polygons["name"].tolist() == ["dog"] * 4 and res.totals["unknown_class"] == 0
    res = P.polygon_rle(cells, W, H, max_pixels_per_row=12, backend=be)
    assert res.rows["status"].tolist() == ["rasterised", "no_size", "rasterised", "fractional_size", "too_large"]
    res = P.polygon_rle(pd.Series([], dtype=object), [], [], backend=be)
    assert len(res.polygons) == 0 and res.counts == [] and res.totals["runs"] == 0 and len(res.per_class) == 0


def test_chunks_change_nothing(monkeypatch):
    cells, W, H = rows()
    whole = P.polygon_rle(cells, W, H, backend=RleBackend())
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 2)
    be = RleBackend()
    parts = P.polygon_rle(cells, W, H, backend=be)
    assert be.calls == 3 and parts.counts == whole.counts and parts.sizes == whole.sizes and parts.totals == whole.totals
    assert parts.polygons.equals(whole.polygons) and parts.rows.equals(whole.rows) and parts.per_class.equals(whole.per_class)


@pytest.mark.parametrize("bad", [dict(max_pixels_per_row=0), dict(max_pixels_per_row=2 ** 30 + 1), dict(max_pixels_per_row=1.0),
                                 dict(max_pixels_per_row=True), dict(classes=["a", "a"]), dict(classes=[1]), dict(labels=["a", "b"])])
def test_argument_validation(bad):
    with pytest.raises(ValueError):
        P.polygon_rle([cell(ob("a", [(0, 0), (2, 2)]))], [4], [4], backend=RleBackend(), **bad)
    with pytest.raises(ValueError):
        P.polygon_rle([cell()], [4, 4], [4], backend=RleBackend())


def test_a_backend_without_the_entry_and_a_device_that_disagrees(tmp_path):
    with pytest.raises(TypeError, match="polygon_rle"):
        P.polygon_rle([], [], [], backend=OracleBackend())
    df = pd.DataFrame({COL: [cell(ob("a", [(0, 0), (2, 2)]))], "width": [4], "height": [4]})
    with pytest.raises(TypeError, match="polygon_rle"):
        P.export_coco_frame(df, tmp_path / "x.json", segmentation="rle", backend=CocoBackend())
    with pytest.raises(TypeError, match="polygon_rle"):
        P.export_coco_from_excels([], tmp_path, segmentation="rle", backend=CocoBackend())

    class Off(RleBackend):
        def polygon_rle(self, *a, **k):
            out = list(super().polygon_rle(*a, **k))
            out[0] = out[0] ^ 1
            return out

    with pytest.raises(RuntimeError, match="differs"):
        P.polygon_rle([cell(ob("a", [(0, 0), (2, 2)]))], [4], [4], backend=Off())
    with pytest.raises(RuntimeError, match="differs"):
        P.export_coco_frame(df, tmp_path / "x.json", segmentation="rle", backend=Off())


# ----------------------------------------------------------------------------------------------- the COCO file
def frame():
    cells, W, H = rows()
    return pd.DataFrame({"source": ["http://x/a.jpg", "b.png", "c.png", "d.png", "dir/e.png"], COL: cells, "width": W, "height": H,
                         "label": ["cat", "dog", "cat", "cat", "dog"]})


def check_rle_file(path, df, iscrowd=0, labels=None):
    """the file against the rule: every printed polygon's decoded mask is its cover; ids and images follow K16's rules"""
    raw = open(path, "rb").read()
    doc = json.loads(raw.decode("utf-8"))
    cells, W, H = df[COL].tolist(), df["width"].tolist(), df["height"].tolist()
    want, n_polys, images = [], 0, set()
    cat_of = {c["name"]: c["id"] for c in doc["categories"]}
    for i, c in enumerate(cells):
        objs = json.loads(c)["objects"]
        st, w, h = K21.row_size(float(W[i]), float(H[i]), 1 << 26)
        if st == 0:
            images.add(i + 1)
        for k, o in enumerate(objs):
            pts = np.asarray([(p["x"], p["y"]) for p in o["polygon"]["ptList"]], np.float64).reshape(-1, 2)
            ok = isinstance(o["name"], str) and (labels is None or o["name"] == labels[i])
            if ok and st == 0 and len(pts) >= 2 and (np.abs(pts) < K21.LIMIT).all() and K21.cover(pts, w, h).any():
                want.append((n_polys + k + 1, i + 1, cat_of[o["name"]], K21.cover(pts, w, h)))
        n_polys += len(objs)
    assert len(doc["annotations"]) == len(want)
    for a, (aid, iid, cat, full) in zip(doc["annotations"], want):
        assert (a["id"], a["image_id"], a["category_id"], a["iscrowd"]) == (aid, iid, cat, iscrowd)
        seg = a["segmentation"]
        assert seg["size"] == list(full.shape) and np.array_equal(U.rle_to_mask(seg["counts"], seg["size"]), full)
        ys, xs = np.nonzero(full)
        assert a["area"] == full.sum() and a["bbox"] == [xs.min(), ys.min(), np.ptp(xs) + 1, np.ptp(ys) + 1]
        assert b'"area":%d.00,' % full.sum() in raw
    assert {im["id"] for im in doc["images"]} == images
    return doc


def test_export_coco_frame_in_rle_mode(tmp_path):
    df = frame()
    stats = {}
    res = P.export_coco_frame(df, tmp_path / "r.json", segmentation="rle", skipped_csv=tmp_path / "s.csv", backend=RleBackend(),
                              stats=stats)
    doc = check_rle_file(res["output"], df)
    assert stats == res and res["annotations"] == len(doc["annotations"]) == 5 and res["clipped"] == 0 and res["written"] == 5
    assert (res["empty"], res["no_size"], res["bad_coords"], res["too_few_points"], res["too_large"]) == (1, 2, 1, 1, 0)
    assert res["rows_no_size"] == 2 and res["images"] == 3 and res["unmatchable_name_polygons"] == 1
    assert res["rle_device_seconds"] >= 0 and res["rle_format_seconds"] >= 0
    assert [c["name"] for c in doc["categories"]] == ["cat", "dog", "bird"]
    skipped = pd.read_csv(tmp_path / "s.csv", encoding="utf-8-sig")
    assert skipped["action"].tolist() == ["empty", "too_few_points", "bad_coords", "no_size", "no_size"]
    assert skipped["row"].tolist() == [0, 0, 0, 1, 3] and skipped["object"].tolist() == [2, 3, 4, 0, 0]
    res = P.export_coco_frame(df, tmp_path / "c.json", segmentation="rle", iscrowd=1, label_col="label", keep_empty_images=False,
                              backend=RleBackend())
    doc = json.load(open(res["output"], encoding="utf-8"))
    assert [a["id"] for a in doc["annotations"]] == [1, 10] and all(a["iscrowd"] == 1 for a in doc["annotations"])
    assert [im["id"] for im in doc["images"]] == [1, 5]
    for bad in (dict(segmentation="RLE"), dict(segmentation="rle", iscrowd=2), dict(segmentation="rle", iscrowd=True),
                dict(segmentation="rle", max_pixels_per_row=0)):
        with pytest.raises(ValueError):
            P.export_coco_frame(df, tmp_path / "x.json", backend=RleBackend(), **bad)
    assert not (tmp_path / "x.json").exists()


def test_the_counts_string_is_json_escaped(tmp_path):
    """a run whose code holds the backslash (byte 92 = 44 + 48: the value 12 + 32 k with a continuation) must survive the file"""
    w, h = 3, 140                                                                # runs 140 = 12 + 4 * 32: "\\4"
    df = pd.DataFrame({COL: [cell(ob("a", [(1, 0), (2, h)]))], "width": [w], "height": [h]})
    res = P.export_coco_frame(df, tmp_path / "b.json", segmentation="rle", backend=RleBackend())
    raw = open(res["output"], "rb").read()
    seg = json.loads(raw)["annotations"][0]["segmentation"]
    assert "\\" in seg["counts"] and b"\\\\" in raw and R.dec(seg["counts"]) == [140, 140, 140]


def test_polygon_lists_are_what_they_were(tmp_path):
    """segmentation=True / False write what they wrote before the run-length mode existed: tests/golden/coco_rle_frame_*.json
    are the files of the commit before it for frame(), byte for byte"""
    df = frame()
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for seg, name in ((True, "coco_rle_frame_polygons.json"), (False, "coco_rle_frame_detect.json")):
        res = P.export_coco_frame(df, tmp_path / f"a{seg}.json", segmentation=seg, backend=RleBackend())
        assert open(res["output"], "rb").read() == open(os.path.join(golden, name), "rb").read()
        assert "rle_format_seconds" not in res
        res = P.export_coco_frame(df, tmp_path / f"b{seg}.json", COL, "width", "height", "source", None, None, seg, True, None, None,
                                  RleBackend(), None)                            # the positional arguments keep their places
        assert open(res["output"], "rb").read() == open(os.path.join(golden, name), "rb").read()


def test_export_coco_csv_in_rle_mode(tmp_path):
    df = frame()
    path = tmp_path / "in.csv"
    df.to_csv(path, index=False, encoding="utf-8-sig")
    want = open(P.export_coco_frame(df, tmp_path / "f.json", segmentation="rle", backend=RleBackend())["output"], "rb").read()
    res = P.export_coco_csv(path, tmp_path / "c.json", segmentation="rle", backend=RleBackend())
    assert res is not None and open(res["output"], "rb").read() == want
    check_rle_file(res["output"], df)
