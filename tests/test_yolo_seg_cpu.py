"""YOLO segmentation labels (K13) without a GPU: the host side of yolo_seg_label_texts and of
generate_yolo_datasets_from_excels(task="segment"), with the device stage stood in for by the restatement in
tests/yolo_seg_ref.py."""
import json
import math
import random

import numpy as np
import pandas as pd
import pytest

import yolo_seg_ref as R
from box_repair_ref import decide
from helpers import OracleBackend
from test_yolo_host_cpu import _Sheets

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd import native_json as nj
from deal_yolo_daya_amd.core import processor as P
from deal_yolo_daya_amd.core import utils as U


class SegBackend(OracleBackend):
    def yolo_seg_lines(self, xy, pt_off, row_off, sel, width, height, class_id):
        return R.seg_arrays(xy, pt_off, row_off, sel, width, height, class_id)


BE = SegBackend()


def ob(name, pts):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def seg(cells, labels, cids, ws, hs, **kw):
    stats = {}
    texts, reasons = P.yolo_seg_label_texts(cells, labels, cids, ws, hs, BE, stats, **kw)
    return texts, reasons, stats


def check_rows(cells, labels, cids, ws, hs):
    texts, reasons, stats = seg(cells, labels, cids, ws, hs)
    counts = {a: 0 for a in R.ACTIONS}
    for k, (c, lab, cid, w, h) in enumerate(zip(cells, labels, cids, ws, hs)):
        t, why, acts = R.seg_row(c, lab, cid, w, h)
        assert (texts[k], reasons[k]) == (t, why), (k, c, w, h)
        for a in acts:
            counts[a] += 1
    assert {a: stats[a] for a in R.ACTIONS} == counts
    assert stats["polygons"] == sum(counts.values())
    return texts, reasons, stats


# ------------------------------------------------------------------ the worked answers
WORKED = [
    (cell(ob("a", [(-100, 50), (10, 0), (10, 100)])), 3, 200, 200,
     "3 0.000000 0.022727 0.050000 0.000000 0.050000 0.500000 0.000000 0.477273", "clipped"),
    (cell(ob("a", [(10, 30), (30, 10)])), 0, 1280, 720,
     "0 0.007812 0.013889 0.023438 0.013889 0.023438 0.041667 0.007812 0.041667", "written"),
    (cell(ob("a", [(0, 0), (0, 10), (-5, 5)])), 0, 100, 100, None, "empty"),
    (cell(ob("a", [(1280, 0), (1279.9994, 720), (0, 360)])), 7, 1280, 720,
     "7 1.000000 0.000000 1.000000 1.000000 0.000000 0.500000", "written"),
]


@pytest.mark.parametrize("c,cid,w,h,text,act", WORKED)
def test_worked_answers(c, cid, w, h, text, act):
    assert R.seg_row(c, "a", cid, w, h)[0] == text
    texts, reasons, stats = seg([c], ["a"], [cid], [w], [h])
    assert texts == [text] and stats[act] == 1
    assert reasons == [None if text else P.REASON_NO_VALID_BOX]


# ------------------------------------------------------------------ each action and each rule edge
EDGES = [
    [(0, 0), (100, 0), (100, 100)],                  # on the borders: written
    [(-0.0, 0), (50, -0.0), (50, 50)],
    [(float("nan"), 0), (1, 1), (2, 0)],
    [(float("inf"), 0), (1, 1), (2, 0)],
    [(2.0 ** 43, 0), (1, 1), (2, 0)],
    [(2.0 ** 43 - 1, 0), (1, 1), (2, 0)],
    [("1", 0), (1, 1), (2, 0)],
    [(None, 0), (1, 1), (2, 0)],
    [(True, 0), (5, 5), (0, 9)],
    [(10 ** 400, 0), (1, 1), (2, 0)],
    [],
    [(5, 5)],
    [(5, 5), (20, 30)],
    [(-5, -5), (20, 30)],
    [(-50, -50), (-10, -20), (-30, -5)],             # entirely outside
    [(200, 10), (300, 20), (250, 90)],
    [(10, 10), (20, 20), (30, 30)],                  # collinear: its clip has no area
    [(10, 10), (10, 10)],
    [(0.5, 0.5), (0.5, 10), (10, 10)],
]


def edge_cells():
    out = []
    for pts in EDGES:
        objs = [{"name": "a", "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}]
        out.append(json.dumps({"objects": objs}, allow_nan=True))
    return out


def test_each_action_and_rule_edge():
    cells = edge_cells()
    # coordinates json cannot spell natively (strings, null, huge ints, true, Infinity) go to the Python path
    for w, h in ((100, 100), (100.0, 50), (1, 1)):
        _, _, stats = check_rows(cells, ["a"] * len(cells), [1] * len(cells), [w] * len(cells), [h] * len(cells))
        if w == 100:
            assert all(stats[a] for a in R.ACTIONS if a != "no_size"), stats
    objs = [ob("a", [(0, 0), (1, 1)])]
    bad = [c for c in cells if "ptList\": []" not in c][:3]
    assert R.seg_row(bad[2], "a", 0, 100, 100)[2] == ["bad_coords"]
    assert R.seg_row(cell(*objs), "a", 0, 100, 100)[0] == "0 0.000000 0.000000 0.010000 0.000000 0.010000 0.010000 0.000000 0.010000"


@pytest.mark.parametrize("w,h", [(float("nan"), 10), (-5, 10), ("100", 10), (0, 10), (10, 0), (None, 10), (2.0 ** 43, 10),
                                 (float("inf"), 10), (np.float32(64), np.int64(48)), (True, 1)])
def test_sizes(w, h):
    cells = [cell(ob("a", [(1, 1), (5, 2), (3, 4)]))]
    texts, reasons, stats = check_rows(cells, ["a"], [2], [w], [h])
    if not w or not h:
        assert reasons == [P.REASON_NO_IMAGE_SIZE]
    elif R.size_of(w) is None:
        assert reasons == [P.REASON_NO_VALID_BOX] and stats["no_size"] == 1


def test_ties_round_half_to_even():
    # 10/1280 = 0.0078125 and 30/1280 = 0.0234375 are exact ties; the others round as CPython's "%.6f"
    for v, W, want in ((10, 1280, "0.007812"), (30, 1280, "0.023438"), (1, 8, "0.125000"), (5, 2 ** 21, "0.000002"),
                       (1, 3, "0.333333"), (2, 3, "0.666667")):
        c = cell(ob("a", [(v, v), (W, W)]))
        t = seg([c], ["a"], [0], [W], [W])[0][0]
        assert t.split()[1] == want, (v, W, t)
        assert f"{v / W:.6f}" == want


def test_no_match_and_label_order():
    cells = [cell(ob("b", [(1, 1), (5, 5), (1, 5)])), None, "not json", cell(ob("a", [(1, 1), (5, 5), (1, 5)]), ob("b", [(0, 0), (9, 9)]))]
    texts, reasons, _ = check_rows(cells, ["a", "a", "a", "a"], [0, 0, 0, 4], [0, 10, 10, 10], [10, 10, 10, 10])
    assert reasons[:3] == [P.REASON_NO_MATCHING_BOX] * 3 and texts[3].startswith("4 ")


def test_negative_and_odd_class_ids_go_to_the_host():
    cells = [cell(ob("a", [(1, 1), (5, 5), (1, 5)]))] * 3
    texts, reasons, stats = check_rows(cells, ["a"] * 3, [-1, 2 ** 40, 3], [10] * 3, [10] * 3)
    assert texts[0].startswith("-1 ") and texts[1].startswith(f"{2 ** 40} ") and stats["python_rows"] == 2


# ------------------------------------------------------------------ the native polygon scan
def fuzz_cells(n, seed, numeric=False):
    rnd = random.Random(seed)
    names = ["a", "b", "", None, 5, "猫", "a\ud800"]
    out = []
    for _ in range(n):
        objs = []
        for _ in range(rnd.randint(0, 4)):
            kind = rnd.random()
            if kind < 0.05:
                objs.append(rnd.choice([3, "x", None, []]))
                continue
            pts = []
            for _ in range(rnd.randint(0, 6)):
                p = {}
                if rnd.random() < 0.9:
                    odd = [rnd.uniform(-50, 150), rnd.randint(-10, 110)] + ([] if numeric else [1e300 * 10, "s", None, 2 ** 60])
                    p["x"] = rnd.choice(odd) if rnd.random() < 0.1 else rnd.uniform(-50, 150)
                if rnd.random() < 0.9:
                    p["y"] = rnd.uniform(-50, 150)
                pts.append(p if rnd.random() > 0.03 else 7)
            o = {"name": rnd.choice(names), "polygon": {"ptList": pts}}
            if rnd.random() < 0.03:
                o["polygon"] = []
            objs.append(o)
        doc = {"objects": objs}
        out.append(json.dumps(doc, ensure_ascii=rnd.random() < 0.5) if rnd.random() > 0.03 else rnd.choice([None, "{", "[]", ""]))
    return out


def _plain(c):
    try:
        c.encode("utf-8")
        return True
    except (UnicodeEncodeError, AttributeError):
        return c is None


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_native_polygon_scan_matches_json(threads):
    cells = [c for c in fuzz_cells(600, threads) if _plain(c)]
    labels = ["a"] * len(cells)
    scan = nj.scan_labelled_polygons(cells, labels, n_threads=threads)
    try:
        irregular = 0
        for i, c in enumerate(cells):
            if scan.status[i] == nj.IRREGULAR:
                irregular += 1
                continue
            b0, b1 = int(scan.cell_box_off[i]), int(scan.cell_box_off[i + 1])
            got = [(bool(scan.sel[b]), scan.xy[2 * scan.pt_off[b]:2 * scan.pt_off[b + 1]].reshape(-1, 2).tolist()) for b in range(b0, b1)]
            want = [(name == "a", [[float(x), float(y)] for x, y in pts]) for _, name, pts in fl.seg_cell_polygons(c)]
            assert got == want, (i, c)
        assert 0 < irregular < len(cells)
    finally:
        scan.close()


def test_matched_objects_equal_the_detect_step():
    cells = fuzz_cells(800, 11)
    for c in cells:
        boxes = U._extract_boxes_with_labels(c)
        polys = fl.seg_cell_polygons(c)
        assert [b[0] for b in boxes] == [p[1] for p in polys]
        assert [b[1:] for b in boxes] == [b[2:] for b in fl.audit_cell_boxes(c)]
    cells = fuzz_cells(800, 12, numeric=True)          # the detect step's arithmetic raises on str coordinates, as the reference's
    labels = ["a"] * len(cells)
    det = P.yolo_label_texts(cells, labels, [0] * len(cells), [100] * len(cells), [100] * len(cells), BE)[1]
    segr = seg(cells, labels, [0] * len(cells), [100] * len(cells), [100] * len(cells))[1]
    assert [r == P.REASON_NO_MATCHING_BOX for r in det] == [r == P.REASON_NO_MATCHING_BOX for r in segr]
    check_rows(cells, labels, [0] * len(cells), [100] * len(cells), [100] * len(cells))


def test_two_point_polygons_follow_the_box_repair():
    rnd = random.Random(5)
    for _ in range(3000):
        W, H = rnd.choice([(100.0, 80.0), (1280.0, 720.0), (7.0, 3.0)])
        pick = lambda lim: rnd.choice([rnd.uniform(-lim, 2 * lim), float(rnd.randint(-2, int(lim) + 2)), 0.0, lim, -0.0])  # noqa: E731
        a, b = (pick(W), pick(H)), (pick(W), pick(H))
        act, line = R.polygon([a, b], W, H, 0)
        box = (min(a[0], b[0]), min(a[1], b[1]), max(a[0], b[0]), max(a[1], b[1]))
        ract, corners = decide(box, "ok", W, H)
        assert (act in ("written", "clipped")) == (ract in ("keep", "clip")), (a, b, W, H, act, ract)
        if act == "clipped":
            assert ract == "clip"
            x1, y1, x2, y2 = corners
            got = R.clip([(box[0], box[1]), (box[2], box[1]), (box[2], box[3]), (box[0], box[3])], W, H)
            assert len(got) == 4 and set(got) == {(x1, y1), (x2, y1), (x2, y2), (x1, y2)}, (got, corners)
        elif act == "written":
            assert ract == "keep"


# ------------------------------------------------------------------ the dataset step
def _frames(tmp_path, polygons_first):
    img = tmp_path / "img"
    img.mkdir(exist_ok=True)
    rows = []
    rnd = random.Random(3)
    for k in range(40):
        (img / f"r{k}.jpg").write_bytes(b"x")
        pts = [(rnd.uniform(-40, 680), rnd.uniform(-40, 520)) for _ in range(rnd.randint(3, 8))]
        poly = cell(ob("猫" if k % 3 else "狗", pts))
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        box = cell(ob("猫" if k % 3 else "狗", [(min(xs), min(ys)), (max(xs), max(ys))]))
        rows.append({"source": str(img / f"r{k}.jpg"), "分类标签": "猫" if k % 3 else "狗",
                     P.BBOX_COL: poly if polygons_first else box, P.ANNOTATION_COL: poly if polygons_first else box,
                     "width": 640, "height": 480})
    return {"train": pd.DataFrame(rows[:30]), "val": pd.DataFrame(rows[30:])}


def _run(frames, tmp_path, **kw):
    book = tmp_path / "cat.xlsx"
    book.write_bytes(b"")
    with _Sheets(frames):
        return P.generate_yolo_datasets_from_excels([str(book)], str(tmp_path / "out"), download_images=False, backend=BE, **kw)


@pytest.mark.parametrize("polygons_first", [True, False])
def test_generate_segment(tmp_path, capsys, polygons_first):
    res = _run(_frames(tmp_path, polygons_first), tmp_path, task="segment")
    out = capsys.readouterr().out
    assert ("json_columns=[ANNOTATION_COL, BBOX_COL]" in out) == (not polygons_first)
    ds = res["datasets"][0]
    n_files = 0
    for f in (ds / "labels").rglob("*.txt"):
        n_files += 1
        for line in f.read_text().splitlines():
            vals = [float(v) for v in line.split()[1:]]
            assert len(vals) % 2 == 0 and len(vals) >= 6 and all(0.0 <= v <= 1.0 for v in vals)
    assert n_files == 40
    counts = P.summarize_yolo_label_counts([str(ds)])
    assert counts is not None
    with pytest.raises(ValueError):
        _run(_frames(tmp_path, polygons_first), tmp_path, task="obb")


def test_generate_segment_needs_the_method(tmp_path):
    with pytest.raises(TypeError):
        with _Sheets(_frames(tmp_path, True)):
            book = tmp_path / "c.xlsx"
            book.write_bytes(b"")
            P.generate_yolo_datasets_from_excels([str(book)], str(tmp_path / "o"), download_images=False, backend=OracleBackend(),
                                                 task="segment")


def test_polygon_first_split_workflow():
    rnd = random.Random(9)
    rows = []
    for k in range(60):
        objs = []
        for j in range(rnd.randint(1, 4)):
            pts = [(rnd.uniform(-100, 1400), rnd.uniform(-100, 800)) for _ in range(rnd.randint(3, 9))]
            objs.append(ob(rnd.choice(["猫", "狗", "鸟"]), pts))
        poly = json.dumps({"width": 1280, "height": 720, "objects": objs}, ensure_ascii=False)    # the replace step reads the size here
        rows.append({"source": f"s{k}.jpg", P.ANNOTATION_COL: poly})
    df = pd.DataFrame(rows)
    kept, _ = P.replace_ptlist_frame(df, backend=BE)
    rules = {"猫": "动物", "狗": "动物", "鸟": "动物"}
    poly_first = P.split_frames(kept, rules, json_columns=[P.ANNOTATION_COL, P.BBOX_COL], backend=BE)
    default = P.split_frames(kept, rules, backend=BE)
    longest = 0
    for a, b in zip(poly_first["categories"]["动物"], default["categories"]["动物"]):
        if not len(a):
            continue
        labels = a["分类标签"].tolist()
        n = len(a)
        cids = [0] * n
        t_seg = seg(a[P.ANNOTATION_COL].tolist(), labels, cids, a["width"].tolist(), a["height"].tolist())[0]
        assert all(t is None or all(len(line.split()) >= 7 for line in t.split("\n")) for t in t_seg)
        longest = max([longest] + [len(line.split()) for t in t_seg if t for line in t.split("\n")])
        det_a = P.yolo_label_texts([x or y for x, y in zip(a[P.BBOX_COL], a[P.ANNOTATION_COL])], labels, cids,
                                   a["width"].tolist(), a["height"].tolist(), BE)
        det_b = P.yolo_label_texts([x or y for x, y in zip(b[P.BBOX_COL], b[P.ANNOTATION_COL])], b["分类标签"].tolist(), cids,
                                   b["width"].tolist(), b["height"].tolist(), BE)
        assert det_a == det_b
    assert longest > 9                                  # polygons, not boxes
