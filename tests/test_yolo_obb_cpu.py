"""YOLO oriented-box labels (K17) without a GPU: the host side of yolo_obb_label_texts and of
generate_yolo_obb_datasets_from_excels, with the device stage stood in for by the restatement in tests/yolo_obb_ref.py, and
the restatement itself against exact arithmetic.

tests/golden/yolo_dataset_labels.json holds what generate_yolo_datasets_from_excels wrote for task="detect" and
task="segment" on `_frames` before the OBB step shared its body: `PYTHONPATH=. python tests/test_yolo_obb_cpu.py <file>` on that commit."""
import json
import random
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import yolo_obb_ref as R
import yolo_seg_ref as S
from helpers import OracleBackend
from test_yolo_host_cpu import _Sheets
from test_yolo_seg_cpu import EDGES, SegBackend, _frames, cell, ob

from deal_yolo_daya_amd.core import processor as P

GOLDEN = Path(__file__).parent / "golden" / "yolo_dataset_labels.json"


class ObbBackend(SegBackend):
    def yolo_obb_lines(self, xy, pt_off, row_off, sel, width, height, class_id, corners=False):
        res = R.obb_arrays(xy, pt_off, row_off, sel, width, height, class_id)
        return res if corners else res[:5]


BE = ObbBackend()


def obb(cells, labels, cids, ws, hs):
    stats = {}
    texts, reasons = P.yolo_obb_label_texts(cells, labels, cids, ws, hs, BE, stats)
    return texts, reasons, stats


def check_rows(cells, labels, cids, ws, hs):
    texts, reasons, stats = obb(cells, labels, cids, ws, hs)
    counts, clamped = {a: 0 for a in R.ACTIONS}, 0
    for k, (c, lab, cid, w, h) in enumerate(zip(cells, labels, cids, ws, hs)):
        t, why, acts = R.obb_row(c, lab, cid, w, h)
        assert (texts[k], reasons[k]) == (t, why), (k, c, w, h)
        for a in acts:
            counts[a] += 1
        if acts:
            clamped += sum(R.polygon(p, S.size_of(w), S.size_of(h), cid)[2] for p in S.matched_polygons(c, lab))
    assert {a: stats[a] for a in R.ACTIONS} == counts and stats["clamped"] == clamped
    assert stats["polygons"] == sum(counts.values())
    return texts, reasons, stats


# ------------------------------------------------------------------ the worked answers
SQUARE = "3 0.400000 0.100000 0.800000 0.400000 0.500000 0.800000 0.100000 0.500000"
WORKED = [
    ([(40, 10), (80, 40), (50, 80), (10, 50)], 100, 100, 3, SQUARE, 0),
    ([(40, 10), (45, 45), (80, 40), (50, 80), (44, 46), (10, 50)], 100, 100, 3, SQUARE, 0),     # the same outline, with pockets
    ([(10, 10), (60, 10), (60, 40), (10, 40), (30, 20)], 200, 100, 0,
     "0 0.050000 0.100000 0.300000 0.100000 0.300000 0.400000 0.050000 0.400000", 0),
    ([(0, 0), (4, 0), (2, 3)], 8, 8, 2, "2 0.000000 0.000000 0.500000 0.000000 0.500000 0.375000 0.000000 0.375000", 0),
    ([(0, 30), (40, 0), (100, 80), (60, 100)], 100, 100, 5,
     "5 0.400000 0.000000 1.000000 0.800000 0.600000 1.000000 0.000000 0.300000", 1),           # corner (60, 110)
    ([(10, 10), (20, 20), (30, 30)], 100, 100, 7, None, 0),                                      # flat; K13 writes it
]


@pytest.mark.parametrize("pts,w,h,cid,text,clamped", WORKED)
def test_worked_answers(pts, w, h, cid, text, clamped):
    c = cell(ob("a", pts))
    assert R.obb_row(c, "a", cid, w, h)[0] == text
    texts, reasons, stats = obb([c], ["a"], [cid], [w], [h])
    assert texts == [text] and stats["clamped"] == clamped
    assert reasons == [None if text else P.REASON_NO_VALID_BOX]
    assert stats["flat"] == (text is None) and stats["written"] == (text is not None)
    if text is None:
        assert S.seg_row(c, "a", cid, w, h)[2] == ["written"]
    if clamped:
        assert R.polygon(pts, float(w), float(h), cid)[3][2] == (60.0, 110.0)


# ------------------------------------------------------------------ exact on integer coordinates
def exact_minimum(C):
    """the exact minimum rectangle area over every direction c_i -> c_j that has no point of C on its right, or None"""
    best = None
    for i, (cx, cy) in enumerate(C):
        for j, (bx, by) in enumerate(C):
            dx, dy = bx - cx, by - cy
            if (dx, dy) == (0, 0) or any(dx * (y - cy) - dy * (x - cx) < 0 for x, y in C):
                continue
            us = [(x - cx) * dx + (y - cy) * dy for x, y in C]
            vs = [(y - cy) * dx - (x - cx) * dy for x, y in C]
            area = Fraction((max(us) - min(us)) * (max(vs) - min(vs)), dx * dx + dy * dy)
            best = area if best is None or area < best else best
    return best


def encloses(corners, C, size):
    """every vertex on the inner side of the four edges.  A corner is off by at most 8 eps * size (its formula's roundings, on
    values up to size), which moves an edge's cross product, over lengths up to 2 * size, by less than 32 eps * size^2."""
    tol = 32 * sys.float_info.epsilon * size * size
    for x, y in C:
        for k in range(4):
            (ax, ay), (bx, by) = corners[k], corners[(k + 1) % 4]
            if (bx - ax) * (y - ay) - (by - ay) * (x - ax) < -tol:
                return False
    return True


def integer_polygons():
    rnd = random.Random(17)
    for k in range(1500):
        hi = 1024 if k % 2 else 5
        pts = [(rnd.randint(0, hi), rnd.randint(0, hi)) for _ in range(rnd.randint(3, 12))]
        if k % 5 == 0:                                    # a repeated vertex and a collinear run
            pts.insert(rnd.randrange(len(pts)), pts[0])
            (ax, ay), (bx, by) = pts[0], pts[1]
            pts.insert(rnd.randrange(len(pts)), ((ax + bx) // 2 * 2 - ax, (ay + by) // 2 * 2 - ay) if k % 10 else (bx, by))
            pts = [(min(max(x, 0), hi), min(max(y, 0), hi)) for x, y in pts]
        yield pts, float(hi)


def test_exact_on_integer_coordinates():
    n = 0
    for pts, size in integer_polygons():
        C = [(float(x), float(y)) for x, y in pts]
        area, corners = R.rectangle(C)
        want = exact_minimum(pts)
        assert area == (None if want is None else float(want)), (pts, area, want)     # correctly rounded, every case
        act, line, clamped, _ = R.polygon(pts, size, size, 0)
        if not want:
            assert act in ("flat", "empty") and line is None
        else:
            assert act == "written" and len(line.split()) == 9
            assert encloses(corners, C, size)
        n += 1
    assert n == 1500


def test_every_direction_encloses_on_floats():
    rnd = random.Random(23)
    for k in range(900):
        kind = k % 3
        pick = (lambda: rnd.uniform(0, 1000)) if kind == 0 else (lambda: round(rnd.uniform(0, 1000), 2)) if kind == 1 else \
            (lambda: float(rnd.randint(0, 9)))
        C = [(pick(), pick()) for _ in range(rnd.randint(3, 12))]
        if k % 7 == 0:
            C.insert(rnd.randrange(len(C)), C[0])
        area, corners = R.rectangle(C)
        assert area is not None and encloses(corners, C, 1000.0), C


# ------------------------------------------------------------------ two points, actions, rule edges
def test_two_point_polygon_in_the_image_is_the_segment_line():
    rnd = random.Random(5)
    for _ in range(500):
        W, H = rnd.choice([(100.0, 80.0), (1280.0, 720.0), (7.0, 3.0)])
        pts = [(rnd.uniform(0, W), rnd.uniform(0, H)), (rnd.choice([0.0, W, rnd.uniform(0, W)]), rnd.uniform(0, H))]
        act, line = S.polygon(pts, W, H, 4)
        got = R.polygon(pts, W, H, 4)
        assert got[0] == act and got[1] == line and got[2] == 0, pts
    c = cell(ob("a", [(10, 30), (30, 10)]))
    assert obb([c], ["a"], [0], [1280], [720])[0] == P.yolo_seg_label_texts([c], ["a"], [0], [1280], [720], BE)[0]


OBB_EDGES = EDGES + [
    [(10, 10), (20, 20), (30, 30), (40, 40)],            # flat
    [(5, 5), (5, 5), (9, 9)],
    [(0, 30), (40, 0), (100, 80), (60, 100)],            # clamped
    [(-20, 50), (50, -20), (120, 50), (50, 120)],        # clipped to an octagon
    [(3, 3), (3, 3), (7, 3), (7, 9), (7, 9), (3, 9)],    # repeated vertices
]


def edge_cells():
    out = []
    for pts in OBB_EDGES:
        objs = [{"name": "a", "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}]
        out.append(json.dumps({"objects": objs}, allow_nan=True))
    return out


def test_each_action_and_rule_edge():
    cells = edge_cells()
    for w, h in ((100, 100), (100.0, 50), (1, 1)):
        _, _, stats = check_rows(cells, ["a"] * len(cells), [1] * len(cells), [w] * len(cells), [h] * len(cells))
        if w == 100 and h == 100:
            assert all(stats[a] for a in R.ACTIONS if a != "no_size"), stats
            assert stats["clamped"] >= 1 and stats["flat"] >= 3
    _, _, stats = check_rows(cells[:3], ["a"] * 3, [1] * 3, [float("nan")] * 3, [10] * 3)
    assert stats["no_size"] == 3
    assert P.OBB_ACTIONS == R.ACTIONS == P.SEG_ACTIONS + ("flat",)


def test_class_ids_the_device_does_not_print_go_to_the_host():
    cells = [cell(ob("a", [(1, 1), (5, 5), (1, 5)]), ob("a", [(2, 2), (12, 5), (8, 11)]))] * 3
    texts, _, stats = check_rows(cells, ["a"] * 3, [-1, 2 ** 40, 3], [10] * 3, [10] * 3)
    assert texts[0].startswith("-1 ") and texts[1].startswith(f"{2 ** 40} ") and stats["python_rows"] == 2
    assert all(len(t.split("\n")) == 2 for t in texts)


def random_polygons(rnd, n):
    out = []
    for _ in range(n):
        W, H = rnd.choice([(100.0, 80.0), (640.0, 480.0)])
        r = rnd.choice([10, 60, 400])
        cx, cy = rnd.uniform(0, W), rnd.uniform(0, H)
        pts = [(cx + rnd.uniform(-r, r), cy + rnd.uniform(-r, r)) for _ in range(rnd.randint(0, 9))]
        if rnd.random() < 0.2:
            pts = [(float(round(x)), float(round(y))) for x, y in pts]
        out.append((pts, W, H))
    return out


def test_obb_lines_python_against_the_restatement():
    rnd = random.Random(31)
    seen = set()
    for pts, W, H in random_polygons(rnd, 1500) + [(p, 100.0, 100.0) for p in OBB_EDGES if all(
            isinstance(v, (int, float)) and not isinstance(v, bool) and abs(v) < 1e300 for q in p for v in q)]:
        act, line, clamped, _ = R.polygon(pts, W, H, 9)
        lines, actions, n_clamped = P._obb_lines_python([pts], 9, W, H)
        assert (lines, actions, n_clamped) == ([line] if line else [], [R.ACTIONS.index(act)], clamped), pts
        seen.add((act, clamped))
    assert {a for a, _ in seen} >= {"written", "clipped", "too_few_points", "empty", "flat"} and ("written", 1) in seen
    assert P._obb_lines_python([[(1, 1), (5, 2), (3, 4)]], 0, float("nan"), 10) == ([], [5], 0)
    assert P._seg_lines_python([[(1, 1), (5, 2), (3, 4)]], 0, 10, 10) == (["0 0.100000 0.100000 0.500000 0.200000 0.300000 0.400000"], [0])


# ------------------------------------------------------------------ the dataset step
def _run(frames, tmp_path, fn, backend=BE, **kw):
    book = tmp_path / "cat.xlsx"
    book.write_bytes(b"")
    with _Sheets(frames):
        return fn([str(book)], str(tmp_path / "out"), download_images=False, backend=backend, **kw)


@pytest.mark.parametrize("polygons_first", [True, False])
def test_generate_obb(tmp_path, capsys, polygons_first):
    res = _run(_frames(tmp_path, polygons_first), tmp_path, P.generate_yolo_obb_datasets_from_excels)
    out = capsys.readouterr().out
    assert ("json_columns=[ANNOTATION_COL, BBOX_COL]" in out) == (not polygons_first)
    ds = res["datasets"][0]
    n_files = 0
    for f in (ds / "labels").rglob("*.txt"):
        n_files += 1
        for line in f.read_text().splitlines():
            vals = [float(v) for v in line.split()[1:]]
            assert len(line.split()) == 9 and all(0.0 <= v <= 1.0 for v in vals)
    assert n_files == 40
    assert (ds / "data.yaml").exists() and P.summarize_yolo_label_counts([str(ds)]) is not None
    # the same files as task="segment" writes, a rectangle where it has an outline
    (tmp_path / "seg").mkdir()
    seg = _run(_frames(tmp_path / "seg", polygons_first), tmp_path / "seg", P.generate_yolo_datasets_from_excels, task="segment")
    names = lambda d: sorted(str(p.relative_to(d)) for p in (d / "labels").rglob("*.txt"))   # noqa: E731
    assert names(ds) == names(seg["datasets"][0])
    assert res["stats"] == seg["stats"] and res["processed"] == seg["processed"]


def test_generate_obb_needs_the_method(tmp_path):
    for backend in (OracleBackend(), SegBackend()):
        with pytest.raises(TypeError):
            _run(_frames(tmp_path, True), tmp_path, P.generate_yolo_obb_datasets_from_excels, backend=backend)
    with pytest.raises(TypeError):
        P.yolo_obb_label_texts([], [], [], [], [], SegBackend())
    with pytest.raises(ValueError):
        _run(_frames(tmp_path, True), tmp_path, P.generate_yolo_datasets_from_excels, task="obb")


def dataset_labels(tmp_path, task):
    """{split/file name: text} of the label files generate_yolo_datasets_from_excels writes on `_frames`"""
    (tmp_path / task).mkdir()
    res = _run(_frames(tmp_path / task, True), tmp_path / task, P.generate_yolo_datasets_from_excels, backend=SegBackend(), task=task)
    root = res["datasets"][0] / "labels"
    return {str(p.relative_to(root)): p.read_text(encoding="utf-8") for p in sorted(root.rglob("*.txt"))}


@pytest.mark.parametrize("task", ["detect", "segment"])
def test_detect_and_segment_datasets_are_unchanged(tmp_path, task):
    want = json.loads(GOLDEN.read_text(encoding="utf-8"))[task]
    assert len(want) == 40 and dataset_labels(tmp_path, task) == want


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        Path(sys.argv[1]).write_text(json.dumps({t: dataset_labels(Path(d), t) for t in ("detect", "segment")}, indent=1) + "\n",
                                     encoding="utf-8")
