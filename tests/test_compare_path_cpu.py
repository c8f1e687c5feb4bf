"""The path the box comparison and the polygon comparison share (core/processor.py: compare_boxes_* and compare_polygons_*), host
side.  One table of integer rectangles goes to the box step as two-point boxes and to the polygon step as four-corner polygons:
the two steps must tell one story.  And calls with several faults at once: the fault that wins is the one that won before the
two steps shared their entry bodies.  Backends are the tests' restatements.  No GPU."""
import contextlib
import io
import json

import numpy as np
import pandas as pd
import pytest

import box_compare_ref
import polygon_compare_ref
from helpers import OracleBackend

from deal_yolo_daya_amd.core import processor as P

TWIN_W, TWIN_H, TWIN_ROWS = 40, 30, 24
TWIN_NAMES = ("a", "b", "c", 7)
TWIN_CONFIGS = [(thr, by_label) for thr in (0.3, 0.5, 1.0) for by_label in (False, True)]


class RefBackend(OracleBackend):
    def compare_boxes(self, *args):
        return box_compare_ref.compare_rows(*args)

    def compare_polygons(self, *args):
        return polygon_compare_ref.compare_arrays(*args)[:15]


BE = RefBackend()


# ----------------------------------------------------------------------------------------------- the twin table
def twin_rects(seed=7):
    """-> per side, per row a list of (name, x1, y1, x2, y2): 0 to 5 integer rectangles with x1 < x2 <= 40 and y1 < y2 <= 30.
    About 70 % of B's are copies of one of the row's A rectangles, half of those grown by 0 to 2 pixels a side (kept inside the
    image) and a fifth renamed."""
    rng = np.random.default_rng(seed)

    def rect():
        x1, y1 = int(rng.integers(0, TWIN_W)), int(rng.integers(0, TWIN_H))
        return [TWIN_NAMES[int(rng.integers(0, 4))], x1, y1, int(rng.integers(x1 + 1, TWIN_W + 1)), int(rng.integers(y1 + 1, TWIN_H + 1))]

    side_a, side_b = [], []
    for _ in range(TWIN_ROWS):
        a = [rect() for _ in range(int(rng.integers(0, 6)))]
        b = []
        for _ in range(int(rng.integers(0, 6))):
            if a and rng.random() < 0.7:
                r = list(a[int(rng.integers(0, len(a)))])
                if rng.random() < 0.5:
                    g = rng.integers(0, 3, 4)
                    r[1:] = [max(r[1] - int(g[0]), 0), max(r[2] - int(g[1]), 0), min(r[3] + int(g[2]), TWIN_W), min(r[4] + int(g[3]), TWIN_H)]
                if rng.random() < 0.2:
                    r[0] = TWIN_NAMES[(TWIN_NAMES.index(r[0]) + 1 + int(rng.integers(0, 3))) % 4]
                b.append(r)
            else:
                b.append(rect())
        side_a.append([tuple(r) for r in a])
        side_b.append([tuple(r) for r in b])
    return side_a, side_b


def twin_cells(side, corners: int) -> list:
    """the rows of one side as annotation cells: two-point boxes (corners=2) or four-corner polygons (corners=4)"""
    def pts(x1, y1, x2, y2):
        return [(x1, y1), (x2, y2)] if corners == 2 else [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]

    return [json.dumps({"objects": [{"name": nm, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts(*r)]}} for nm, *r in row]})
            for row in side]


def twin_results(thr, by_label, backend):
    """-> (BoxComparison, PolygonComparison) of the twin table; backend=None: the device"""
    side_a, side_b = twin_rects()
    boxes = P.compare_boxes_cells(twin_cells(side_a, 2), twin_cells(side_b, 2), thr, by_label, backend=backend)
    polys = P.compare_polygons_cells(twin_cells(side_a, 4), twin_cells(side_b, 4), [TWIN_W] * TWIN_ROWS, [TWIN_H] * TWIN_ROWS, thr,
                                     by_label, backend=backend)
    return boxes, polys


def assert_one_story(boxes, polys, by_label):
    """The IoU columns are compared exactly: an integer rectangle inside the image covers exactly (x2-x1)*(y2-y1) pixel centres,
    so both steps divide the same two integers in double precision."""
    assert boxes.classes == polys.classes == ["a", "b", "c", None]
    pd.testing.assert_frame_equal(boxes.confusion, polys.confusion)
    assert boxes.hist_iou.dtype == polys.hist_iou.dtype and np.array_equal(boxes.hist_iou, polys.hist_iou)
    cols = ["agree", "relabelled", "missing", "extra"]
    pd.testing.assert_frame_equal(boxes.per_row[cols], polys.per_row[cols])
    assert (polys.per_row["status"] == "compared").all()
    db, dp = boxes.differences, polys.differences
    for c in ("row", "kind", "a_object", "b_object", "iou", "best_iou"):
        assert db[c].dtype == dp[c].dtype and db[c].tolist() == dp[c].tolist(), c          # the floats bit for bit
    for c in ("a_name", "b_name"):
        assert [None if not isinstance(v, str) else v for v in db[c]] == dp[c].tolist(), c
    assert 7 in db["a_name"].tolist() and 7 in db["b_name"].tolist()                       # the box step lists the name itself
    assert 7 not in dp["a_name"].tolist() and 7 not in dp["b_name"].tolist()
    t = boxes.totals
    assert {k: t[k] for k in cols} == {k: polys.totals[k] for k in cols}
    assert t["agree"] > 0 and t["missing"] > 0 and t["extra"] > 0 and (t["relabelled"] > 0) != by_label    # none passes empty
    assert boxes.hist_iou.sum() == t["agree"] and set(db["kind"]) == {"missing", "extra"} | (set() if by_label else {"relabelled"})


@pytest.mark.parametrize("thr,by_label", TWIN_CONFIGS)
def test_the_two_steps_tell_one_story(thr, by_label):
    assert_one_story(*twin_results(thr, by_label, BE), by_label)


def test_the_twin_table_is_what_it_says():
    side_a, side_b = twin_rects()
    rects = [r for side in (side_a, side_b) for row in side for r in row]
    assert len(side_a) == len(side_b) == TWIN_ROWS and all(len(row) <= 5 for row in side_a + side_b)
    assert all(0 <= x1 < x2 <= TWIN_W and 0 <= y1 < y2 <= TWIN_H for _, x1, y1, x2, y2 in rects)
    assert {r[0] for r in rects} == set(TWIN_NAMES) and any(not row for row in side_a) and any(not row for row in side_b)
    copies = sum(r[1:] in [q[1:] for q in a] for a, b in zip(side_a, side_b) for r in b)
    assert 0.2 * len(rects) / 2 < copies < 0.7 * len(rects) / 2


# ----------------------------------------------------------------------------------------------- which fault wins
def ob(name, *pts):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def fault_frames():
    """-> (df_a, df_b) with both annotation columns and the sizes: four rows, B's keys in another order with one of its own"""
    sq = [(0, 0), (4, 4)]
    cells_a = [cell(ob("a", *sq)), cell(ob("b", *sq), ob("a", (4, 4), (8, 8))), cell(ob("c", (1, 1), (5, 5))), cell()]
    cells_b = [cell(ob("a", (4, 4), (8, 8))), cell(ob("a", *sq)), cell(ob("x", (1, 1), (2, 2))), cell(ob("c", (1, 1), (5, 5)))]
    both = lambda cells: {P.BBOX_COL: pd.Series(cells, dtype=object), P.ANNOTATION_COL: pd.Series(cells, dtype=object)}   # noqa: E731
    df_a = pd.DataFrame({"source": ["u0", "u1", "u2", "u3"], **both(cells_a), "width": 8, "height": 8})
    df_b = pd.DataFrame({"source": ["u1", "u0", "u9", "u2"], **both(cells_b), "width": 8, "height": 8})
    return df_a, df_b


def fault_files(d):
    """the frames of fault_frames and their variants as CSVs under d -> {name: path}; "nope" does not exist"""
    df_a, df_b = fault_frames()
    files = {"a": df_a, "b": df_b, "short": df_b.iloc[:3], "dup": pd.concat([df_b, df_b.iloc[:1]]),
             "nokey": df_b.drop(columns=["source"]), "nojson": df_b.drop(columns=[P.BBOX_COL, P.ANNOTATION_COL])}
    paths = {"nope": d / "nope.csv"}
    for name, frame in files.items():
        paths[name] = d / f"{name}.csv"
        frame.to_csv(paths[name], index=False, encoding="utf-8-sig")
    return paths


LACKS = OracleBackend()                                  # a backend without the two compare entries
C1 = [cell(ob("a", (0, 0), (2, 2)))]


def _frames(fn, a="a", b="b", **kw):
    def call(_):
        df_a, df_b = fault_frames()
        dup = pd.concat([df_b, df_b.iloc[:1]], ignore_index=True)
        pick = {"a": df_a, "b": df_b, "short": df_b.iloc[:3], "dup": dup, "nokey": df_b.drop(columns=["source"]), None: None,
                "dup_a": pd.concat([df_a, df_a.iloc[:1]], ignore_index=True)}
        return fn(pick[a], pick[b], **{"backend": BE, **kw})
    return call


def _files(fn, a, b, **kw):
    def call(d):
        f = fault_files(d)
        return fn(f[a], f[b], d / "out", **{"backend": BE, **kw})
    return call


def _outcome_of(kind, text):
    return lambda *args: (kind, text.format(*args))


THR = _outcome_of("ValueError", "iou_threshold must be a number, got {}")
MAX_PIXELS = _outcome_of("ValueError", "max_pixels_per_row must be an int in 1..1073741824, got {}")
BY_POSITION = _outcome_of("ValueError", "without a key the {} are compared by position: 4 against {} rows")
DUPLICATE = _outcome_of("ValueError", "the {} table holds the key '{}' of column 'source' more than once: run the dedup step "
                        "(dedup_frame / deduplicate_csv_by_source) on it first")
NO_COLUMN = _outcome_of("printed", "错误：缺少必要列 {}\n")
UNREADABLE = ("printed", "读取失败：[Errno 2] No such file or directory: '<tmp>/nope.csv'\n")
OTHER_COL = ("ValueError", "with one frame, other_col names the column to compare json_col against")
LACKS_BOXES, LACKS_POLYGONS = ("TypeError", "backend lacks ['compare_boxes']"), ("TypeError", "backend lacks ['compare_polygons']")

# (id, call(tmp dir), outcome on the commit before the two steps shared their entry bodies): an outcome is (exception type, its
# text) or ("printed", the printed text with the tmp dir as <tmp>) for a call that returns None
FAULTS = [
    # --- compare_boxes_cells
    ("boxes_cells: threshold, lengths", lambda _: P.compare_boxes_cells(C1, C1 + C1, "0.5", backend=BE),
     THR("'0.5'")),
    ("boxes_cells: threshold, backend", lambda _: P.compare_boxes_cells(C1, C1, True, backend=LACKS),
     THR(True)),
    ("boxes_cells: backend, lengths", lambda _: P.compare_boxes_cells(C1, C1 + C1, backend=LACKS),
     LACKS_BOXES),
    # --- compare_boxes_frame
    ("boxes_frame: threshold, other_col", _frames(P.compare_boxes_frame, b=None, iou_threshold=None),
     THR(None)),
    ("boxes_frame: threshold, lengths", _frames(P.compare_boxes_frame, b="short", key=None, iou_threshold="1"),
     THR("'1'")),
    ("boxes_frame: threshold, duplicate key", _frames(P.compare_boxes_frame, b="dup", iou_threshold=[0.5]),
     THR([0.5])),
    ("boxes_frame: other_col, backend", _frames(P.compare_boxes_frame, b=None, backend=LACKS),
     OTHER_COL),
    ("boxes_frame: lengths, backend", _frames(P.compare_boxes_frame, b="short", key=None, backend=LACKS),
     BY_POSITION("frames", 3)),
    ("boxes_frame: lengths, column", _frames(P.compare_boxes_frame, b="short", key=None, other_col="nowhere"),
     BY_POSITION("frames", 3)),
    ("boxes_frame: duplicate key both sides", _frames(P.compare_boxes_frame, a="dup_a", b="dup"),
     DUPLICATE("base", "u0")),
    ("boxes_frame: duplicate key, backend", _frames(P.compare_boxes_frame, b="dup", backend=LACKS),
     DUPLICATE("other", "u1")),
    ("boxes_frame: duplicate key, key column", _frames(P.compare_boxes_frame, a="dup_a", b="nokey"),
     ("KeyError", "'source'")),
    # --- compare_boxes_csv
    ("boxes_csv: threshold, unreadable", _files(P.compare_boxes_csv, "nope", "b", iou_threshold="x"),
     THR("'x'")),
    ("boxes_csv: unreadable, key column", _files(P.compare_boxes_csv, "nope", "nokey"),
     UNREADABLE),
    ("boxes_csv: key column, unreadable", _files(P.compare_boxes_csv, "nokey", "nope"),
     NO_COLUMN("source")),
    ("boxes_csv: json column, key column", _files(P.compare_boxes_csv, "nojson", "nokey"),
     NO_COLUMN(P.BBOX_COL)),
    ("boxes_csv: lengths, json column", _files(P.compare_boxes_csv, "a", "nojson", key=None),
     NO_COLUMN(P.BBOX_COL)),
    ("boxes_csv: lengths, backend", _files(P.compare_boxes_csv, "a", "short", key=None, backend=LACKS),
     BY_POSITION("files", 3)),
    ("boxes_csv: duplicate key, backend", _files(P.compare_boxes_csv, "a", "dup", backend=LACKS),
     DUPLICATE("other", "u1")),
    # --- compare_polygons_cells
    ("polygons_cells: threshold, max_pixels", lambda _: P.compare_polygons_cells(C1, C1, [4], [4], "0.5", max_pixels_per_row=0, backend=BE),
     THR("'0.5'")),
    ("polygons_cells: max_pixels, backend", lambda _: P.compare_polygons_cells(C1, C1, [4], [4], max_pixels_per_row=0, backend=LACKS),
     MAX_PIXELS(0)),
    ("polygons_cells: backend, lengths", lambda _: P.compare_polygons_cells(C1, C1 + C1, [4], [4], backend=LACKS),
     LACKS_POLYGONS),
    ("polygons_cells: lengths, sizes", lambda _: P.compare_polygons_cells(C1, C1 + C1, [4, 4], [4], backend=BE),
     ("ValueError", "the two lists must hold one cell per image each: 1 against 2 cells")),
    # --- compare_polygons_frame
    ("polygons_frame: max_pixels, other_col", _frames(P.compare_polygons_frame, b=None, max_pixels_per_row=0),
     MAX_PIXELS(0)),
    ("polygons_frame: batch_pairs, backend", _frames(P.compare_polygons_frame, b="short", key=None, batch_pairs=0, backend=LACKS),
     ("ValueError", "batch_pairs must be an int in 1..1099511627776, got 0")),
    ("polygons_frame: backend, other_col", _frames(P.compare_polygons_frame, b=None, backend=LACKS),
     LACKS_POLYGONS),
    ("polygons_frame: backend, lengths", _frames(P.compare_polygons_frame, b="short", key=None, backend=LACKS),
     LACKS_POLYGONS),
    ("polygons_frame: lengths, column", _frames(P.compare_polygons_frame, b="short", key=None, other_col="nowhere"),
     BY_POSITION("frames", 3)),
    ("polygons_frame: duplicate key both sides", _frames(P.compare_polygons_frame, a="dup_a", b="dup"),
     DUPLICATE("base", "u0")),
    ("polygons_frame: duplicate key, key column", _frames(P.compare_polygons_frame, a="dup_a", b="nokey"),
     ("KeyError", "'source'")),
    # --- compare_polygons_csv
    ("polygons_csv: max_pixels, unreadable", _files(P.compare_polygons_csv, "nope", "b", max_pixels_per_row=2 ** 30 + 1),
     MAX_PIXELS(2 ** 30 + 1)),
    ("polygons_csv: backend, unreadable", _files(P.compare_polygons_csv, "nope", "b", backend=LACKS),
     LACKS_POLYGONS),
    ("polygons_csv: unreadable, key column", _files(P.compare_polygons_csv, "nope", "nokey"),
     UNREADABLE),
    ("polygons_csv: key column, unreadable", _files(P.compare_polygons_csv, "nokey", "nope"),
     NO_COLUMN("source")),
    ("polygons_csv: json column, key column", _files(P.compare_polygons_csv, "nojson", "nokey"),
     NO_COLUMN(P.ANNOTATION_COL)),
    ("polygons_csv: lengths, json column", _files(P.compare_polygons_csv, "a", "nojson", key=None),
     NO_COLUMN(P.ANNOTATION_COL)),
    ("polygons_csv: lengths, duplicate key", _files(P.compare_polygons_csv, "a", "dup", key=None),
     BY_POSITION("files", 5)),
]


def outcome(call, d):
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            res = call(d)
    except Exception as e:          # noqa: BLE001 - the type is part of the outcome
        return type(e).__name__, str(e).replace(str(d), "<tmp>")
    assert res is None, "every call here has a fault"
    return "printed", out.getvalue().replace(str(d), "<tmp>")


@pytest.mark.parametrize("call,want", [pytest.param(c, w, id=i) for i, c, w in FAULTS])
def test_the_same_fault_wins(call, want, tmp_path):
    assert outcome(call, tmp_path) == want
    assert not (tmp_path / "out").exists()
