"""Box audit (core/processor.py: audit_boxes_*), host side: spelled-out known answers, the native named-box scan against
utils._extract_boxes_with_labels, the step functions and their CSV route, and a cross-check with the YOLO step — driven by a
test backend whose device stage is the numpy restatement of tests/box_audit_ref.py.  No GPU."""
import json
import math
import random

import numpy as np
import pandas as pd
import pytest

from box_audit_ref import audit_arrays, audit_table, check_audit
from helpers import OracleBackend

from deal_yolo_daya_amd import native_json as nj
from deal_yolo_daya_amd.core import processor as P
from deal_yolo_daya_amd.core.utils import _extract_boxes_with_labels

COL = P.BBOX_COL


class AuditBackend(OracleBackend):
    def box_audit(self, box4, row_off, cls, width, height, size_status, n_classes, nbins):
        return audit_arrays(box4, row_off, cls, width, height, size_status, n_classes, nbins)


BE = AuditBackend()


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def audit(cells, widths, heights, nbins=16, **kw):
    a = P.audit_boxes_cells(cells, widths, heights, nbins=nbins, backend=BE, **kw)
    check_audit(a, audit_table(cells, widths, heights, nbins))
    return a


def one(c, w=640, h=480, nbins=16):
    """the audit of a one-row table: (per_row dict, per_class frame indexed by class, problems frame)"""
    a = audit([c], [w], [h], nbins)
    return a.per_row.iloc[0].to_dict(), a.per_class.set_index("class"), a.problems, a


# ----------------------------------------------------------------------------------------------- known answers
def test_inverted_points_give_the_min_max_box():
    r, pc, pb, a = one(cell(ob("a", [(100, 90), (20, 10)])))
    assert r["writable"] == 1 and r["out_of_image"] == 0
    assert a.hist_xy[0].sum() == 1
    xc, yc = (20 + 100) / 2 / 640, (10 + 90) / 2 / 480
    assert a.hist_xy[0, int(xc * 16), int(yc * 16)] == 1
    assert a.hist_wh[0, int(80 / 640 * 16), int(80 / 480 * 16)] == 1
    assert pc.loc["a", "medium"] == 1 and len(pb) == 0          # 80 * 80 = 6400


def test_one_point_ptlist_is_degenerate():
    r, pc, pb, _ = one(cell(ob("a", [(5, 5)])))
    assert r["degenerate"] == 1 and r["n_boxes"] == 1
    assert pb[["object", "name", "issue"]].values.tolist() == [[0, "a", "degenerate"]]


def test_edge_touching_and_a_hair_past():
    r, pc, pb, _ = one(cell(ob("a", [(0, 0), (640, 480)]), ob("a", [(0, 0), (640.0000001, 480)]),
                            ob("a", [(-0.0, 0), (10, 10)])))
    assert r["writable"] == 3 and r["out_of_image"] == 1
    assert pb["object"].tolist() == [1] and pb["issue"].tolist() == ["out_of_image"]
    assert pc.loc["a", "large"] == 2 and pc.loc["a", "small"] == 1


@pytest.mark.parametrize("box", [[(-1, 0), (5, 5)], [(0, -1), (5, 5)], [(0, 0), (641, 5)], [(0, 0), (5, 481)]])
def test_each_side_out_of_image(box):
    r, _, pb, _ = one(cell(ob("a", box)))
    assert r["out_of_image"] == 1 and pb["issue"].tolist() == ["out_of_image"]


def test_nan_and_infinity_coordinates():
    c = '{"objects": [%s, %s, %s]}' % (json.dumps(ob("a", [(1, 2), (3, 4)])).replace('"x": 1', '"x": NaN'),
                                       json.dumps(ob("b", [(1, 2), (3, 4)])).replace('"y": 4', '"y": Infinity'),
                                       json.dumps(ob("c", [(1, 2), (30, 40)])))
    r, pc, pb, _ = one(c)
    assert r["bad_coords"] == 2 and r["writable"] == 1
    assert pb["issue"].tolist() == ["bad_coords", "bad_coords"]
    assert math.isinf(pb["y2"].iloc[1])


def test_nan_inside_the_list_follows_first_wins_min_max():
    c = '{"objects": [{"name": "a", "polygon": {"ptList": [{"x": 5, "y": 1}, {"x": NaN, "y": 9}]}}]}'
    assert _extract_boxes_with_labels(c) == [("a", 5, 1, 5, 9)]
    r, _, _, _ = one(c)
    assert r["degenerate"] == 1


def test_string_and_null_coordinates_are_bad_not_raising():
    r, pc, pb, _ = one(cell(ob("a", [("1", "2"), ("3", "4")]), ob("a", [(None, 1)]), ob("a", [(1, 1), (9, 9)])))
    assert r["bad_coords"] == 2 and r["writable"] == 1
    assert pb["issue"].tolist() == ["bad_coords", "bad_coords"] and np.isnan(pb["x1"].iloc[0])
    a = P.audit_boxes_cells([cell(ob("a", [(1, 1), ("x", 9)]), ob("b", [(1, 1), (9, 9)]))], [640], [480], backend=BE)
    assert a.totals["boxes"] == 0                       # min() of int and str raises: the walk keeps the (empty) prefix


def test_non_str_names_are_unmatchable():
    r, pc, _, a = one(cell(ob(3, [(1, 1), (9, 9)]), ob(True, [(1, 1), (9, 9)]), ob(["x"], [(1, 1), (9, 9)]),
                           ob("a", [(1, 1), (9, 9)]), ob(0, [(1, 1), (9, 9)])))
    assert r["n_boxes"] == 4 and r["unmatchable"] == 3 and a.totals["unmatchable_name_boxes"] == 3
    assert a.classes == ["a"]


def test_unnamed_and_non_dict_objects_are_skipped_with_their_index_kept():
    c = json.dumps({"objects": [5, {"polygon": {"ptList": [{"x": 1, "y": 1}]}}, ob("", [(0, 0), (1, 1)]), "s",
                                ob("a", [(0, 0), (0, 1)]), ob(None, [(0, 0), (1, 1)])]})
    r, _, pb, _ = one(c)
    assert r["n_boxes"] == 1 and pb["object"].tolist() == [4]


def test_polygon_of_many_points():
    pts = [(math.cos(t) * 100 + 200, math.sin(t) * 50 + 100) for t in np.linspace(0, 6.2, 300)]
    r, pc, _, a = one(cell(ob("poly", pts)))
    assert r["writable"] == 1
    box = _extract_boxes_with_labels(cell(ob("poly", pts)))[0]
    bw, bh = box[3] - box[1], box[4] - box[2]
    assert a.hist_wh[0, math.floor(bw / 640 * 16), math.floor(bh / 480 * 16)] == 1


@pytest.mark.parametrize("w,h,status", [(0, 480, "missing"), (None, 480, "missing"), ("", 480, "missing"),
                                        (float("nan"), 480, "invalid"), (-5, 480, "invalid"), ("640", 480, "invalid"),
                                        (True, True, "ok"), (640, float("inf"), "invalid"), (10 ** 400, 5, "invalid"),
                                        (640.0, np.int64(480), "ok")])
def test_size_status(w, h, status):
    c = cell(ob("a", [(0, 0), (0.5, 0.5)]))
    r, pc, _, _ = one(c, w, h)
    assert r["size_status"] == status
    assert (r["no_size"] == 1) == (status != "ok")
    if status == "ok" and w is True:
        assert r["out_of_image"] == 0 and r["writable"] == 1     # W = H = 1.0


def test_numeric_size_columns_take_the_numpy_route_with_the_same_answer():
    cells = [cell(ob("a", [(0, 0), (10, 10)]))] * 5
    w = np.asarray([640.0, 0.0, np.nan, -3.0, 10.0])
    h = np.asarray([480, 480, 480, 480, 5])
    a = audit(cells, w, h)
    assert a.per_row["size_status"].tolist() == ["ok", "missing", "invalid", "invalid", "ok"]
    assert a.per_row["out_of_image"].tolist() == [0, 0, 0, 0, 1]


def test_exact_bin_edges_and_the_last_bin():
    # xc = 0.5, yc = 0.25, wn = 0.5, hn = 1.0: v * nb is an integer; v = 1.0 lands in the last bin
    c = cell(ob("a", [(160, 0), (480, 240)]), ob("a", [(0, 0), (640, 480)]))
    for nb in (1, 4, 16, 64):
        _, _, _, a = one(c, 640, 480, nb)
        assert a.hist_xy[0, min(nb // 2, nb - 1), min(nb // 4, nb - 1)] >= 1
        assert a.hist_wh[0, nb - 1, nb - 1] == (2 if nb == 1 else 1) and a.hist_wh[0, min(nb // 2, nb - 1), min(nb // 2, nb - 1)] >= 1


def test_overflowing_boxes_clamp_into_the_bins():
    c = cell(ob("a", [(-1e308, 0), (1e308, 10)]))
    r, pc, _, a = one(c, 640, 480, 8)
    assert r["writable"] == 1 and r["out_of_image"] == 1 and pc.loc["a", "large"] == 1
    assert a.hist_wh[0, 7, 0] == 1


def test_nbins_range_is_checked():
    for nb in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            P.audit_boxes_cells([cell()], [1], [1], nbins=nb, backend=BE)


def test_frame_without_size_columns_and_backend_check():
    df = pd.DataFrame({COL: [cell(ob("a", [(0, 0), (9, 9)])), None, "not json"]})
    a = P.audit_boxes_frame(df, backend=BE)
    assert a.per_row["size_status"].tolist() == ["missing"] * 3 and a.per_class["no_size"].tolist() == [1]
    assert "source" not in a.per_row.columns
    with pytest.raises(TypeError, match="box_audit"):
        P.audit_boxes_frame(df, backend=OracleBackend())


def test_boxes_per_image_and_images():
    cells = [cell(*[ob("a" if k % 2 else "b", [(0, 0), (1, 1)]) for k in range(n)]) for n in (0, 1, 3, 255, 256, 300)]
    a = audit(cells, [640] * 6, [480] * 6)
    assert a.boxes_per_image[[0, 1, 3, 255, 256]].tolist() == [1, 1, 1, 1, 2] and a.boxes_per_image.sum() == 6
    assert a.per_class.set_index("class")["images"].to_dict() == {"a": 4, "b": 5}


# ----------------------------------------------------------------------------------------------- scan fuzz
def _rand_value(rng):
    return rng.choice([1, 2.5, -3, 0, "7", None, True, 1e308, 10 ** 20, 2 ** 60, 5, [1], {"a": 1}])


def _rand_cell(rng):
    r = rng.random()
    if r < 0.03:
        return None
    if r < 0.05:
        return "{bad"
    if r < 0.06:
        return "[1, 2]"
    objs = []
    for _ in range(rng.randint(0, 7)):
        if rng.random() < 0.05:
            objs.append(rng.choice([5, "s", None, []]))
            continue
        o = {}
        if rng.random() < 0.9:
            o["name"] = rng.choice(["a", "b", "", "猫", "c,d", None, 3, True, "a", "é", "b"])
        if rng.random() < 0.9:
            pts = []
            for _ in range(rng.randint(0, 5)):
                p = {}
                if rng.random() < 0.9:
                    p["x"] = _rand_value(rng) if rng.random() < 0.1 else rng.randint(-5, 700)
                if rng.random() < 0.9:
                    p["y"] = _rand_value(rng) if rng.random() < 0.1 else round(rng.uniform(-5, 500), 3)
                pts.append(p if rng.random() < 0.95 else [1, 2])
            o["polygon"] = {"ptList": pts} if rng.random() < 0.97 else []
        objs.append(o)
    return json.dumps({"objects": objs, "width": 3}, ensure_ascii=rng.random() < 0.5)


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_named_box_scan_matches_the_python_walk(threads):
    rng = random.Random(threads)
    cells = [_rand_cell(rng) for _ in range(4000)]
    s = nj.scan_named_boxes(cells, n_threads=threads)
    regular = 0
    for i, c in enumerate(cells):
        if s.status[i] == nj.IRREGULAR:
            continue
        regular += 1
        want = [(k, nm, *xy) for k, (nm, *xy) in zip([None] * 99, _extract_boxes_with_labels(c))]
        b0, b1 = int(s.cell_box_off[i]), int(s.cell_box_off[i + 1])
        got = [(s.names[s.box_class[b]], *s.box4[b].tolist()) for b in range(b0, b1)]
        assert [g[0] for g in got] == [w[1] for w in want]
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g[1:], float), np.asarray(w[2:], float), equal_nan=True)
        from box_audit_ref import boxes_of
        assert s.box_object[b0:b1].tolist() == [k for k, *_ in boxes_of(c)]
    order = []
    for b in s.box_class.tolist():                      # ids numbered by first occurrence, whatever the thread count
        if b not in order:
            order.append(b)
    assert order == list(range(len(s.names))) and regular > 1000
    ref = nj.scan_named_boxes(cells, n_threads=1)
    assert s.names == ref.names and np.array_equal(s.box_class, ref.box_class)
    s.close()
    ref.close()


def test_fuzzed_tables_through_the_step_function():
    rng = random.Random(5)
    cells = [_rand_cell(rng) for _ in range(3000)]
    sizes = [rng.choice([640, 0, None, float("nan"), "7", 480.5, True, -1]) for _ in cells]
    a = audit(cells, sizes, [rng.choice([480, 480, 0]) for _ in cells], nbins=8)
    assert a.totals["python_cells"] > 0
    old = P._NATIVE_CHUNK_CELLS
    P._NATIVE_CHUNK_CELLS = 257                          # several chunks: class ids merge across them
    try:
        b = P.audit_boxes_cells(cells, sizes, [480] * len(cells), nbins=8, backend=BE)
    finally:
        P._NATIVE_CHUNK_CELLS = old
    check_audit(b, audit_table(cells, sizes, [480] * len(cells), 8))


# ----------------------------------------------------------------------------------------------- step functions
def _table(n=400, seed=0):
    rng = np.random.default_rng(seed)
    cells = []
    for i in range(n):
        objs = []
        for k in range(int(rng.integers(0, 9))):
            x, y = float(rng.integers(-20, 700)), float(rng.integers(-20, 500))
            objs.append(ob(f"c{int(rng.integers(0, 6))}", [(x, y), (x + float(rng.integers(0, 90)), y + 30.5)]))
        cells.append(cell(*objs))
    w = rng.choice([640.0, 0.0, np.nan], n, p=[0.9, 0.05, 0.05])
    return pd.DataFrame({"source": [f"s{i}.jpg" for i in range(n)], COL: cells, "width": w, "height": 480})


def test_frame_matches_the_restatement():
    df = _table()
    a = P.audit_boxes_frame(df, nbins=32, backend=BE)
    check_audit(a, audit_table(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), 32))
    assert a.per_row["source"].tolist() == df["source"].tolist()
    assert a.problems["source"].tolist() == [df["source"][r] for r in a.problems["row"]]
    assert list(a.problems.columns) == ["source", "row", "object", "name", "issue", "x1", "y1", "x2", "y2"]
    pr = a.problems
    assert pr[["row", "object"]].apply(tuple, axis=1).is_monotonic_increasing


def test_csv_route_writes_what_the_pandas_route_writes(tmp_path, monkeypatch):
    df = _table(600, seed=3)
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    res = P.audit_boxes_csv(src, tmp_path / "native", nbins=16, backend=BE)
    assert P.LAST_IO_PATH["audit"] == "native"
    monkeypatch.setattr(P._fc, "enabled", lambda: False)
    res2 = P.audit_boxes_csv(src, tmp_path / "pandas", nbins=16, backend=BE)
    assert P.LAST_IO_PATH["audit"] == "pandas"
    for k in ("classes", "problems"):
        assert open(res["paths"][k], "rb").read() == open(res2["paths"][k], "rb").read()
    z1, z2 = np.load(res["paths"]["hist"]), np.load(res2["paths"]["hist"])
    for k in ("classes", "hist_wh", "hist_xy", "boxes_per_image"):
        assert np.array_equal(z1[k], z2[k])
    assert {k: v for k, v in res.items() if k != "paths"} == {k: v for k, v in res2.items() if k != "paths"}
    ref = audit_table(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), 16)
    assert pd.read_csv(res["paths"]["classes"], encoding="utf-8-sig")["class"].tolist() == ref["classes"]
    assert res["boxes"] == sum(r["n_boxes"] for r in ref["rows"])


def test_csv_error_conventions(tmp_path, capsys):
    assert P.audit_boxes_csv(tmp_path / "nope.csv", tmp_path / "o", backend=BE) is None
    assert "读取失败：" in capsys.readouterr().out
    p = tmp_path / "x.csv"
    pd.DataFrame({"a": [1]}).to_csv(p, index=False)
    assert P.audit_boxes_csv(p, tmp_path / "o", backend=BE) is None
    assert f"错误：缺少必要列 {COL}" in capsys.readouterr().out


# ----------------------------------------------------------------------------------------------- YOLO cross-check
def test_writable_counts_agree_with_the_yolo_step():
    rng = np.random.default_rng(11)
    n = 300
    labels = [f"L{int(k)}" for k in rng.integers(0, 4, n)]
    cells = []
    for i in range(n):
        objs = []
        for _ in range(int(rng.integers(0, 6))):
            x, y = float(rng.integers(-10, 650)), float(rng.integers(-10, 490))
            dx = float(rng.choice([0, 0, 12, 40]))
            objs.append(ob(labels[i], [(x, y), (x + dx, y + float(rng.choice([0, 7, 90])))]))
        cells.append(cell(*objs))
    w = rng.choice([640, 0], n, p=[0.9, 0.1]).astype(np.int64)
    h = np.full(n, 480, np.int64)
    a = P.audit_boxes_cells(cells, w, h, backend=BE)
    texts, reasons = P.yolo_label_texts(cells, labels, [int(v[1:]) for v in labels], w, h, backend=BE)
    pr = a.per_row
    ok = (pr["size_status"] == "ok").to_numpy()
    lines = np.asarray([len(t.split("\n")) if t else 0 for t in texts])
    assert np.array_equal(lines[ok], pr["writable"].to_numpy()[ok])
    invalid = {i for i, r in enumerate(reasons) if r == P.REASON_NO_VALID_BOX}
    assert invalid == set(np.flatnonzero(ok & (pr["n_boxes"].to_numpy() > 0) & (pr["writable"].to_numpy() == 0)).tolist())

