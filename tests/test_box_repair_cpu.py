"""Box repair (core/processor.py: repair_boxes_*), host side: one known answer per action, the edges of the rules, the native
emitter against json.dumps, the step functions and their CSV route, and the invariants (idempotence, the audit after the repair,
YOLO label lines in [0, 1]) — driven by a test backend whose device stage is the numpy restatement of tests/box_repair_ref.py.
No GPU."""
import json
import math
import random

import numpy as np
import pandas as pd
import pytest

from box_audit_ref import audit_arrays
from box_repair_ref import ACTIONS, check_repair, repair_arrays, repair_table
from helpers import OracleBackend

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd import native_json as nj
from deal_yolo_daya_amd.core import processor as P

COL = P.BBOX_COL


class RepairBackend(OracleBackend):
    def repair_boxes(self, box4, row_off, cls, width, height, size_status, n_classes, min_visibility, min_size):
        return repair_arrays(box4, row_off, cls, width, height, size_status, n_classes, min_visibility, min_size)

    def box_audit(self, box4, row_off, cls, width, height, size_status, n_classes, nbins):
        return audit_arrays(box4, row_off, cls, width, height, size_status, n_classes, nbins)


BE = RepairBackend()


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def repair(cells, widths, heights, min_visibility=0.0, min_size=0.0, **kw):
    stats = {}
    res = P.repair_boxes_cells(cells, widths, heights, min_visibility, min_size, backend=BE, stats=stats, **kw)
    check_repair(res, repair_table(cells, widths, heights, min_visibility, min_size), cells, stats)
    return res + (stats,)


def one(c, w=640, h=480, **kw):
    """the repair of a one-row table: (output cell, changes frame, per_class frame indexed by class)"""
    out, ch, pc, _ = repair([c], [w], [h], **kw)
    return out[0], ch, pc.set_index("class")


def actions_of(c, w=640, h=480, **kw):
    return one(c, w, h, **kw)[1]["action"].tolist()


# ----------------------------------------------------------------------------------------------- known answers
def test_keep_leaves_the_cell_object_untouched():
    c = cell(ob("a", [(10, 10), (20, 30)]))
    out, ch, pc = one(c)
    assert out is c and len(ch) == 0 and pc.loc["a", "keep"] == 1 and pc.loc["a", "boxes"] == 1


def test_clip_replaces_the_ptlist_with_two_float_corners():
    c = cell(ob("a", [(-10, 5), (700, 500)], extra=1))
    out, ch, pc = one(c)
    assert json.loads(out)["objects"] == [{"name": "a", "polygon": {"ptList": [{"x": 0.0, "y": 5.0}, {"x": 640.0, "y": 480.0}]},
                                           "extra": 1}]
    assert '"x": 0.0' in out and pc.loc["a", "clip"] == 1
    assert ch[["action", "nx1", "ny1", "nx2", "ny2"]].values.tolist() == [["clip", 0.0, 5.0, 640.0, 480.0]]


def test_no_size_leaves_even_a_broken_box():
    c = cell(ob("a", [(-10, 5), (-10, 5)]))
    out, ch, pc = one(c, 0, 480)
    assert out is c and pc.loc["a", "no_size"] == 1 and len(ch) == 0


@pytest.mark.parametrize("pts,action", [([(math.nan, 1), (3, 4)], "bad_coords"), ([(5, 5)], "degenerate"),
                                        ([(700, 10), (800, 20)], "outside")])
def test_removed_actions(pts, action):
    c = cell(ob("a", [(1, 1), (9, 9)]), ob("a", pts))
    out, ch, pc = one(c)
    assert json.loads(out)["objects"] == [ob("a", [(1, 1), (9, 9)])]
    assert ch["action"].tolist() == [action] and ch["object"].tolist() == [1] and pc.loc["a", action] == 1
    assert np.isnan(ch[["nx1", "ny1", "nx2", "ny2"]].to_numpy()).all()


def test_low_visibility_and_small():
    c = cell(ob("a", [(-90, 0), (10, 10)]), ob("b", [(0, 0), (3, 50)]), ob("c", [(0, 0), (50, 50)]))
    assert actions_of(c, min_visibility=0.5, min_size=4) == ["low_visibility", "small"]
    assert actions_of(c, min_visibility=0.1, min_size=4) == ["clip", "small"]
    assert actions_of(c) == ["clip"]


def test_rules_are_tested_in_order():
    # outside before low_visibility before small, bad_coords before degenerate
    c = cell(ob("a", [(-10, 0), (0, 5)]), ob("a", [(-100, 0), (1, 1)]), ob("a", [(math.inf, 0), (math.inf, 0)]))
    assert actions_of(c, min_visibility=1.0, min_size=100) == ["outside", "low_visibility", "bad_coords"]


# ----------------------------------------------------------------------------------------------- edges
def test_edge_exactly_at_the_size_is_kept_one_ulp_past_is_clipped():
    past = np.nextafter(640.0, 1e9)
    c = cell(ob("a", [(0, 0), (640, 480)]), ob("a", [(0, 0), (past, 480)]))
    out, ch, pc = one(c)
    assert ch["action"].tolist() == ["clip"] and ch["object"].tolist() == [1]
    assert ch["x2"].iloc[0] == past and ch["nx2"].iloc[0] == 640.0
    objs = json.loads(out)["objects"]
    assert objs[0] == ob("a", [(0, 0), (640, 480)]) and objs[1]["polygon"]["ptList"][1] == {"x": 640.0, "y": 480.0}


def test_negative_zero_is_not_outside_and_stays_negative_when_clipped():
    c = cell(ob("a", [(-0.0, 0), (10, 10)]))
    out, ch, _ = one(c)
    assert out is c and len(ch) == 0
    c2 = cell(ob("a", [(-0.0, 0), (641, 10)]))
    out2, ch2, _ = one(c2)
    assert ch2["action"].tolist() == ["clip"] and '"x": -0.0' in out2 and math.copysign(1, ch2["nx1"].iloc[0]) == -1


def test_clip_that_leaves_zero_width_is_outside():
    assert actions_of(cell(ob("a", [(640, 0), (700, 10)]))) == ["outside"]
    assert actions_of(cell(ob("a", [(-50, 0), (0, 10)]))) == ["outside"]


def test_visibility_exactly_at_the_threshold_is_kept():
    # visible 50 x 10 of 100 x 10: 500 == 0.5 * 1000 exactly
    c = cell(ob("a", [(-50, 0), (50, 10)]))
    assert actions_of(c, min_visibility=0.5) == ["clip"]
    assert actions_of(c, min_visibility=np.nextafter(0.5, 1)) == ["low_visibility"]
    assert actions_of(cell(ob("a", [(0, 0), (4, 4)])), min_size=4) == []


def test_nan_inside_the_list_follows_first_wins_min_max():
    c = '{"objects": [{"name": "a", "polygon": {"ptList": [{"x": -5, "y": 1}, {"x": NaN, "y": 9}]}}]}'
    out, ch, _ = one(c)
    assert ch["action"].tolist() == ["degenerate"]                       # (min x, max x) = (-5, -5)
    c2 = '{"objects": [{"name": "a", "polygon": {"ptList": [{"x": NaN, "y": 1}, {"x": 5, "y": 9}]}}]}'
    assert actions_of(c2) == ["bad_coords"]


def test_inf_string_and_null_coordinates_are_removed():
    c = cell(ob("a", [(1, 1), (math.inf, 9)]), ob("a", [("1", "2"), ("3", "4")]), ob("a", [(None, 1)]), ob("a", [(1, 1), (9, 9)]))
    out, ch, pc = one(c)
    assert ch["action"].tolist() == ["bad_coords"] * 3 and pc.loc["a", "keep"] == 1
    assert json.loads(out)["objects"] == [ob("a", [(1, 1), (9, 9)])]


def test_non_str_and_empty_names():
    c = json.dumps({"objects": [ob(3, [(-1, 1), (9, 9)]), ob("", [(-1, 1), (9, 9)]), ob(None, [(700, 1), (800, 9)]),
                                ob(True, [(700, 1), (800, 9)]), ob("a", [(1, 1), (9, 9)])]})
    out, ch, pc = one(c)
    assert ch["name"].tolist() == [3, True] and ch["action"].tolist() == ["clip", "outside"]
    assert list(pc.index) == ["a"] and pc.loc["a", "boxes"] == 1
    objs = json.loads(out)["objects"]
    assert len(objs) == 4 and objs[1] == ob("", [(-1, 1), (9, 9)]) and objs[2] == ob(None, [(700, 1), (800, 9)])


def test_non_dict_objects_keep_their_indices():
    c = json.dumps({"objects": [5, "s", None, ob("a", [(700, 0), (800, 9)]), [1], ob("a", [(-3, 0), (9, 9)]), {}]})
    out, ch, _ = one(c)
    assert ch["object"].tolist() == [3, 5] and ch["action"].tolist() == ["outside", "clip"]
    objs = json.loads(out)["objects"]
    assert objs[:3] == [5, "s", None] and objs[3] == [1] and objs[5] == {} and objs[4]["polygon"]["ptList"][0] == {"x": 0.0, "y": 0.0}


def test_many_point_polygons():
    pts = [(math.cos(t) * 100 + 200, math.sin(t) * 50 + 100) for t in np.linspace(0, 6.2, 300)]
    inside = cell(ob("poly", pts))
    out, ch, _ = one(inside)
    assert out is inside
    shifted = cell(ob("poly", [(x + 400, y) for x, y in pts]))
    out, ch, _ = one(shifted)
    ptl = json.loads(out)["objects"][0]["polygon"]["ptList"]
    assert len(ptl) == 2 and ptl[1]["x"] == 640.0 and ch["action"].tolist() == ["clip"]


def test_int_coordinates_become_floats_only_in_clipped_boxes():
    c = cell(ob("a", [(1, 2), (3, 4)]), ob("a", [(-1, 2), (3, 4)]))
    out, _, _ = one(c)
    objs = json.loads(out)["objects"]
    assert objs[0] == ob("a", [(1, 2), (3, 4)]) and isinstance(objs[0]["polygon"]["ptList"][0]["x"], int)
    assert objs[1]["polygon"]["ptList"] == [{"x": 0.0, "y": 2.0}, {"x": 3.0, "y": 4.0}]


def test_non_ascii_names_and_text():
    c = cell(ob("猫", [(-1, 0), (5, 5)], note="é "), ob("é", [(1, 1), (2, 2)]))
    out, ch, pc = one(c)
    assert "猫" in out and "\\u" not in out and list(pc.index) == ["é", "猫"]
    assert out == json.dumps(json.loads(out), ensure_ascii=False)


def test_size_columns_missing_or_odd():
    c = cell(ob("a", [(-1, 0), (5, 5)]))
    out, ch, pc, st = repair([c, c, c], [None, "640", 640], [480, 480, 480])
    assert out[0] is c and out[1] is c and out[2] != c and st["rows_no_size"] == 2
    df = pd.DataFrame({COL: [c]})
    o, ch, pc = P.repair_boxes_frame(df, backend=BE)
    assert o[COL].iloc[0] is c and pc["no_size"].tolist() == [1]


# ----------------------------------------------------------------------------------------------- native emitter
def _rand_value(rng):
    return rng.choice([1, 2.5, -3, 0, -0.0, 1e308, 5e-324, 2 ** 60, 5, 1e22, 123456789.125])


def _rand_cell(rng):
    objs = []
    for _ in range(rng.randint(0, 7)):
        if rng.random() < 0.05:
            objs.append(rng.choice([5, "s", None, [], {"x": [1, {"y": 2}]}]))
            continue
        o = {}
        if rng.random() < 0.3:
            o["id"] = rng.randint(0, 9)
        if rng.random() < 0.9:
            o["name"] = rng.choice(["a", "b", "", "猫", "c,d", None, "a\"q", "é\n", "b"])
        if rng.random() < 0.9:
            pts = []
            for _ in range(rng.randint(0, 5)):
                p = {}
                if rng.random() < 0.9:
                    p["x"] = _rand_value(rng) if rng.random() < 0.1 else rng.randint(-50, 700)
                if rng.random() < 0.9:
                    p["y"] = _rand_value(rng) if rng.random() < 0.1 else round(rng.uniform(-50, 500), 3)
                if rng.random() < 0.1:
                    p["z"] = "☃"
                pts.append(p)
            poly = {"ptList": pts}
            if rng.random() < 0.3:
                poly = {"type": "polygon", **poly, "closed": True}
            o["polygon"] = poly
        if rng.random() < 0.3:
            o["attrs"] = {"t": rng.random(), "u": [1.5, None, "猫"]}
        objs.append(o)
    doc = {"objects": objs}
    if rng.random() < 0.5:
        doc = {"width": 3, **doc, "tail": [1e-7, 1e16, 12345678901234567890]}
    text = json.dumps(doc, ensure_ascii=rng.random() < 0.5)
    return text if rng.random() < 0.8 else text.replace(", ", ",").replace(": ", ":")


def _respell(c, action, box, obj):
    doc = json.loads(c)
    objs = doc["objects"]
    drop = set()
    for a, bx, k in zip(action, box, obj):
        if a == 1:
            objs[k]["polygon"]["ptList"] = [{"x": bx[0], "y": bx[1]}, {"x": bx[2], "y": bx[3]}]
        elif a >= 3:
            drop.add(k)
    doc["objects"] = [o for k, o in enumerate(objs) if k not in drop]
    return json.dumps(doc, ensure_ascii=False)


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_emit_repaired_matches_json_dumps(threads):
    rng = random.Random(100 + threads)
    cells = [_rand_cell(rng) for _ in range(3000)]
    s = nj.scan_named_boxes(cells, n_threads=threads)
    try:
        nb = s.n_boxes
        nrng = np.random.default_rng(threads)
        action = nrng.choice(8, nb, p=[0.5, 0.2, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05]).astype(np.uint8)
        action |= np.where(nrng.random(nb) < 0.1, 0x80, 0).astype(np.uint8)          # the class bit is ignored
        box = nrng.choice([0.0, -0.0, 1.5, 640.0, 1e-5, 1e17, 0.1 + 0.2, 123.456], (nb, 4))
        changed, strs = s.emit_repaired(action, box, n_threads=threads)
        code = action & 7
        k = 0
        n_changed = 0
        for i, c in enumerate(cells):
            b0, b1 = int(s.cell_box_off[i]), int(s.cell_box_off[i + 1])
            touched = ((code[b0:b1] == 1) | (code[b0:b1] >= 3)).any()
            assert changed[i] == (1 if touched else 0), i
            if touched:
                assert strs[k] == _respell(c, code[b0:b1], box[b0:b1].tolist(), s.box_object[b0:b1].tolist()), i
                k += 1
                n_changed += 1
        assert k == len(strs) and n_changed > 500
    finally:
        s.close()


def test_repair_cell_matches_the_native_emitter():
    c = cell(ob("a", [(1, 2), (3, 4)], k=[1, 2]), 7, ob("b", [(5, 6), (7, 8), (9, 10)]), ob("c", [(0, 0), (1, 1)]))
    s = nj.scan_named_boxes([c])
    try:
        changed, strs = s.emit_repaired(np.asarray([1, 5, 0], np.uint8), np.asarray([[0.5, -0.0, 3, 4], [0] * 4, [0] * 4], float))
    finally:
        s.close()
    assert changed.tolist() == [1]
    assert strs[0] == fl.repair_cell(c, {0: (0.5, -0.0, 3, 4), 2: None})


# ----------------------------------------------------------------------------------------------- step functions
def _table(n=500, seed=0):
    rng = np.random.default_rng(seed)
    cells = []
    for i in range(n):
        objs = []
        for k in range(int(rng.integers(0, 9))):
            x, y = float(rng.integers(-60, 700)), float(rng.integers(-60, 520))
            objs.append(ob(f"c{int(rng.integers(0, 6))}", [(x, y), (x + float(rng.choice([0, 3, 40, 90])), y + 30.5)]))
        if rng.random() < 0.05:
            objs.append(ob(5, [(-1, 0), (9, 9)]))                              # an irregular cell (numeric name)
        cells.append(cell(*objs))
    w = rng.choice([640.0, 0.0, np.nan], n, p=[0.9, 0.05, 0.05])
    return pd.DataFrame({"source": [f"s{i}.jpg" for i in range(n)], COL: cells, "width": w, "height": 480})


def test_frame_matches_the_restatement_and_only_the_json_column_differs():
    df = _table()
    st = {}
    out, ch, pc = P.repair_boxes_frame(df, min_visibility=0.25, min_size=2.0, backend=BE, stats=st)
    ref = repair_table(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), 0.25, 2.0)
    check_repair((out[COL].tolist(), ch, pc), ref, None, st)
    assert out.drop(columns=[COL]).equals(df.drop(columns=[COL])) and out.index.equals(df.index)
    assert ch["source"].tolist() == [df["source"][r] for r in ch["row"]]
    assert ch[["row", "object"]].apply(tuple, axis=1).is_monotonic_increasing
    assert st["python_cells"] > 0 and st["boxes_clipped"] > 0 and st["boxes_removed"] > 0


def test_chunks_merge_their_classes():
    df = _table(400, seed=4)
    old = P._NATIVE_CHUNK_CELLS
    P._NATIVE_CHUNK_CELLS = 37
    try:
        repair(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), 0.5, 1.0)
    finally:
        P._NATIVE_CHUNK_CELLS = old


def test_lone_surrogate_chunk_goes_through_cpython():
    c = '{"objects": [{"name": "a", "polygon": {"ptList": [{"x": -1, "y": 0}, {"x": 5, "y": 5}]}}], "t": "\\ud800"}'
    cells = [json.loads(json.dumps(c)), cell(ob("b", [(-2, 0), (5, 5)]))]
    out, ch, pc, st = repair(cells, [640, 640], [480, 480])
    assert st["python_cells"] >= 1 and ch["action"].tolist() == ["clip", "clip"]


def test_csv_route_writes_what_the_pandas_route_writes(tmp_path, monkeypatch):
    df = _table(700, seed=3)
    df["note"] = "x"
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    kw = dict(min_visibility=0.3, min_size=1.5, backend=BE)
    res = P.repair_boxes_csv(src, tmp_path / "n.csv", tmp_path / "nc.csv", tmp_path / "nk.csv", **kw)
    assert P.LAST_IO_PATH["repair"] == "native"
    monkeypatch.setattr(P._fc, "enabled", lambda: False)
    res2 = P.repair_boxes_csv(src, tmp_path / "p.csv", tmp_path / "pc.csv", tmp_path / "pk.csv", **kw)
    assert P.LAST_IO_PATH["repair"] == "pandas"
    for a, b in (("n.csv", "p.csv"), ("nc.csv", "pc.csv"), ("nk.csv", "pk.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes(), a
    strip = ("output", "changes_output", "classes_output")
    assert {k: v for k, v in res.items() if k not in strip} == {k: v for k, v in res2.items() if k not in strip}
    ref = repair_table(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), 0.3, 1.5)
    for k, v in ref["totals"].items():
        assert res[k] == v, k
    back = pd.read_csv(tmp_path / "n.csv", encoding="utf-8-sig")
    assert back[COL].tolist() == ref["cells"] and back["note"].tolist() == ["x"] * len(df)
    assert set(res) == {"rows", "rows_changed", "boxes", "boxes_clipped", "boxes_removed", "rows_no_size", "python_cells",
                        "output", "changes_output", "classes_output"}


def test_csv_error_conventions(tmp_path, capsys):
    assert P.repair_boxes_csv(tmp_path / "nope.csv", tmp_path / "o.csv", backend=BE) is None
    assert "读取失败：" in capsys.readouterr().out
    p = tmp_path / "x.csv"
    pd.DataFrame({"a": [1]}).to_csv(p, index=False)
    assert P.repair_boxes_csv(p, tmp_path / "o.csv", backend=BE) is None
    assert f"错误：缺少必要列 {COL}" in capsys.readouterr().out
    assert not (tmp_path / "o.csv").exists()


@pytest.mark.parametrize("kw", [dict(min_visibility=-0.1), dict(min_visibility=1.5), dict(min_visibility=math.nan),
                                dict(min_size=-1), dict(min_size=math.inf), dict(min_size=math.nan), dict(min_size="2"),
                                dict(min_visibility=None), dict(min_visibility=True)])
def test_argument_validation(kw, tmp_path):
    with pytest.raises(ValueError):
        P.repair_boxes_cells([cell()], [1], [1], backend=BE, **kw)
    with pytest.raises(ValueError):
        P.repair_boxes_csv(tmp_path / "nope.csv", tmp_path / "o.csv", backend=BE, **kw)


def test_backend_and_size_arguments_are_checked():
    with pytest.raises(TypeError, match="repair_boxes"):
        P.repair_boxes_cells([cell()], [1], [1], backend=OracleBackend())
    with pytest.raises(ValueError):
        P.repair_boxes_cells([cell(), cell()], [1], [1, 1], backend=BE)
    with pytest.raises(ValueError):
        P.repair_boxes_cells([cell()], [1], None, backend=BE)


# ----------------------------------------------------------------------------------------------- invariants
def _yolo_numbers(texts):
    vals = []
    for t in texts:
        for line in (t.split("\n") if t else []):
            vals += [float(v) for v in line.split()[1:]]
    return np.asarray(vals, np.float64)


def test_invariants_idempotence_audit_and_yolo_lines():
    df = _table(600, seed=9)
    w, h = df["width"].tolist(), df["height"].tolist()
    cells = df[COL].tolist()
    before = P.audit_boxes_cells(cells, w, h, backend=BE)
    out, ch, pc = P.repair_boxes_cells(cells, w, h, backend=BE)
    again, ch2, pc2 = P.repair_boxes_cells(out, w, h, backend=BE)
    assert len(ch2) == 0 and all(a is b for a, b in zip(again, out))
    assert pc2["clip"].sum() == 0 and pc2[list(ACTIONS[3:])].to_numpy().sum() == 0
    after = P.audit_boxes_cells(out, w, h, backend=BE)
    apc = after.per_class.set_index("class")
    assert (apc[["bad_coords", "degenerate", "out_of_image"]].to_numpy() == 0).all()
    rpc = pc.set_index("class")
    for c in apc.index:
        assert apc.loc[c, "writable"] == rpc.loc[c, "keep"] + rpc.loc[c, "clip"], c
        assert apc.loc[c, "no_size"] == rpc.loc[c, "no_size"], c
    assert before.per_class["out_of_image"].sum() > 0
    # label lines of the rows with a usable size (a NaN width is `no_size`: the repair leaves it, the YOLO step writes nan)
    ok = np.flatnonzero(after.per_row["size_status"].to_numpy() == "ok")
    labels = [f"c{k % 6}" for k in ok]
    sub = [out[k] for k in ok]
    texts, _ = P.yolo_label_texts(sub, labels, [k % 6 for k in ok], [w[k] for k in ok], [h[k] for k in ok], backend=BE)
    nums = _yolo_numbers(texts)
    assert len(nums) > 100 and ((nums >= 0) & (nums <= 1)).all()
    raw, _ = P.yolo_label_texts([cells[k] for k in ok], labels, [k % 6 for k in ok], [w[k] for k in ok], [h[k] for k in ok],
                                backend=BE)
    rn = _yolo_numbers(raw)
    assert ((rn < 0) | (rn > 1)).any()                    # the unrepaired table does write such lines
