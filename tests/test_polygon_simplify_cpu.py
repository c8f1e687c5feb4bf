"""Polygon simplification (core/processor.py: simplify_polygons_*), host side: one known answer per action, the edges of the
rule, the native emitter against flatten.simplify_cell and json.dumps, the step functions and their CSV route, and the
invariants (idempotence, dev2 <= e2, the three-vertex floor, no repeats, the audit afterwards) — driven by a test backend whose
device stage is the restatement of tests/polygon_simplify_ref.py; tests/test_gpu_polygon_simplify.py checks K19 itself.
No GPU."""
import json
import math
import random

import numpy as np
import pandas as pd
import pytest

import polygon_audit_ref as A
import polygon_simplify_ref as R
from helpers import OracleBackend

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd import native_json as nj
from deal_yolo_daya_amd.core import processor as P

COL = P.ANNOTATION_COL


class SimplifyBackend(OracleBackend):
    def simplify_polygons(self, xy, pt_off, tolerance=1.0):
        return R.simplify_arrays(xy, pt_off, tolerance)

    def audit_polygons(self, xy, pt_off, row_off, cls, width, height, status, n_classes, min_area=1.0):
        return A.audit_arrays(xy, pt_off, row_off, cls, width, height, status, n_classes, min_area)


BE = SimplifyBackend()


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def simp(cells, tolerance=1.0, **kw):
    stats = {}
    res = P.simplify_polygons_cells(cells, tolerance, backend=BE, stats=stats, **kw)
    R.check_simplify(res, R.simplify_table(cells, tolerance), cells, stats)
    return res + (stats,)


def one(c, tolerance=1.0):
    """the simplification of a one-row table: (output cell, changes frame, per_class frame indexed by class)"""
    out, ch, pc, _ = simp([c], tolerance)
    return out[0], ch, pc.set_index("class")


def kept_points(out, k=0):
    return [(p["x"], p["y"]) for p in json.loads(out)["objects"][k]["polygon"]["ptList"]]


def fl_pts(pts):
    return [(float(x), float(y)) for x, y in pts]


# ----------------------------------------------------------------------------------------------- known answers
def test_one_known_answer_per_action():
    square = [(0, 0), (10, 0), (10, 10), (0, 10)]
    c = cell(ob("a", square),                                            # kept
             ob("a", [(0, 0), (5, 0), (10, 0), (10, 10), (0, 10)]),      # simplified: (5, 0) goes
             ob("b", [(0, 0), (math.inf, 0), (10, 10), (0, 10)]),        # bad_coords
             ob("b", [(0, 0), (10, 0), (5, 0)]))                         # too_few_points
    out, ch, pc = one(c, 0.0)
    objs = json.loads(out)["objects"]
    assert objs[0] == ob("a", square) and kept_points(out, 1) == square
    assert objs[2] == json.loads(c)["objects"][2] and objs[3] == ob("b", [(0, 0), (10, 0), (5, 0)])
    assert pc.loc["a", ["polygons", "kept", "simplified", "points_in", "points_out"]].tolist() == [2, 1, 1, 9, 8]
    assert pc.loc["b", ["bad_coords", "too_few_points", "points_in", "points_out"]].tolist() == [1, 1, 7, 7]
    assert ch[["object", "name", "points", "kept", "max_deviation"]].values.tolist() == [[1, "a", 5, 4, 0.0]]


def test_coordinate_at_the_bound_is_bad_coords():
    V = fl_pts([(0, 0), (5, 0), (10, 0), (10, 10)])
    assert R.simplify(V, 0.0)[1] == 1
    assert R.simplify(V[:3] + [(10.0, 2.0 ** 43)], 0.0)[1] == 2 and R.simplify(V[:3] + [(math.nan, 1.0)], 0.0)[1] == 2
    assert R.simplify(V[:3] + [(10.0, -np.nextafter(2.0 ** 43, 0))], 0.0)[1] == 1


def test_square_with_midpoints_becomes_its_corners_at_tolerance_zero():
    pts = [(0, 0), (5, 0), (10, 0), (10, 5), (10, 10), (5, 10), (0, 10), (0, 5)]
    out, ch, _ = one(cell(ob("a", pts)), 0)
    assert kept_points(out) == [(0, 0), (10, 0), (10, 10), (0, 10)]
    assert ch[["points", "kept", "max_deviation"]].values.tolist() == [[8, 4, 0.0]]
    assert '"x": 10, "y": 0' in out                                      # the values keep their spelling


def test_distance_exactly_the_tolerance_is_removed_the_next_one_above_is_kept():
    tol = 2.0
    up = float(np.nextafter(tol, 3.0))
    base = [(0.0, 0.0), (50.0, tol), (100.0, 0.0), (100.0, 50.0), (0.0, 50.0)]
    keep, act, kept, dev2 = R.simplify(base, tol)
    assert keep == [1, 0, 1, 1, 1] and act == 1 and dev2 == tol * tol
    base[1] = (50.0, up)                                                 # c = 100 * up, s = (c * c) / 10000 = up * up > e2
    assert R.dist2(base[0], base[2], base[1]) > tol * tol
    keep, act, kept, dev2 = R.simplify(base, tol)
    assert keep == [1] * 5 and act == 0 and dev2 == 0.0
    out, ch, _ = one(cell(ob("a", [(0.0, 0.0), (50.0, tol), (100.0, 0.0), (100.0, 50.0), (0.0, 50.0)])), tol)
    assert len(kept_points(out)) == 4 and ch["max_deviation"].tolist() == [tol]


def test_forced_split_keeps_three_vertices_of_a_sliver():
    V = fl_pts([(0, 0), (10, 1), (20, 2), (30, 0), (20, -1), (10, -3)])
    # b = 3; s*(0, 3) = 4 at k = 2, s*(3, 6) = 9 at k = 5: neither exceeds 100^2, the larger one splits anyway
    assert R.farthest(V, 0, 3) == (4.0, 2) and R.farthest(V, 3, 6) == (9.0, 5)
    keep, act, kept, dev2 = R.simplify(V, 100.0)
    assert keep == [1, 0, 0, 1, 0, 1] and (act, kept) == (1, 3)
    assert dev2 == max(4.0, R.farthest(V, 3, 5)[0])
    out, ch, _ = one(cell(ob("a", V)), 100.0)
    assert kept_points(out) == [V[0], V[3], V[5]] and ch["kept"].tolist() == [3]
    # a tie goes to (0, b)
    T = fl_pts([(0, 0), (10, 2), (30, 0), (10, -2)])
    assert R.simplify(T, 100.0)[0] == [1, 1, 1, 0]


def test_all_coincident_points_are_untouched():
    c = cell(ob("a", [(3, 3)] * 6))
    out, ch, pc = one(c, 5.0)
    assert out is c and len(ch) == 0 and pc.loc["a", "kept"] == 1 and pc.loc["a", "points_out"] == 6


def test_b_on_a_tie_goes_to_the_lowest_index():
    V = fl_pts([(0, 0), (10, 0), (0, 10), (-10, 0), (0, -10)])           # four vertices at distance 10
    keep, act, kept, _ = R.simplify(V, 0.5)
    assert keep == [1] * 5                                               # b = 1: (0, 1) has no interior
    # with b = 1 the vertex (0, 10) is interior to (1, 5); were b = 2, vertex 1 would be judged against (0, 2) instead
    V2 = fl_pts([(0, 0), (6, 8), (10, 0), (6, -8), (5, 0)])              # |V1| = |V2| = |V3| = 10
    assert R._anchor(V2) == (100.0, 1)


def test_b_first_and_last_leave_a_root_without_interior():
    first = fl_pts([(0, 0), (100, 0), (50, 1), (20, 1), (10, 1)])        # b = 1
    keep, act, kept, dev2 = R.simplify(first, 2.0)
    assert R._anchor(first)[1] == 1 and keep[0] == keep[1] == 1 and kept == 3 and act == 1
    last = fl_pts([(0, 0), (10, 1), (20, 1), (50, 1), (100, 0)])         # b = m - 1
    keep, act, kept, dev2 = R.simplify(last, 2.0)
    assert R._anchor(last)[1] == 4 and keep == [1, 1, 0, 0, 1] and dev2 == R.farthest(last, 1, 4)[0]   # s = 1 thrice: the lowest k
    for V in (first, last):
        out, ch, _ = one(cell(ob("a", V)), 2.0)
        assert len(kept_points(out)) == 3


def test_closing_repeat_is_removed():
    V = [(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]
    out, ch, _ = one(cell(ob("a", V)), 0)
    assert kept_points(out) == V[:4] and ch[["points", "kept"]].values.tolist() == [[5, 4]]


def test_spike_is_judged_by_end_point_distance():
    P_, Q = (0.0, 0.0), (10.0, 0.0)
    assert R.dist2(P_, Q, (-3.0, 4.0)) == 25.0                           # t < 0: distance to P, not to the line (16)
    assert R.dist2(P_, Q, (13.0, 4.0)) == 25.0                           # t > L2: distance to Q
    assert R.dist2(P_, Q, (5.0, 4.0)) == 16.0
    assert R.dist2(P_, P_, (3.0, 4.0)) == 25.0                           # L2 == 0
    # the spike tip is 1 from the line through its segment but 5 from the segment: kept at tolerance 2
    V = fl_pts([(0, 0), (-3, 1), (-3, 0), (0, -1), (40, 0), (40, 40), (0, 40)])
    keep = R.simplify(V, 2.0)[0]
    assert keep[1] == 1 or keep[2] == 1
    out, _, _ = one(cell(ob("a", V)), 2.0)
    assert len(kept_points(out)) == sum(keep)


def test_rounds_form_equals_the_recursive_form():
    rnd = random.Random(3)
    for _ in range(1500):
        V = _grid_polygon(rnd, rnd.randint(4, 40))
        tol = rnd.choice([0, 0.5, 1, 2.5, 7, 100])
        assert R.simplify(V, tol) == R.simplify_rounds(V, tol)


# ----------------------------------------------------------------------------------------------- native emitter
def _grid_polygon(rnd, n):
    span = rnd.choice([3, 8, 30])
    V = [(float(rnd.randint(0, span)), float(rnd.randint(0, span))) for _ in range(n)]
    if rnd.random() < 0.3:
        k = rnd.randrange(n)
        V[k] = V[k - 1]
    if rnd.random() < 0.2:
        V[-1] = V[0]
    if rnd.random() < 0.2:                                               # a collinear run
        k = rnd.randrange(n)
        for d in range(min(4, n - k)):
            V[k + d] = (float(k + d), 1.0)
    return V


def _rand_cell(rng, irregular=True):
    objs = []
    for _ in range(rng.randint(0, 5)):
        if rng.random() < 0.05:
            objs.append(rng.choice([5, "s", None, [], {"x": [1, {"y": 2}]}]))
            continue
        o = {}
        if rng.random() < 0.3:
            o["id"] = rng.randint(0, 9)
        if rng.random() < 0.95:
            o["name"] = rng.choice(["a", "b", "", "猫", "c,d", None, "a\"q", "é\n", "b"])
            if irregular and rng.random() < 0.03:
                o["name"] = rng.choice([5, True, 2.5])
        if rng.random() < 0.95:
            pts = []
            for x, y in _grid_polygon(rng, rng.randint(1, 14)):
                r = rng.random()
                if r < 0.04:
                    pts.append(rng.choice([7, None, "p", [1, 2], {}, {"x": 1}, {"y": 2, "z": 3}]))   # no vertex: stays
                p = {"x": int(x) if rng.random() < 0.5 else x, "y": y if rng.random() < 0.7 else int(y)}
                if rng.random() < 0.05:
                    p = {"y": p["y"], "t": "☃", "x": p["x"]}
                if rng.random() < 0.02:
                    p["x"] = rng.choice([1e308, 5e-324, 0.1 + 0.2, -0.0, 1e22])
                if irregular and rng.random() < 0.01:
                    p["x"] = rng.choice(["3", None, 2 ** 60])
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


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_emit_simplified_matches_simplify_cell(threads):
    rng = random.Random(200 + threads)
    cells = [_rand_cell(rng) for _ in range(2500)]
    s = nj.scan_named_polygons(cells, n_threads=threads)
    try:
        nrng = np.random.default_rng(threads)
        keep = (nrng.random(int(s.pt_off[-1])) < 0.7).astype(np.uint8)
        whole = nrng.random(s.n_boxes) < 0.5                              # half of the polygons lose nothing
        keep[np.repeat(whole, np.diff(s.pt_off))] = 1
        changed, strs = s.emit_simplified(keep, n_threads=threads)
        k = n_changed = 0
        for i, c in enumerate(cells):
            b0, b1 = int(s.cell_box_off[i]), int(s.cell_box_off[i + 1])
            dec = {int(s.box_object[b]): keep[s.pt_off[b]:s.pt_off[b + 1]].tolist() for b in range(b0, b1)
                   if not keep[s.pt_off[b]:s.pt_off[b + 1]].all()}
            assert changed[i] == (1 if dec else 0), i
            if dec:
                want = fl.simplify_cell(c, dec)
                assert strs[k] == want, i
                doc = json.loads(c)                                       # only vertices left: everything else as json.dumps
                for ko, flags in dec.items():
                    pl = doc["objects"][ko]["polygon"]["ptList"]
                    n_vert = sum(isinstance(p, dict) and "x" in p and "y" in p for p in pl)
                    assert len(json.loads(want)["objects"][ko]["polygon"]["ptList"]) == len(pl) - (n_vert - sum(flags))
                k += 1
                n_changed += 1
        assert k == len(strs) and n_changed > 300 and (s.status == nj.IRREGULAR).sum() > 10
    finally:
        s.close()


def test_non_vertex_entries_extra_keys_and_spellings_stay():
    c = ('{"objects": [{"id": 1, "name": "猫", "polygon": {"type": "p", "ptList": [{"x": 0, "y": 0.0}, 7, {"x": 5, "y": 0, "t": "☃"}, '
         '{"x": 1}, {"y": 0.0, "x": 10.5}, null, {"x": 10.5, "y": 10}, {"x": 0, "y": 1e1}], "closed": true}, "k": [1, 2]}]}')
    out, ch, pc = one(c, 0)
    assert out == ('{"objects": [{"id": 1, "name": "猫", "polygon": {"type": "p", "ptList": [{"x": 0, "y": 0.0}, 7, '
                   '{"x": 1}, {"y": 0.0, "x": 10.5}, null, {"x": 10.5, "y": 10}, {"x": 0, "y": 10.0}], "closed": true}, "k": [1, 2]}]}')
    assert ch[["points", "kept"]].values.tolist() == [[5, 4]] and list(pc.index) == ["猫"]


def test_irregular_cells_and_odd_names_go_through_cpython():
    pts = [(0, 0), (5, 0), (10, 0), (10, 10), (0, 10)]
    c_num = json.dumps({"objects": [ob(5, pts), ob("a", pts)]})           # a numeric name: the scanner leaves the cell to CPython
    c_str = json.dumps({"objects": [ob("a", [("0", 0), ("5", 0), ("9", 0), ("9", 9)]), ob("b", pts)]})   # str coordinates: NaN
    c_sur = '{"objects": [' + json.dumps(ob("a", pts)) + '], "t": "\\ud800"}'
    cells = [c_num, c_str, json.loads(json.dumps(c_sur)), cell(ob("a", [(0, 0), (9, 9), (0, 9), (1, 1)]))]
    out, ch, pc, st = simp(cells, 0)
    assert st["python_cells"] >= 3 and ch["name"].tolist() == [5, "a", "b", "a"] and out[3] is cells[3]
    assert pc.set_index("class").loc["a", ["polygons", "simplified", "bad_coords", "kept"]].tolist() == [4, 2, 1, 1]
    assert kept_points(out[0], 0) == kept_points(out[0], 1) == [(0, 0), (10, 0), (10, 10), (0, 10)]


# ----------------------------------------------------------------------------------------------- step functions
def _table(n=400, seed=0, max_pts=30):
    rng = random.Random(seed)
    cells = []
    for i in range(n):
        objs = []
        for _ in range(rng.randint(0, 5)):
            m = rng.randint(0, max_pts) if rng.random() < 0.4 else rng.randint(0, 7)
            V = _grid_polygon(rng, m) if m else []
            objs.append(ob(f"c{rng.randint(0, 5)}", V))
        if rng.random() < 0.05:
            objs.append(ob(5, _grid_polygon(rng, 9)))                     # an irregular cell (numeric name)
        cells.append(cell(*objs) if rng.random() > 0.02 else None)
    return pd.DataFrame({"source": [f"s{i}.jpg" for i in range(n)], COL: cells, "width": 640, "height": 480})


def test_frame_matches_the_restatement_and_only_the_json_column_differs():
    df = _table()
    st = {}
    out, ch, pc = P.simplify_polygons_frame(df, tolerance=1.0, backend=BE, stats=st)
    ref = R.simplify_table(df[COL].tolist(), 1.0)
    R.check_simplify((out[COL].tolist(), ch, pc), ref, None, st)
    assert out.drop(columns=[COL]).equals(df.drop(columns=[COL])) and out.index.equals(df.index)
    assert ch["source"].tolist() == [df["source"][r] for r in ch["row"]]
    assert ch[["row", "object"]].apply(tuple, axis=1).is_monotonic_increasing
    assert st["python_cells"] > 0 and st["polygons_simplified"] > 50 and st["points_removed"] > 0
    assert set(st) == {"rows", "rows_changed", "polygons", "polygons_simplified", "points", "points_removed", "python_cells",
                       "tolerance"}
    same = [a is b for a, b in zip(out[COL].tolist(), df[COL].tolist())]
    assert sum(same) == len(df) - st["rows_changed"]


def test_chunks_merge_their_classes():
    df = _table(300, seed=4)
    old = P._NATIVE_CHUNK_CELLS
    P._NATIVE_CHUNK_CELLS = 37
    try:
        simp(df[COL].tolist(), 2.5)
    finally:
        P._NATIVE_CHUNK_CELLS = old


def test_csv_route_writes_what_the_frame_route_writes(tmp_path, monkeypatch):
    df = _table(500, seed=3)
    df["note"] = "x"
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    kw = dict(tolerance=1.5, backend=BE)
    res = P.simplify_polygons_csv(src, tmp_path / "n.csv", tmp_path / "nc.csv", tmp_path / "nk.csv", **kw)
    assert P.LAST_IO_PATH["simplify"] == "native"
    monkeypatch.setattr(P._fc, "enabled", lambda: False)
    res2 = P.simplify_polygons_csv(src, tmp_path / "p.csv", tmp_path / "pc.csv", tmp_path / "pk.csv", **kw)
    assert P.LAST_IO_PATH["simplify"] == "pandas"
    for a, b in (("n.csv", "p.csv"), ("nc.csv", "pc.csv"), ("nk.csv", "pk.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes(), a
    strip = ("output", "changes_output", "classes_output")
    assert {k: v for k, v in res.items() if k not in strip} == {k: v for k, v in res2.items() if k not in strip}
    back = pd.read_csv(tmp_path / "n.csv", encoding="utf-8-sig")
    ref = R.simplify_table(back[COL].where(back[COL].notna(), None).tolist(), 1.5)
    assert ref["totals"]["polygons_simplified"] == 0                     # and a second run finds nothing to do
    ref = R.simplify_table(df[COL].tolist(), 1.5)
    for k, v in ref["totals"].items():
        assert res[k] == v, k
    got = back[COL].where(back[COL].notna(), None).tolist()
    assert got == ref["cells"] and back["note"].tolist() == ["x"] * len(df)
    assert set(res) == {"rows", "rows_changed", "polygons", "polygons_simplified", "points", "points_removed", "python_cells",
                        "tolerance", "output", "changes_output", "classes_output"}


def test_csv_error_conventions(tmp_path, capsys):
    assert P.simplify_polygons_csv(tmp_path / "nope.csv", tmp_path / "o.csv", backend=BE) is None
    assert "读取失败：" in capsys.readouterr().out
    p = tmp_path / "x.csv"
    pd.DataFrame({"a": [1]}).to_csv(p, index=False)
    assert P.simplify_polygons_csv(p, tmp_path / "o.csv", backend=BE) is None
    assert f"错误：缺少必要列 {COL}" in capsys.readouterr().out
    assert not (tmp_path / "o.csv").exists()


@pytest.mark.parametrize("tol", [-0.1, math.nan, math.inf, 2.0 ** 43, "2", None, True])
def test_argument_validation(tol, tmp_path):
    with pytest.raises(ValueError):
        P.simplify_polygons_cells([cell()], tol, backend=BE)
    with pytest.raises(ValueError):
        P.simplify_polygons_csv(tmp_path / "nope.csv", tmp_path / "o.csv", tolerance=tol, backend=BE)


def test_backend_is_checked():
    with pytest.raises(TypeError, match="simplify_polygons"):
        P.simplify_polygons_cells([cell()], backend=OracleBackend())


# ----------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("tol", [0, 0.5, 1, 2.5, 7, 100])
def test_invariants_on_random_polygons(tol):
    rnd = random.Random(int(tol * 10) + 1)
    simplified = 0
    for _ in range(1200):
        V = _grid_polygon(rnd, rnd.randint(4, 50))
        keep, act, kept, dev2 = R.simplify(V, tol)
        assert dev2 <= tol * tol and kept == sum(keep) and keep[0] == 1
        if act == 0:
            assert kept == len(V) and dev2 == 0.0
            continue
        simplified += 1
        U = [v for v, k in zip(V, keep) if k]
        assert len(U) >= 3
        if len(U) >= 4:
            assert all(U[k] != U[k - 1] for k in range(len(U))), V
            assert R.simplify(U, tol)[1] == 0, V                          # a second run removes nothing
    assert simplified > 300


def test_second_run_changes_nothing_and_the_audit_finds_no_repeats():
    df = _table(500, seed=9, max_pts=45)
    cells = df[COL].tolist()
    out, ch, pc = P.simplify_polygons_cells(cells, 0, backend=BE)
    again, ch2, pc2 = P.simplify_polygons_cells(out, 0, backend=BE)
    # polygons cut down to three vertices are too_few_points now; none is simplified again
    assert len(ch2) == 0 and all(a is b for a, b in zip(again, out)) and pc2["simplified"].sum() == 0
    assert pc2["points_in"].sum() == pc["points_out"].sum()
    before = P.audit_polygons_cells(cells, [640] * len(cells), [480] * len(cells), backend=BE)
    after = P.audit_polygons_cells(out, [640] * len(out), [480] * len(out), backend=BE)
    assert before.totals["duplicate_vertices"] > 20
    dup = after.problems[after.problems["defects"].str.contains("duplicate_vertices")]
    assert (dup["points"] <= 3).all()
    assert after.totals["polygons"] == before.totals["polygons"]         # no object is dropped
