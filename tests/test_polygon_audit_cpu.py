"""Polygon audit (K14) on the host: the definition's worked answers, the defect predicate against exact arithmetic, the
categories against the segment step's actions, the native named-polygon scan, and the frame / CSV entries.  The device stage
is a stand-in built on tests/polygon_audit_ref.py; tests/test_gpu_polygon_audit.py checks K14 itself."""
import json
import random
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import polygon_audit_ref as R
import yolo_seg_ref as S
from helpers import OracleBackend
from test_yolo_seg_cpu import _plain, fuzz_cells

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd import native_json as nj
from deal_yolo_daya_amd.core import processor as P


class PolyBackend(OracleBackend):
    def audit_polygons(self, xy, pt_off, row_off, cls, width, height, status, n_classes, min_area=1.0):
        return R.audit_arrays(xy, pt_off, row_off, cls, width, height, status, n_classes, min_area)


BE = PolyBackend()


def ob(name, pts):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


WORKED = [   # (points, defects, area) on a 100 x 100 image
    ([(0, 0), (10, 10), (10, 0), (0, 10)], "self_intersecting|tiny_area", 0.0),
    ([(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], "duplicate_vertices", 100.0),
    ([(10, 10), (20, 20), (30, 30)], "self_intersecting|tiny_area", 0.0),
    ([(0, 0), (10, 0), (5, 0), (5, 5)], "self_intersecting", 12.5),
    ([(0, 0), (10, 0), (5, 5), (10, 10), (0, 10), (5, 5)], "self_intersecting", 50.0),
    ([(0, 0), (20, 0), (20, 5), (5, 5), (5, 20), (0, 20)], "", 175.0),
]


@pytest.mark.parametrize("pts,defects,area", WORKED)
def test_worked_answers(pts, defects, area):
    code, bits, a = R.polygon([(float(x), float(y)) for x, y in pts], 100.0, 100.0)
    assert S.ACTIONS[code] == "written" and a == area
    assert "|".join(d for k, d in enumerate(R.DEFECTS) if bits >> k & 1) == defects
    audit = P.audit_polygons_cells([cell(ob("k", pts))], [100], [100], backend=BE)
    assert audit.per_class["written"].tolist() == [1]
    if defects:
        row = audit.problems.iloc[0]
        assert (row["category"], row["defects"], row["points"], row["area"]) == ("written", defects, len(pts), area)
    else:
        assert audit.problems.empty


def test_one_polygon_per_category():
    c = cell(ob("a", [(10, 10), (50, 10), (50, 50)]),                 # written
             ob("a", [(-10, 10), (50, 10), (50, 50)]),                # clipped
             ob("b", [(10, float("inf")), (50, 10), (50, 50)]),       # bad_coords
             ob("b", [(10, 10)]),                                     # too_few_points
             ob("c", [(200, 200), (300, 200), (300, 300)]),           # empty: outside the image
             {"name": 7, "polygon": {"ptList": [{"x": 1, "y": 1}]}})  # unmatchable
    audit = P.audit_polygons_cells([c, cell(ob("a", [(1, 1), (5, 5)]))], [100, None], [100, 100], backend=BE)
    pc = audit.per_class.set_index("class")
    assert audit.classes == ["a", "b", "c"]
    assert pc.loc["a", "written"] == 1 and pc.loc["a", "clipped"] == 1 and pc.loc["a", "no_size"] == 1
    assert pc.loc["a", "polygons"] == 3 and pc.loc["a", "images"] == 2
    assert pc.loc["b", "bad_coords"] == 1 and pc.loc["b", "too_few_points"] == 1 and pc.loc["c", "empty"] == 1
    assert audit.totals["unmatchable_name_polygons"] == 1 and audit.totals["polygons"] == 7
    assert audit.problems["category"].tolist() == ["bad_coords", "too_few_points", "empty", "no_size"]
    assert audit.problems["object"].tolist() == [2, 3, 4, 0] and audit.problems["row"].tolist() == [0, 0, 0, 1]
    assert pc.loc["a", ["small", "medium", "large"]].tolist() == [1, 1, 0]
    assert audit.hist_vertices[0, 1] == 2 and audit.hist_vertices[0, 0] == 1


def test_hist_bins_and_area_buckets():
    assert [R.hist_bin(n) for n in (0, 2, 3, 4, 5, 8, 9, 1024, 1025)] == [0, 0, 1, 2, 3, 3, 4, 9, 10]
    big = [(0, 0), (200, 0), (200, 200), (0, 200)]
    mid = [(0, 0), (50, 0), (50, 50), (0, 50)]
    audit = P.audit_polygons_cells([cell(ob("a", big), ob("a", mid), ob("a", [(0, 0), (1, 0), (1, 1)]))], [500], [500],
                                   backend=BE)
    assert audit.per_class[["small", "medium", "large", "tiny_area"]].values.tolist() == [[1, 1, 1, 1]]


def _random_polygon(rnd):
    n = rnd.randint(3, 12)
    return [(float(rnd.randint(0, 20)), float(rnd.randint(0, 20))) for _ in range(n)]


def test_defect_predicate_is_exact_on_integer_coordinates():
    rnd = random.Random(1)
    hits = 0
    for _ in range(3000):
        V = _random_polygon(rnd)
        if rnd.random() < 0.2:                       # repeated and closing points
            k = rnd.randrange(len(V))
            V.insert(k, V[k])
        Vf = [(Fraction(x), Fraction(y)) for x, y in V]
        assert R.self_intersecting(V) == R.self_intersecting(Vf), V
        assert R.defects(V, V, 1.0) == R.defects(Vf, Vf, 1), V
        hits += R.self_intersecting(V)
    assert 0 < hits < 3000


def test_categories_equal_the_segment_actions():
    cells = [c for c in fuzz_cells(1500, 21, numeric=True) if _plain(c)]
    rnd = random.Random(5)
    labels = [rnd.choice(["a", "a", "猫"]) for _ in cells]
    ws = [rnd.choice([100, 100, 100.5, 80, 0, None, -3, float("nan")]) for _ in cells]
    hs = [rnd.choice([100, 60, 100, 0, float("inf")]) for _ in cells]
    status, W, H = P._audit_sizes(ws, hs, len(cells))
    row_off, xy, pt_off, obj, cls, names, _ = P._poly_chunk(np.asarray(cells, object))
    cat = R.audit_arrays(xy, pt_off, row_off, cls, W, H, status, len(names))[0]
    compared = 0
    for i, c in enumerate(cells):
        _, _, acts = S.seg_row(c, labels[i], 0, ws[i], hs[i])
        mine = [S.ACTIONS[cat[p]] for p in range(row_off[i], row_off[i + 1]) if cls[p] >= 0 and names[cls[p]] == labels[i]]
        if acts:
            assert mine == acts, (i, c)
            compared += len(acts)
    assert compared > 100


@pytest.mark.parametrize("threads", [1, 4])
def test_native_named_polygon_scan_matches_flatten(threads):
    cells = [c for c in fuzz_cells(600, 40 + threads) if _plain(c)]
    scan = nj.scan_named_polygons(cells, n_threads=threads)
    try:
        irregular = 0
        for i, c in enumerate(cells):
            if scan.status[i] == nj.IRREGULAR:
                irregular += 1
                continue
            b0, b1 = int(scan.cell_box_off[i]), int(scan.cell_box_off[i + 1])
            got = [(int(scan.box_object[b]), scan.names[scan.box_class[b]],
                    scan.xy[2 * scan.pt_off[b]:2 * scan.pt_off[b + 1]].reshape(-1, 2).tolist()) for b in range(b0, b1)]
            want = [(k, name, [[float(x), float(y)] for x, y in pts]) for k, name, pts in fl.seg_cell_polygons(c)]
            assert got == want, (i, c)
        assert 0 < irregular < len(cells)
    finally:
        scan.close()


def test_class_ids_do_not_depend_on_the_thread_count():
    cells = [cell(*[ob(nm, [(1, 1), (2, 2), (3, 1)]) for nm in random.Random(k).sample("abcdefgh", 3)]) for k in range(400)]
    ref = None
    for threads in (1, 2, 4, 7):
        scan = nj.scan_named_polygons(cells, n_threads=threads)
        got = (scan.names, scan.box_class.tolist())
        scan.close()
        ref = ref or got
        assert got == ref


def _table(n, seed):
    rnd = random.Random(seed)
    cells = [c for c in fuzz_cells(n, seed, numeric=True) if _plain(c) and "ud800" not in str(c)]   # a lone surrogate name: no CSV
    return pd.DataFrame({"source": [f"s{k}" for k in range(len(cells))], P.ANNOTATION_COL: cells,
                         "width": [rnd.choice([100, 0, 80.5]) for _ in cells], "height": [rnd.choice([100, 60]) for _ in cells]})


def _check_sums(audit):
    pc = audit.per_class
    t = audit.totals
    assert int(pc["polygons"].sum()) + t["unmatchable_name_polygons"] == t["polygons"]
    assert (pc[list(S.ACTIONS)].sum(axis=1) == pc["polygons"]).all()
    assert (pc[["small", "medium", "large"]].sum(axis=1) == pc["written"] + pc["clipped"]).all()
    assert (audit.hist_vertices.sum(axis=1) == pc["polygons"].to_numpy()).all()
    for k in (*S.ACTIONS, *R.DEFECTS):
        assert int(pc[k].sum()) == t[k]
    assert len(audit.problems) == int(pc[["bad_coords", "too_few_points", "empty", "no_size"]].to_numpy().sum()) + \
        int(((audit.problems["category"].isin(["written", "clipped"])).sum()))


def test_frame_and_csv(tmp_path):
    df = _table(700, 3)
    stats = {}
    audit = P.audit_polygons_frame(df, backend=BE, stats=stats)
    _check_sums(audit)
    assert stats == audit.totals and audit.totals["written"] > 0 and audit.totals["self_intersecting"] > 0
    assert audit.classes == sorted(audit.classes) and audit.problems["source"].tolist() == \
        df["source"].to_numpy()[audit.problems["row"].to_numpy()].tolist()
    path = tmp_path / "t.csv"
    df.to_csv(path, index=False, encoding="utf-8-sig")
    res = P.audit_polygons_csv(str(path), tmp_path / "out", backend=BE)
    assert {k: v for k, v in res.items() if k != "paths"} == audit.totals
    got = pd.read_csv(res["paths"]["classes"], encoding="utf-8-sig", keep_default_na=False)
    assert got["polygons"].tolist() == audit.per_class["polygons"].tolist()
    assert got["class"].astype(str).tolist() == [str(c) for c in audit.classes]
    h = np.load(res["paths"]["hist"])
    assert np.array_equal(h["hist_vertices"], audit.hist_vertices) and h["edges"].tolist() == list(R.HIST_EDGES)
    assert len(pd.read_csv(res["paths"]["problems"], encoding="utf-8-sig")) == len(audit.problems)


def test_frame_without_size_columns():
    audit = P.audit_polygons_frame(pd.DataFrame({P.ANNOTATION_COL: [cell(ob("a", [(1, 1), (5, 5)]))]}), backend=BE)
    assert audit.per_class["no_size"].tolist() == [1] and audit.totals["rows_missing"] == 1


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), "1", None, True])
def test_min_area_must_be_finite_and_not_negative(bad, tmp_path):
    with pytest.raises(ValueError):
        P.audit_polygons_cells([cell(ob("a", [(1, 1), (5, 5)]))], [10], [10], min_area=bad, backend=BE)
    with pytest.raises(ValueError):
        P.audit_polygons_csv(str(tmp_path / "none.csv"), tmp_path, min_area=bad, backend=BE)


def test_min_area_moves_the_tiny_bit():
    c = [cell(ob("a", [(0, 0), (4, 0), (4, 4), (0, 4)]))]
    assert P.audit_polygons_cells(c, [10], [10], min_area=16.0, backend=BE).totals["tiny_area"] == 0
    assert P.audit_polygons_cells(c, [10], [10], min_area=16.5, backend=BE).totals["tiny_area"] == 1
    assert P.audit_polygons_cells(c, [10], [10], min_area=0, backend=BE).totals["tiny_area"] == 0


def test_backend_without_the_method():
    with pytest.raises(TypeError, match="audit_polygons"):
        P.audit_polygons_cells([cell(ob("a", [(1, 1), (5, 5)]))], [10], [10], backend=OracleBackend())
