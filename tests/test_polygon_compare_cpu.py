"""Polygon comparison (core/processor.py: compare_polygons_*; flatten.compare_rows / compare_batches), host side, and the K22 rule
itself as restated in tests/polygon_compare_ref.py: cases worked by hand, identities on random tables, the row rule, the three
alignments, batches, the class merge and the files written — driven by a test backend whose device stage is the restatement;
tests/test_gpu_polygon_compare.py checks K22 itself.  No GPU."""
import json
import math

import numpy as np
import pandas as pd
import pytest

import polygon_compare_ref as R
import polygon_raster_ref as RR
from helpers import OracleBackend
from polygon_compare_tables import (RANDOM, assert_same_cover, box, random_rows, random_table, random_want, raster_side, shared_table,
                                    shared_want, table)

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd.core import processor as P

COL = P.ANNOTATION_COL
(STATUS, PAIR_OFF, A_ACT, B_ACT, A_PIX, B_PIX, A_MATCH, B_MATCH, B_IOU, A_BEST, B_BEST, ROWS, CONF, PCONF, ROW_PIX, PAIRS) = range(16)


class CompareBackend(OracleBackend):
    def __init__(self):
        self.calls = []

    def compare_polygons(self, *args):
        out = R.compare_arrays(*args)
        self.calls.append((len(args[8]), int(out[PAIR_OFF][-1])))
        return out[:15]


def one_row(a, b, w=8, h=8, n_classes=2, **kw):
    return R.compare_arrays(*table([(w, h, a, b)]), n_classes, **kw)


# ----------------------------------------------------------------------------------------------- the rule
def test_the_threshold_is_inclusive():
    a, b = [(0, box(0, 0, 1, 1))], [(0, box(0, 0, 2, 1))]                      # 1 and 2 pixels, 1 in common: IoU 1 / 2
    out = one_row(a, b, thr=0.5)
    assert out[PAIRS].tolist() == [1] and out[A_PIX].tolist() == [1] and out[B_PIX].tolist() == [2]
    assert out[B_MATCH].tolist() == [0] and out[B_IOU].tolist() == [0.5] and out[ROWS].tolist() == [[1, 0, 0, 0]]
    out = one_row(a, b, thr=np.nextafter(0.5, 1))
    assert out[B_MATCH].tolist() == [-1] and out[B_IOU].tolist() == [0.0] and out[B_BEST].tolist() == [0.5] and out[ROWS].tolist() == [[0, 0, 1, 1]]
    out = one_row([(0, box(0, 0, 3, 3))], [(0, box(1, 1, 4, 4))], thr=4 / 14)   # two squares a unit apart: 4 of 14 pixels
    assert out[PAIRS].tolist() == [4] and out[B_IOU].tolist() == [4 / 14]


def test_a_tie_goes_to_the_lowest_index():
    sq = box(1, 1, 5, 5)
    out = one_row([(0, box(6, 6, 8, 8)), (0, sq), (0, sq)], [(0, sq), (0, sq)])
    assert out[B_MATCH].tolist() == [1, 2] and out[A_MATCH].tolist() == [-1, 0, 1] and out[B_IOU].tolist() == [1.0, 1.0]


def test_an_earlier_polygon_takes_the_partner_a_later_one_scores_higher_with():
    out = one_row([(0, box(0, 0, 4, 4))], [(0, box(0, 0, 4, 3)), (0, box(0, 0, 4, 4))])
    assert out[B_MATCH].tolist() == [0, -1] and out[B_IOU].tolist() == [0.75, 0.0] and out[B_BEST].tolist() == [0.75, 1.0]
    assert out[A_BEST].tolist() == [1.0] and out[ROWS].tolist() == [[1, 0, 0, 1]] and out[CONF].tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 0]]


def test_by_label_gives_no_relabelled_pair():
    a, b = [(0, box(0, 0, 4, 4)), (1, box(4, 4, 8, 8))], [(1, box(0, 0, 4, 4)), (1, box(4, 4, 8, 7))]
    out = one_row(a, b)
    assert out[ROWS].tolist() == [[1, 1, 0, 0]] and out[CONF].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]]
    out = one_row(a, b, by_label=True)
    assert out[ROWS].tolist() == [[1, 0, 1, 1]] and out[B_MATCH].tolist() == [-1, 1] and out[B_BEST].tolist() == [1.0, 0.75]
    assert out[PCONF].tolist() == [[0, 16, 0], [0, 12, 4], [0, 0, 32]]


@pytest.mark.parametrize("thr", [0.0, -1.0, math.nan])
def test_a_threshold_of_nothing(thr):
    a, b = [(0, box(0, 0, 3, 3)), (0, box(5, 5, 8, 8))], [(0, box(4, 0, 7, 3)), (0, box(5, 5, 8, 8))]
    out = one_row(a, b, thr=thr)
    if math.isnan(thr):                                                         # NaN matches nothing
        assert out[B_MATCH].tolist() == [-1, -1] and out[ROWS].tolist() == [[0, 0, 2, 2]]
    else:                                                                       # disjoint polygons never match
        assert out[B_MATCH].tolist() == [-1, 1] and out[A_MATCH].tolist() == [-1, 1] and out[ROWS].tolist() == [[1, 0, 1, 1]]
    assert not np.isnan(out[B_IOU]).any() and out[B_BEST].tolist() == [0.0, 1.0]


def test_a_polygon_without_a_pixel_centre_is_never_matched():
    speck = box(0.6, 0.6, 1.4, 1.4)
    out = one_row([(0, speck)], [(0, speck)], thr=0.0)
    assert out[A_ACT].tolist() == [0] and out[A_PIX].tolist() == [0] and out[PAIRS].tolist() == [0]
    assert out[B_MATCH].tolist() == [-1] and out[ROWS].tolist() == [[0, 0, 1, 1]] and out[CONF].tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]
    assert out[PCONF].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 64]]


def test_polygons_that_are_not_compared_count_nowhere():
    sq = box(0, 0, 4, 4)
    odd = [(0, [(1.0, 1.0), (math.nan, 2.0), (3.0, 3.0)]), (0, [(2.0, 2.0)]), (-1, sq)]
    out = R.compare_arrays(*table([(8, 8, odd + [(1, sq)], [(1, sq)] + odd), (0, 8, [(0, sq)], [(0, sq)])]), 2)
    assert out[A_ACT].tolist() == [2, 3, 255, 0, 5] and out[B_ACT].tolist() == [0, 2, 3, 255, 5]
    assert out[ROWS].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0]] and out[CONF].sum() == 1 and out[CONF][1, 1] == 1
    assert out[A_MATCH].tolist() == [-1, -1, -1, 0, -1] and out[B_MATCH].tolist() == [3, -1, -1, -1, -1]
    assert out[PCONF].sum() == 64 and out[PCONF][1, 1] == 16 and out[STATUS].tolist() == [0, 1] and out[PAIR_OFF].tolist() == [0, 16, 16]
    assert out[PAIRS].sum() == 16 and out[PAIRS][3 * 4 + 0] == 16


def test_the_row_rule():
    sq = [(0, box(0, 0, 2, 2))]
    rows = [(4, 4, sq * 2, sq * 3), (4, 4, sq * 2, sq * 4), (0, 4, sq, sq), (4.5, 4, sq, sq), (9, 9, sq * 9, sq * 9), (4, 4, [], sq)]
    t = table(rows)
    out = R.compare_arrays(*t, 1, max_pixels_per_row=16, max_pairs_per_row=6)
    assert out[STATUS].tolist() == [0, 4, 1, 2, 3, 0] and out[PAIR_OFF].tolist() == [0, 6, 6, 6, 6, 6, 6]
    status, pixels, pairs = fl.compare_rows(t[8], t[9], np.diff(t[2]), np.diff(t[6]), 16, 6)
    assert status.tolist() == out[STATUS].tolist() and pixels.tolist() == [16, 0, 0, 0, 0, 16] and pairs.tolist() == [6, 0, 0, 0, 0, 0]
    assert fl.compare_batches([5, 5, 5, 50, 5], [1, 1, 9, 1, 1], 12, 9) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert fl.compare_batches([], [], 1, 1) == [] and fl.compare_batches([9], [9], 1, 1) == [(0, 1)]


# ----------------------------------------------------------------------------------------------- identities
def test_pixel_confusion_against_the_raster_step():
    t, want = random_table(), random_want()
    W, H = t[8], t[9]
    compared = want[STATUS] == 0
    assert want[PCONF].sum() == int((W[compared] * H[compared]).sum())
    assert want[ROW_PIX][~compared].sum() == 0 and (want[ROW_PIX][:, 0] <= want[ROW_PIX][:, 1]).all()
    for side, axis in ((0, 1), (1, 0)):
        xy, pt_off, row_off, cls = t[4 * side:4 * side + 4]
        row = np.repeat(np.arange(len(W)), np.diff(row_off))
        val = np.where(compared[row], cls, -1)                                  # K21 paints rows that K22 does not compare
        owned = RR.raster_arrays(xy, pt_off, row_off, val, W, H, 255, RANDOM["max_pixels_per_row"])[4]
        per_class = np.bincount(cls[val >= 0], weights=owned[val >= 0], minlength=3).astype(np.int64)
        assert want[PCONF].sum(axis=axis)[:3].tolist() == per_class.tolist() and per_class.min() > 0
    fg = want[PCONF].sum() - want[PCONF][3, 3]
    assert want[ROW_PIX][:, 1].sum() == fg and want[ROW_PIX][:, 0].sum() == np.trace(want[PCONF][:3, :3])


@pytest.mark.parametrize("which", ["shared", "random"])
def test_the_two_restatements_agree_on_the_cover(which):
    """what tests/test_gpu_polygon_compare.py asserts between K21's and K22's outputs holds between the restatements, which take
    their pixels from one cover(): the GPU test's expectation does not rest on the code under test"""
    assert R.cover is RR.cover
    if which == "shared":
        t, (mask_a, mask_b, out) = shared_table(), shared_want()
    else:
        t, out = random_table(), random_want()
        mask_a, mask_b = (RR.raster_arrays(*raster_side(t, side), 0, RANDOM["max_pixels_per_row"]) for side in (0, 1))
    assert_same_cover(t, mask_a, mask_b, out)
    assert (out[STATUS] == 0).sum() >= 6 and (out[ROW_PIX][:, 0] > 0).sum() >= 6 and {0, 255} <= set(out[A_ACT].tolist())
    if which == "shared":                                                       # the table holds what its docstring says
        n_pts = np.concatenate([np.diff(t[1]), np.diff(t[5])])
        assert out[STATUS].tolist() == [0, 0, 0, 0, 0, 2, 0] and (n_pts == 2).sum() >= 2 and (n_pts == 65).sum() == 2
        assert 5 in out[A_ACT].tolist() and 255 in out[B_ACT].tolist() and out[A_PIX][12] > 300 and out[B_PIX][out[B_ACT] == 0].min() > 0
    else:
        assert (out[STATUS] == R.STATUS_PAIRS).any()


def test_a_table_against_itself_and_swapped():
    t = random_table()
    a = t[:4]
    out = R.compare_arrays(*a, *a, t[8], t[9], **RANDOM)
    live = (out[B_ACT] == 0) & (out[B_PIX] > 0)
    assert live.sum() > 50 and (out[B_IOU][live] == 1.0).all() and (out[B_MATCH][live] >= 0).all()
    assert (out[B_MATCH][~live] == -1).all() and out[PCONF].sum() == np.trace(out[PCONF]) and out[ROWS][:, 1].sum() == 0
    want = random_want()
    swapped = R.compare_arrays(*t[4:8], *t[:4], t[8], t[9], **RANDOM)
    assert np.array_equal(swapped[PCONF], want[PCONF].T) and np.array_equal(swapped[A_PIX], want[B_PIX])
    assert np.array_equal(swapped[ROW_PIX], want[ROW_PIX]) and swapped[PAIRS].sum() == want[PAIRS].sum()


# ----------------------------------------------------------------------------------------------- the host layer
def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


NAMES = ["cat", "dog", "emu"]


def cells_of(rows, k):
    return [cell(*[ob(NAMES[c] if c >= 0 else 7, pts) for c, pts in row[k] if all(map(math.isfinite, sum(pts, ())))]) for row in rows]


def frames(n_rows=24, seed=9):
    rows = random_rows(seed, n_rows=n_rows, max_polys=5, max_size=40)
    src = [f"im{k}.jpg" for k in range(n_rows)]
    sizes = {"width": [r[0] for r in rows], "height": [r[1] for r in rows]}
    return (pd.DataFrame({"source": src, COL: cells_of(rows, 2), **sizes}), pd.DataFrame({"source": src, COL: cells_of(rows, 3), **sizes}))


def same_comparison(x, y):
    assert x.classes == y.classes
    assert {k: v for k, v in x.totals.items() if v == v} == {k: v for k, v in y.totals.items() if v == v}   # a NaN equals nothing
    assert [k for k, v in x.totals.items() if v != v] == [k for k, v in y.totals.items() if v != v]
    for name in ("confusion", "pixel_confusion", "per_class", "per_row", "differences", "unpaired"):
        pd.testing.assert_frame_equal(getattr(x, name), getattr(y, name), obj=name)
    assert np.array_equal(x.hist_iou, y.hist_iou)


def test_cells_against_the_restatement():
    sq, other = [(1.0, 1.0), (5.0, 5.0)], [(1.0, 1.0), (5.0, 4.0)]
    a = [cell(ob("cat", sq), ob("dog", [(6.0, 6.0), (8.0, 8.0)]), ob("cat", [(0.0, 6.0)])), cell(ob("cat", sq)), cell()]
    b = [cell(ob("dog", other), ob("emu", [(0.0, 0.0), (1.0, 1.0)])), cell(ob("cat", sq)), cell(ob("cat", sq))]
    stats = {}
    res = P.compare_polygons_cells(a, b, [8, 8, 8.5], [8, 8, 8], backend=CompareBackend(), stats=stats, sources=["x", "y", "z"])
    assert res.classes == ["cat", "dog", "emu"] and stats == res.totals
    assert res.confusion.loc["cat", "dog"] == 1 and res.confusion.loc["cat", "cat"] == 1 and res.confusion.loc["dog", P.COMPARE_NONE] == 1
    assert res.confusion.loc[P.COMPARE_NONE, "emu"] == 1 and res.confusion.to_numpy().sum() == 4
    assert res.pixel_confusion.loc["cat", "dog"] == 12 and res.pixel_confusion.loc["cat", P.COMPARE_BACKGROUND] == 4
    assert res.pixel_confusion.to_numpy().sum() == 128 == res.totals["pixels"]
    assert res.per_row["status"].tolist() == ["compared", "compared", "fractional_size"] and res.per_row["source"].tolist() == ["x", "y", "z"]
    assert res.per_row[["agree", "relabelled", "missing", "extra"]].values.tolist() == [[0, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0]]
    assert res.per_row["pixels_agree_fg"].tolist() == [0, 16, 0] and res.per_row["pixels_fg"].tolist() == [21, 16, 0]
    assert res.per_row["fg_iou"].tolist()[:2] == [0.0, 1.0] and math.isnan(res.per_row["fg_iou"][2])
    d = res.differences
    assert d["kind"].tolist() == ["missing", "extra", "relabelled"] and d["a_object"].tolist() == [1, -1, 0] and d["b_object"].tolist() == [-1, 1, 0]
    assert d["a_name"].tolist() == ["dog", None, "cat"] and d["b_name"].tolist() == [None, "emu", "dog"] and d["iou"].tolist() == [0.0, 0.0, 0.75]
    assert d["a_pixels"].tolist() == [4, -1, 16] and d["b_pixels"].tolist() == [-1, 1, 12] and d["source"].tolist() == ["x"] * 3
    pc = res.per_class.set_index("class")
    assert pc.loc["cat", ["a_polygons", "b_polygons", "agree", "relabelled_to_other", "missing", "a_skipped", "b_skipped"]].tolist() == [2, 1, 1, 1, 0, 1, 0]
    assert pc.loc["cat", ["a_pixels", "b_pixels", "pixels_both"]].tolist() == [32, 16, 16] and pc.loc["cat", "pixel_iou"] == 0.5
    assert res.hist_iou[0].tolist() == [0] * 19 + [1] and res.hist_iou.sum() == 1
    t = res.totals
    assert (t["rows"], t["a_polygons"], t["b_polygons"], t["matched"], t["agree"], t["relabelled"], t["missing"], t["extra"]) == (3, 4, 4, 2, 1, 1, 1, 1)
    assert (t["rows_compared"], t["rows_fractional_size"], t["rows_no_size"], t["a_skipped"], t["python_cells"]) == (2, 1, 0, 1, 0)
    assert t["pixel_accuracy"] == (16 + 91) / 128 and t["mean_pixel_iou"] == (0.5 + 0.0 + 0.0) / 3


def test_batches_give_the_result_of_one_batch():
    df_a, df_b = frames()
    kw = dict(max_pixels_per_row=40 * 40, max_pairs_per_row=20, iou_threshold=0.4)
    one, be = CompareBackend(), CompareBackend()
    want = P.compare_polygons_frame(df_a, df_b, backend=one, **kw)
    assert len(one.calls) == 1 and want.totals["agree"] > 5 and want.totals["pixels"] > 5000
    assert {"compared", "no_size", "fractional_size", "too_many_pairs"} <= set(want.per_row["status"])
    got = P.compare_polygons_frame(df_a, df_b, backend=be, batch_pixels=1500, **kw)
    assert len(be.calls) > 3
    same_comparison(got, want)
    be = CompareBackend()
    got = P.compare_polygons_frame(df_a, df_b, backend=be, batch_pairs=25, **kw)
    assert len(be.calls) > 3 and max(p for _, p in be.calls) <= 25
    same_comparison(got, want)


def test_the_three_alignments():
    df_a, df_b = frames()
    be = CompareBackend()
    kw = dict(backend=be, max_pairs_per_row=20)
    want = P.compare_polygons_frame(df_a, df_b, key=None, **kw)
    assert want.totals["rows_only_a"] == 0 and want.totals["rows_size_mismatch"] == 0
    both = df_a.assign(other=df_b[COL])
    same_comparison(P.compare_polygons_frame(both, other_col="other", **kw), want)
    shuffled = df_b.iloc[::-1].reset_index(drop=True)
    same_comparison(P.compare_polygons_frame(df_a, shuffled, **kw), want)
    # rows on one side only, and rows whose sizes differ
    part_b = shuffled.iloc[3:].reset_index(drop=True).copy()
    extra_row = part_b.iloc[:1].assign(source="new.jpg")
    part_b = pd.concat([part_b, extra_row], ignore_index=True)
    ok = np.flatnonzero(want.per_row["status"].to_numpy() == "compared")
    hit = df_a["source"][ok[ok >= 5][0]]                                        # a row that stays on both sides
    part_b.loc[part_b["source"] == hit, "width"] += 1
    stats = {}
    res = P.compare_polygons_frame(df_a.iloc[2:].reset_index(drop=True), part_b, stats=stats, **kw)
    assert res.unpaired.values.tolist() == [["im21.jpg", "a"], ["im22.jpg", "a"], ["im23.jpg", "a"], ["im1.jpg", "b"], ["im0.jpg", "b"],
                                            ["new.jpg", "b"]]
    assert res.totals["rows_only_a"] == 3 and res.totals["rows_only_b"] == 3 and res.totals["rows"] == 19 and stats == res.totals
    row = res.per_row.set_index("source")
    assert row.loc[hit, "status"] == "size_mismatch" and res.totals["rows_size_mismatch"] == 1 and row.loc[hit, "agree"] == 0
    assert res.per_row["row"].tolist() == list(range(19)) and not (res.differences["source"] == hit).any()
    others = res.per_row[res.per_row["source"] != hit].drop(columns="row").reset_index(drop=True)
    full = want.per_row[want.per_row["source"].isin(others["source"])].drop(columns="row").reset_index(drop=True)
    pd.testing.assert_frame_equal(others, full)
    no_size = P.compare_polygons_frame(df_a, part_b.drop(columns=["width", "height"]), **kw)       # B without sizes: nothing to differ
    assert no_size.totals["rows_size_mismatch"] == 0
    with pytest.raises(ValueError, match="by position"):
        P.compare_polygons_frame(df_a, df_b.iloc[:3], key=None, **kw)
    with pytest.raises(ValueError, match="more than once"):
        P.compare_polygons_frame(df_a, pd.concat([df_b, df_b.iloc[:1]]), **kw)
    with pytest.raises(ValueError, match="other_col"):
        P.compare_polygons_frame(df_a, **kw)


def test_names_that_are_no_str_share_the_last_class():
    sq = [(0.0, 0.0), (4.0, 4.0)]
    a = [cell(ob(7, sq), ob("b", [(4.0, 4.0), (8.0, 8.0)]))]
    b = [cell(ob(2, sq), ob(3.5, [(4.0, 4.0), (8.0, 8.0)]))]
    res = P.compare_polygons_cells(a, b, [8], [8], backend=CompareBackend())
    assert res.classes == ["b", None] and res.confusion.index.tolist() == ["b", None, P.COMPARE_NONE]
    assert res.confusion.to_numpy().tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]]
    assert res.pixel_confusion.to_numpy().tolist() == [[0, 16, 0], [0, 16, 0], [0, 0, 32]]
    assert res.differences["a_name"].tolist() == ["b"] and res.differences["b_name"].tolist() == [None]
    empty = P.compare_polygons_cells([cell()], [cell()], [4], [4], backend=CompareBackend())          # no polygon at all
    assert empty.classes == [] and empty.pixel_confusion.to_numpy().tolist() == [[16]] and empty.totals["pixel_accuracy"] == 1.0
    assert math.isnan(empty.totals["mean_pixel_iou"]) and len(empty.per_class) == 0


def test_csv_twin(tmp_path, capsys):
    df_a, df_b = frames()
    pa, pb = tmp_path / "a.csv", tmp_path / "b.csv"
    df_a.to_csv(pa, index=False, encoding="utf-8-sig")
    df_b.iloc[::-1].to_csv(pb, index=False, encoding="utf-8-sig")
    be = CompareBackend()
    kw = dict(backend=be, max_pairs_per_row=20, iou_threshold=0.4)
    res = P.compare_polygons_csv(pa, pb, tmp_path / "out", **kw)
    want = P.compare_polygons_frame(pd.read_csv(pa, encoding="utf-8-sig"), pd.read_csv(pb, encoding="utf-8-sig"), **kw)
    assert {k: v for k, v in res.items() if k != "paths" and v == v} == {k: v for k, v in want.totals.items() if v == v}
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == [
        "polygon_compare_classes.csv", "polygon_compare_confusion.csv", "polygon_compare_differences.csv", "polygon_compare_hist.npz",
        "polygon_compare_pixels.csv", "polygon_compare_rows.csv"]
    read = lambda k, **o: pd.read_csv(res["paths"][k], encoding="utf-8-sig", **o)   # noqa: E731
    for key, frame in (("confusion", want.confusion), ("pixels", want.pixel_confusion)):
        got = read(key, index_col="a_class")
        assert got.to_numpy().tolist() == frame.to_numpy().tolist()
        assert [c for c in got.columns if not c.startswith("Unnamed")] == [c for c in frame.columns if c is not None]   # None: an empty header
    got = read("classes")
    pd.testing.assert_frame_equal(got.drop(columns="class"), want.per_class.drop(columns="class"), check_dtype=False)
    assert got["class"].fillna("").tolist() == [c or "" for c in want.classes]        # None: an empty field
    pd.testing.assert_frame_equal(read("rows"), want.per_row, check_dtype=False)
    got, names = read("differences"), ["a_name", "b_name"]
    pd.testing.assert_frame_equal(got.drop(columns=names), want.differences.drop(columns=names), check_dtype=False)
    assert len(got) > 5 and {"missing", "extra", "relabelled"} <= set(got["kind"])
    for c in names:
        assert got[c].fillna("").tolist() == [v or "" for v in want.differences[c]]
    hist = np.load(res["paths"]["hist"])
    assert hist["classes"].tolist() == [P.COMPARE_NONE if c is None else c for c in want.classes] and np.array_equal(hist["hist_iou"], want.hist_iou) and want.hist_iou.sum() > 5
    by_pos = P.compare_polygons_csv(pa, pa, tmp_path / "q", key=None, **kw)
    assert by_pos["relabelled"] == 0 and by_pos["missing"] == by_pos["extra"] < 8 and by_pos["agree"] > 10    # polygons without a pixel
    assert by_pos["pixel_accuracy"] == 1.0 and by_pos["rows_only_a"] == 0
    capsys.readouterr()
    assert P.compare_polygons_csv(tmp_path / "nope.csv", pa, tmp_path / "o", **kw) is None
    assert "读取失败" in capsys.readouterr().out
    df_a.drop(columns=[COL]).to_csv(tmp_path / "bad.csv", index=False, encoding="utf-8-sig")
    assert P.compare_polygons_csv(pa, tmp_path / "bad.csv", tmp_path / "o", **kw) is None
    assert "缺少必要列" in capsys.readouterr().out
    df_a.drop(columns=["source"]).to_csv(tmp_path / "nokey.csv", index=False, encoding="utf-8-sig")
    assert P.compare_polygons_csv(pa, tmp_path / "nokey.csv", tmp_path / "o", **kw) is None
    assert "缺少必要列 source" in capsys.readouterr().out


def test_arguments():
    c = [cell(ob("a", [(0.0, 0.0), (2.0, 2.0)]))]
    be = CompareBackend()
    with pytest.raises(TypeError, match="compare_polygons"):
        P.compare_polygons_cells(c, c, [4], [4], backend=OracleBackend())
    with pytest.raises(ValueError, match="one cell per image"):
        P.compare_polygons_cells(c, c + c, [4], [4], backend=be)
    for bad in (dict(iou_threshold="0.5"), dict(iou_threshold=True), dict(max_pixels_per_row=0), dict(max_pixels_per_row=2 ** 30 + 1),
                dict(max_pairs_per_row=0), dict(max_pairs_per_row=2 ** 24 + 1), dict(max_pairs_per_row=2.0), dict(batch_pixels=0),
                dict(batch_pairs=0)):
        with pytest.raises(ValueError):
            P.compare_polygons_cells(c, c, [4], [4], backend=be, **bad)
    with pytest.raises(ValueError, match="widths and heights"):
        P.compare_polygons_cells(c, c, [4, 4], [4], backend=be)


def test_a_device_that_disagrees_with_the_host_is_an_error():
    class Off(CompareBackend):
        def compare_polygons(self, *a):
            out = list(super().compare_polygons(*a))
            out[0] = np.where(out[0] == 0, 3, out[0]).astype(np.uint8)
            return out

    c = [cell(ob("a", [(0.0, 0.0), (2.0, 2.0)]))]
    with pytest.raises(RuntimeError, match="differ from the host"):
        P.compare_polygons_cells(c, c, [4], [4], backend=Off())
