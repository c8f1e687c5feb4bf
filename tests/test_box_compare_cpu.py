"""Box comparison (core/processor.py: compare_boxes_*), host side: the two restatements of K18 against each other, spelled-out
known answers, frame / key handling, chunking and the CSV routes — driven by a test backend whose device stage is the numpy
restatement of tests/box_compare_ref.py.  No GPU."""
import json

import numpy as np
import pandas as pd
import pytest

from box_compare_ref import check_comparison, compare_rows, compare_rows_py, expected_comparison, same_outputs
from helpers import OracleBackend

from deal_yolo_daya_amd.core import processor as P

COL = P.BBOX_COL


class CompareBackend(OracleBackend):
    def compare_boxes(self, a_box4, a_row_off, a_cls, b_box4, b_row_off, b_cls, n_classes, thr, by_label=False):
        return compare_rows(a_box4, a_row_off, a_cls, b_box4, b_row_off, b_cls, n_classes, thr, by_label)


BE = CompareBackend()


def ob(name, x1, y1, x2, y2, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x1, "y": y1}, {"x": x2, "y": y2}]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def compare(cells_a, cells_b, thr=0.5, by_label=False, **kw):
    res = P.compare_boxes_cells(cells_a, cells_b, thr, by_label, backend=BE, **kw)
    check_comparison(res, expected_comparison(cells_a, cells_b, thr, by_label, kw.get("sources")))
    return res


def kinds(res):
    return res.differences["kind"].tolist()


# ----------------------------------------------------------------------------------------------- the two restatements
def random_tables(rng, n_rows, max_boxes=7, n_classes=3):
    na, nb = rng.integers(0, max_boxes + 1, n_rows), rng.integers(0, max_boxes + 1, n_rows)
    a_off, b_off = np.zeros(n_rows + 1, np.int64), np.zeros(n_rows + 1, np.int64)
    np.cumsum(na, out=a_off[1:])
    np.cumsum(nb, out=b_off[1:])
    c = rng.integers(0, 12, (a_off[-1], 2)).astype(np.float64)
    a = np.concatenate([c, c + rng.integers(0, 8, (a_off[-1], 2))], axis=1)
    b = np.zeros((b_off[-1], 4))
    for r in range(n_rows):
        for j in range(b_off[r], b_off[r + 1]):
            if na[r] and rng.random() < 0.7:               # a copy of an A box of the row, sometimes moved a little
                b[j] = a[rng.integers(a_off[r], a_off[r + 1])]
                if rng.random() < 0.5:
                    b[j] += rng.integers(-1, 2, 4)
            else:
                p = rng.integers(0, 12, 2)
                b[j] = (*p, *(p + rng.integers(0, 8, 2)))
    for t in (a, b):
        swap = rng.random(len(t)) < 0.3
        t[swap] = t[swap][:, [2, 3, 0, 1]]
        for k in np.flatnonzero(rng.random(len(t)) < 0.06):
            t[k, rng.integers(0, 4)] = [np.nan, np.inf, -np.inf, -0.0][rng.integers(0, 4)]
    return (a, a_off, rng.integers(0, n_classes, len(a)), b, b_off, rng.integers(0, n_classes, len(b)), n_classes)


@pytest.mark.parametrize("thr", [0.5, 0.98, 0.0, -1.0, 1.0, float("nan")])
@pytest.mark.parametrize("by_label", [False, True])
def test_scalar_and_vectorised_restatements_agree(thr, by_label):
    args = random_tables(np.random.default_rng(18), 300)
    same_outputs(compare_rows(*args, thr, by_label), compare_rows_py(*args, thr, by_label), f"thr={thr}")


def test_restatement_on_a_hand_worked_row():
    # A: two boxes; B: a twin of A1, a box near A0 (IoU 0.81), a far box
    a = [[0, 0, 10, 10], [20, 20, 30, 30]]
    b = [[20, 20, 30, 30], [0, 0, 9, 9], [50, 50, 60, 60]]
    am, bm, bi, ab, bb, rows, conf = compare_rows(a, [0, 2], [0, 1], b, [0, 3], [1, 1, 0], 2, 0.5, False)
    assert am.tolist() == [1, 0] and bm.tolist() == [1, 0, -1]
    assert bi.tolist() == [1.0, 81 / 100, 0.0] and ab.tolist() == [81 / 100, 1.0] and bb.tolist() == [1.0, 81 / 100, 0.0]
    assert rows.tolist() == [[1, 1, 0, 1]]
    assert conf.tolist() == [[0, 1, 0], [0, 1, 0], [1, 0, 0]]


# ----------------------------------------------------------------------------------------------- known answers
def test_exact_twin_pair():
    c = cell(ob("a", 0, 0, 10, 10), ob("b", 20, 20, 40, 40))
    res = compare([c], [c])
    assert len(res.differences) == 0
    assert res.totals["agree"] == 2 and res.totals["matched"] == 2 and res.totals["missing"] == res.totals["extra"] == 0
    assert res.confusion.loc["a", "a"] == 1 and res.confusion.loc["b", "b"] == 1 and res.confusion.to_numpy().sum() == 2
    assert res.hist_iou[:, -1].tolist() == [1, 1] and res.hist_iou.sum() == 2
    assert res.per_row[["a_boxes", "b_boxes", "agree", "relabelled", "missing", "extra"]].values.tolist() == [[2, 2, 2, 0, 0, 0]]


def test_two_b_boxes_compete_for_one_a_box_and_order_decides():
    a = cell(ob("a", 0, 0, 10, 10))
    near, twin = ob("a", 0, 0, 10, 9), ob("a", 0, 0, 10, 10)
    res = compare([a], [cell(near, twin)])                   # the earlier B box takes it, although the later one fits better
    assert kinds(res) == ["extra"] and res.differences["b_object"].tolist() == [1]
    assert res.differences["best_iou"].tolist() == [1.0] and res.differences["iou"].tolist() == [0.0]
    assert res.hist_iou[0, 18] == 1                          # IoU 0.9
    res = compare([a], [cell(twin, near)])
    assert kinds(res) == ["extra"] and res.differences["b_object"].tolist() == [1]
    assert res.differences["best_iou"].tolist() == [0.9] and res.hist_iou[0, 19] == 1


def test_a_tie_goes_to_the_lowest_a_index():
    a = cell(ob("a", 0, 0, 10, 10), ob("a", 0, 0, 10, 10), ob("a", 0, 0, 10, 10))
    res = compare([a], [cell(ob("a", 0, 0, 10, 10))])
    assert kinds(res) == ["missing", "missing"] and res.differences["a_object"].tolist() == [1, 2]
    assert res.differences["best_iou"].tolist() == [1.0, 1.0]
    # the A box that fits better wins over the lower index
    res = compare([cell(ob("a", 0, 0, 10, 8), ob("a", 0, 0, 10, 10))], [cell(ob("a", 0, 0, 10, 10))])
    assert res.differences["a_object"].tolist() == [0]


def test_the_same_box_under_another_name():
    a, b = cell(ob("cat", 0, 0, 10, 10)), cell(ob("dog", 0, 0, 10, 10))
    res = compare([a], [b], by_label=False)
    assert kinds(res) == ["relabelled"]
    d = res.differences.iloc[0]
    assert (d["a_name"], d["b_name"], d["iou"], d["best_iou"], d["a_object"], d["b_object"]) == ("cat", "dog", 1.0, 1.0, 0, 0)
    assert res.confusion.loc["cat", "dog"] == 1 and res.totals["relabelled"] == 1
    pc = res.per_class.set_index("class")
    assert pc.loc["cat", "relabelled_to_other"] == 1 and pc.loc["dog", "relabelled_from_other"] == 1
    assert res.hist_iou.sum() == 0
    res = compare([a], [b], by_label=True)
    assert kinds(res) == ["missing", "extra"] and res.differences["best_iou"].tolist() == [1.0, 1.0]
    assert res.differences["iou"].tolist() == [0.0, 0.0]
    assert res.confusion.loc["cat", P.COMPARE_NONE] == 1 and res.confusion.loc[P.COMPARE_NONE, "dog"] == 1
    assert res.totals["relabelled"] == 0 and res.totals["by_label"] is True


def test_zero_area_box_at_half_and_at_zero_threshold():
    c = cell(ob("a", 5, 5, 5, 9))
    res = compare([c], [c], thr=0.5)
    assert kinds(res) == ["missing", "extra"] and res.differences["best_iou"].tolist() == [0.0, 0.0]
    res = compare([c], [c], thr=0.0)                          # an empty intersection gives IoU 0.0 >= 0.0
    assert len(res.differences) == 0 and res.totals["agree"] == 1 and res.hist_iou[0, 0] == 1
    res = compare([c], [c], thr=float("nan"))
    assert kinds(res) == ["missing", "extra"]


def test_nan_and_string_coordinates():
    good = ob("a", 0, 0, 10, 10)
    nan_cell = cell(good, ob("a", 7, 2, 3, 4)).replace('"x": 7', '"x": NaN')
    res = compare([nan_cell], [cell(good, ob("a", 7, 2, 3, 4))])
    assert kinds(res) == ["missing", "extra"] and res.differences["a_object"].tolist() == [1, -1]
    assert np.isnan(res.differences["ax1"].iloc[0]) and np.isnan(res.differences["ax2"].iloc[0])
    text = cell(good, ob("a", "1", "2", "3", "4"))            # min / max of strings work; float() is never applied: NaN corners
    res = compare([text], [text])
    assert res.totals["agree"] == 1 and kinds(res) == ["missing", "extra"] and res.totals["python_cells"] == 2
    assert np.isnan(res.differences[["ax1", "ay1", "ax2", "ay2"]].iloc[0].to_numpy(float)).all()


def test_non_str_names_share_one_class_listed_last():
    a = cell(ob(3, 0, 0, 10, 10), ob("z", 20, 20, 30, 30), ob(True, 40, 40, 50, 50))
    b = cell(ob(["x"], 0, 0, 10, 10), ob("z", 20, 20, 30, 30), ob("z", 40, 40, 50, 50))
    res = compare([a], [b])
    assert res.classes == ["z", None] and list(res.confusion.index) == ["z", None, P.COMPARE_NONE]
    assert res.totals["agree"] == 2 and kinds(res) == ["relabelled"]
    d = res.differences.iloc[0]
    assert d["a_name"] is True and d["b_name"] == "z" and d["a_object"] == 2
    assert res.confusion.to_numpy().tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 0]]


def test_empty_cell_on_either_side():
    c = cell(ob("a", 0, 0, 10, 10), ob("b", 0, 0, 5, 5))
    for empty in (None, "", '{"objects": []}', float("nan"), "[1"):
        res = compare([c, empty], [empty, c])
        assert kinds(res) == ["missing", "missing", "extra", "extra"]
        assert res.differences["row"].tolist() == [0, 0, 1, 1] and res.differences["best_iou"].tolist() == [0.0] * 4
        assert res.per_row[["missing", "extra"]].values.tolist() == [[2, 0], [0, 2]]
    res = compare([None], [None])
    assert res.classes == [] and res.confusion.shape == (1, 1) and res.totals["a_boxes"] == 0
    res = compare([], [])
    assert res.totals["rows"] == 0 and len(res.per_row) == 0 and len(res.differences) == 0


def test_differences_are_ordered_by_row_kind_object():
    a = cell(ob("a", 0, 0, 10, 10), ob("a", 100, 100, 110, 110), ob("b", 200, 200, 210, 210), ob("a", 300, 300, 310, 310))
    b = cell(ob("c", 200, 200, 210, 210), ob("a", 400, 400, 410, 410), ob("a", 0, 0, 10, 10), ob("b", 500, 500, 510, 510))
    res = compare([a, a], [b, b], sources=["s0", "s1"])
    assert kinds(res) == ["missing", "missing", "extra", "extra", "relabelled"] * 2
    assert res.differences["a_object"].tolist()[:5] == [1, 3, -1, -1, 2]
    assert res.differences["b_object"].tolist()[:5] == [-1, -1, 1, 3, 0]
    assert res.differences["source"].tolist() == ["s0"] * 5 + ["s1"] * 5 and res.per_row["source"].tolist() == ["s0", "s1"]


def test_arguments():
    c = cell(ob("a", 0, 0, 1, 1))
    with pytest.raises(ValueError, match="one cell per image"):
        P.compare_boxes_cells([c], [c, c], backend=BE)
    with pytest.raises(ValueError, match="iou_threshold"):
        P.compare_boxes_cells([c], [c], "0.5", backend=BE)
    with pytest.raises(TypeError, match="compare_boxes"):
        P.compare_boxes_cells([c], [c], backend=OracleBackend())


# ----------------------------------------------------------------------------------------------- frames and keys
def frames():
    a = [cell(ob("a", 0, 0, 10, 10)), cell(ob("b", 0, 0, 10, 10), ob("a", 50, 50, 60, 60)), cell(ob("c", 1, 1, 5, 5)), None]
    b = [cell(ob("a", 50, 50, 60, 60)), cell(ob("a", 0, 0, 10, 10)), cell(ob("x", 1, 1, 2, 2)), cell(ob("c", 1, 1, 5, 5))]
    df_a = pd.DataFrame({"source": ["u0", "u1", "u2", "u3"], COL: pd.Series(a, dtype=object)})
    df_b = pd.DataFrame({"source": ["u1", "u0", "u9", "u2"], COL: pd.Series(b, dtype=object)})
    return df_a, df_b


def test_frame_aligned_on_the_key():
    df_a, df_b = frames()
    stats = {}
    res = P.compare_boxes_frame(df_a, df_b, backend=BE, stats=stats)
    want = expected_comparison(df_a[COL].tolist()[:3], [df_b[COL].iat[1], df_b[COL].iat[0], df_b[COL].iat[3]], 0.5, False,
                               ["u0", "u1", "u2"])
    check_comparison(res, want)
    assert res.per_row["row"].tolist() == [0, 1, 2] and res.totals["agree"] == 3
    assert res.differences[["row", "source", "kind", "a_name"]].values.tolist() == [[1, "u1", "missing", "b"]]
    assert res.unpaired.values.tolist() == [["u3", "a"], ["u9", "b"]]
    assert res.totals["rows_only_a"] == 1 and res.totals["rows_only_b"] == 1 and stats == res.totals
    shifted = df_a.iloc[[3, 0, 1, 2]].reset_index(drop=True)   # rows are positions in df_a
    res = P.compare_boxes_frame(shifted, df_b, backend=BE)
    assert res.per_row["row"].tolist() == [1, 2, 3] and res.differences["row"].tolist() == [2]


def test_frame_by_position_and_within_one_frame():
    df_a, df_b = frames()
    res = P.compare_boxes_frame(df_a, df_b, key=None, backend=BE)
    check_comparison(res, expected_comparison(df_a[COL].tolist(), df_b[COL].tolist(), 0.5, False, df_a["source"].tolist()))
    assert res.totals["rows_only_a"] == 0 and len(res.unpaired) == 0
    both = df_a.assign(other=df_b[COL].to_numpy())
    res2 = P.compare_boxes_frame(both, other_col="other", iou_threshold=0.3, by_label=True, backend=BE)
    check_comparison(res2, expected_comparison(df_a[COL].tolist(), df_b[COL].tolist(), 0.3, True, df_a["source"].tolist()))


def test_frame_errors():
    df_a, df_b = frames()
    with pytest.raises(ValueError, match="by position"):
        P.compare_boxes_frame(df_a, df_b.iloc[:3], key=None, backend=BE)
    dup = pd.concat([df_b, df_b.iloc[:1]], ignore_index=True)
    with pytest.raises(ValueError, match="more than once.*dedup"):
        P.compare_boxes_frame(df_a, dup, backend=BE)
    with pytest.raises(ValueError, match="more than once.*dedup"):
        P.compare_boxes_frame(dup, df_a, backend=BE)
    with pytest.raises(ValueError, match="other_col"):
        P.compare_boxes_frame(df_a, backend=BE)


def test_chunks_with_different_class_lists(monkeypatch):
    rng = np.random.default_rng(5)
    names = ["a", "b", "c", 7, "e", "f"]
    cells_a, cells_b = [], []
    for r in range(23):
        pool = names[(r // 4) % 4:][:1 + (r // 4) % 3]         # the names drift from chunk to chunk
        objs = [ob(pool[int(rng.integers(0, len(pool)))], *(int(v) for v in (x, y, x + w, y + h)))
                for x, y, w, h in rng.integers(1, 40, (int(rng.integers(1, 6)), 4))]
        other = [dict(o, name=pool[int(rng.integers(0, len(pool)))]) if rng.random() < 0.4 else o for o in objs
                 if rng.random() < 0.8]
        cells_a.append(cell(*objs))
        cells_b.append(cell(*other))
    whole = compare(cells_a, cells_b)
    monkeypatch.setattr(P, "_NATIVE_CHUNK_CELLS", 4)
    calls = []
    monkeypatch.setattr(BE, "compare_boxes", lambda *a: calls.append(a[6]) or CompareBackend.compare_boxes(BE, *a), raising=False)
    parts = compare(cells_a, cells_b)
    assert len(calls) == 6 and len(set(calls)) > 1             # class lists of different lengths
    assert parts.differences.equals(whole.differences) and parts.confusion.equals(whole.confusion)
    assert whole.totals["relabelled"] > 0 and whole.totals["missing"] > 0 and None in whole.classes


# ----------------------------------------------------------------------------------------------- CSV routes
def test_csv_native_route_against_pandas_route(tmp_path, monkeypatch):
    df_a, df_b = frames()
    pa, pb = tmp_path / "a.csv", tmp_path / "b.csv"
    df_a.to_csv(pa, index=False, encoding="utf-8-sig")
    df_b.to_csv(pb, index=False, encoding="utf-8-sig")
    res = P.compare_boxes_csv(pa, pb, tmp_path / "n", backend=BE)
    assert P.LAST_IO_PATH["compare"] == "native"
    monkeypatch.setenv("DYD_NATIVE_CSV", "0")
    res2 = P.compare_boxes_csv(pa, pb, tmp_path / "p", backend=BE)
    assert P.LAST_IO_PATH["compare"] == "pandas"
    assert {k: v for k, v in res.items() if k != "paths"} == {k: v for k, v in res2.items() if k != "paths"}
    assert res["rows"] == 3 and res["rows_only_a"] == 1 and res["agree"] == 3 and res["missing"] == 1
    for k in ("confusion", "classes", "differences", "rows"):
        data = open(res["paths"][k], "rb").read()
        assert data.startswith(b"\xef\xbb\xbf") and data == open(res2["paths"][k], "rb").read()
    want = P.compare_boxes_frame(pd.read_csv(pa, encoding="utf-8-sig"), pd.read_csv(pb, encoding="utf-8-sig"), backend=BE)
    assert pd.read_csv(res["paths"]["differences"], encoding="utf-8-sig")["kind"].tolist() == want.differences["kind"].tolist()
    conf = pd.read_csv(res["paths"]["confusion"], encoding="utf-8-sig", index_col=0)
    assert conf.to_numpy().tolist() == want.confusion.to_numpy().tolist() and list(conf.columns) == ["a", "b", "c", "(none)"]
    with np.load(res["paths"]["hist"]) as z:
        assert z["classes"].tolist() == ["a", "b", "c"] and np.array_equal(z["hist_iou"], want.hist_iou)
    by_pos = P.compare_boxes_csv(pa, pb, tmp_path / "q", key=None, backend=BE)
    assert by_pos["rows"] == 4 and by_pos["rows_only_a"] == 0


def test_csv_error_conventions(tmp_path, capsys):
    df_a, _ = frames()
    good = tmp_path / "a.csv"
    df_a.to_csv(good, index=False, encoding="utf-8-sig")
    assert P.compare_boxes_csv(tmp_path / "nope.csv", good, tmp_path / "o", backend=BE) is None
    assert "读取失败" in capsys.readouterr().out
    bad = tmp_path / "bad.csv"
    df_a.rename(columns={COL: "other"}).to_csv(bad, index=False, encoding="utf-8-sig")
    assert P.compare_boxes_csv(good, bad, tmp_path / "o", backend=BE) is None
    assert "错误：缺少必要列" in capsys.readouterr().out
    nokey = tmp_path / "nokey.csv"
    df_a.drop(columns=["source"]).to_csv(nokey, index=False, encoding="utf-8-sig")
    assert P.compare_boxes_csv(good, nokey, tmp_path / "o", backend=BE) is None
    assert "错误：缺少必要列 source" in capsys.readouterr().out
    assert not (tmp_path / "o").exists()
