"""K18 (box comparison) on the MI355X: both ABI entries against the restatement (tests/box_compare_ref.py) with all seven
outputs equal, closed-form displacement chains across the 64-box tiles, and the step functions on synthetic tables."""
import json

import numpy as np
import pandas as pd
import pytest

from box_compare_ref import check_comparison, compare_rows, expected_comparison, records, same_outputs
from test_box_suppress_cpu import KNOWN

from deal_yolo_daya_amd import synth
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu
COL = P.BBOX_COL
THRS = [0.5, 0.98, 0.0, -1.0, 1.0, float("nan")]
N_CLASSES = 3


def _boxes(rng, n):
    """boxes as test_gpu_box_suppress._rows_table makes them: rounded, 30 % with swapped corners"""
    c = rng.uniform(0, 200, (n, 2))
    box4 = np.round(np.concatenate([c, c + rng.uniform(1, 60, (n, 2))], axis=1), 1)
    swap = rng.random(n) < 0.3
    box4[swap] = box4[swap][:, [2, 3, 0, 1]]
    return box4


def _tables(sizes, rng, special=True):
    """sizes = [(na, nb)] per row -> (a_box4, a_off, a_cls, b_box4, b_off, b_cls, n_classes).  B is made from A by copying,
    jittering, dropping and reclassing, plus unrelated boxes; NaN, +-inf and -0.0 are planted on both sides."""
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    a_off, b_off = np.zeros(len(sizes) + 1, np.int32), np.zeros(len(sizes) + 1, np.int32)
    np.cumsum(sizes[:, 0], out=a_off[1:])
    np.cumsum(sizes[:, 1], out=b_off[1:])
    na, nb = int(a_off[-1]), int(b_off[-1])
    a = _boxes(rng, na)
    a_cls = rng.integers(0, N_CLASSES, na).astype(np.int32)
    b = _boxes(rng, nb)
    b_cls = rng.integers(0, N_CLASSES, nb).astype(np.int32)
    for r in range(len(sizes)):
        if a_off[r + 1] == a_off[r]:
            continue
        for j in range(b_off[r], b_off[r + 1]):
            u = rng.random()
            if u < 0.75:                                       # a copy of an A box of the row ...
                i = rng.integers(a_off[r], a_off[r + 1])
                b[j], b_cls[j] = a[i], a_cls[i]
                if u < 0.3:                                    # ... jittered
                    b[j, 3] = b[j, 1] + (b[j, 3] - b[j, 1]) * (0.985 if u < 0.15 else 0.7)
                elif u < 0.4:                                  # ... under another class
                    b_cls[j] = (b_cls[j] + 1) % N_CLASSES
    if special:
        vals = [np.nan, np.inf, -np.inf, -0.0]
        for t in (a, b):
            if len(t) >= 8:
                for k, q in enumerate(rng.choice(len(t), max(4, len(t) // 50), replace=False)):
                    t[q, k % 4] = vals[k % 4]
    return a, a_off, a_cls, b, b_off, b_cls, N_CLASSES


def _dev_call(native, a_box4, a_off, a_cls, b_box4, b_off, b_cls, n_classes, thr, by_label, hz=None):
    """dyd_compare_boxes_dev on torch buffers, every output prefilled with a sentinel so that an unwritten element shows; on a
    delayed side stream through the harness of tests/stream_contract.py (`hz`: the caller's own, with its own decoys)"""
    import torch
    from stream_contract import Harness, moved, rev_off, rot_cls

    hz = hz or Harness((moved(a_box4, 4), rev_off(a_off), rot_cls(a_cls, n_classes), moved(b_box4, 4), rev_off(b_off),
                        rot_cls(b_cls, n_classes)))

    dev = torch.device("cuda:0")
    n, na, nb = len(a_off) - 1, int(a_off[-1]), int(b_off[-1])
    put = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dt)).to(dev)      # noqa: E731
    ins = [put(np.asarray(a_box4, np.float64).reshape(-1), np.float64), put(a_off, np.int32), put(a_cls, np.int32),
           put(np.asarray(b_box4, np.float64).reshape(-1), np.float64), put(b_off, np.int32), put(b_cls, np.int32)]
    full = lambda m, v, dt: torch.full((max(m, 1),), v, dtype=dt, device=dev)      # noqa: E731
    cells = (n_classes + 1) ** 2
    outs = [full(na, -7, torch.int32), full(nb, -7, torch.int32), full(nb, -7.0, torch.float64), full(na, -7.0, torch.float64),
            full(nb, -7.0, torch.float64), full(4 * n, -7, torch.int32), full(cells, 77, torch.int64)]
    hz.arm(ins)
    hz.watch(*outs)
    rc = hz.call(native.lib().dyd_compare_boxes_dev, *(t.data_ptr() for t in ins), n, na, nb, n_classes, float(thr), int(by_label),
                 *(t.data_ptr() for t in outs))
    native.check(rc, "dyd_compare_boxes_dev")
    hz.restore()
    res = [t.cpu().numpy()[:m] for t, m in zip(outs, (na, nb, nb, na, nb, 4 * n, cells))]
    res[5] = res[5].reshape(n, 4)
    res[6] = res[6].reshape(n_classes + 1, n_classes + 1)
    return res


_WANT = {}


def _check(native, key, tables, thr, by_label):
    """both entries against the restatement; `key` shares the restatement's answer among the tests that use the same table"""
    k = (key, repr(thr), by_label)
    if k not in _WANT:
        _WANT[k] = compare_rows(*tables, thr, by_label)
    want = _WANT[k]
    same_outputs(native.compare_boxes(*tables, thr, by_label), want, f"host entry, thr={thr}")
    same_outputs(_dev_call(native, *tables, thr, by_label), want, f"dev entry, thr={thr}")
    return want


_TABLES = {}


def _small_tables():
    if "small" not in _TABLES:
        rng = np.random.default_rng(18)
        fixed = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 63), (64, 64), (1, 64), (64, 1), (63, 1), (0, 64)]
        sizes = np.concatenate([np.asarray(fixed), rng.integers(0, 65, (400, 2))])
        rng.shuffle(sizes)
        _TABLES["small"] = _tables(sizes, rng)
    return _TABLES["small"]


def _big_tables():
    if "big" not in _TABLES:
        rng = np.random.default_rng(19)
        big = [(65, 3), (3, 65), (64, 300), (129, 70), (257, 256), (1000, 1500)]
        sizes = np.concatenate([np.asarray(big), rng.integers(0, 40, (30, 2))])
        rng.shuffle(sizes)
        _TABLES["big"] = _tables(sizes, rng)
    return _TABLES["big"]


@pytest.mark.parametrize("thr", THRS)
@pytest.mark.parametrize("by_label", [False, True])
def test_k18_small_rows(native, thr, by_label):
    _check(native, "small", _small_tables(), thr, by_label)


@pytest.mark.parametrize("thr", THRS)
@pytest.mark.parametrize("by_label", [False, True])
def test_k18_big_rows(native, thr, by_label):
    _check(native, "big", _big_tables(), thr, by_label)


def test_k18_very_big_row(native):
    rng = np.random.default_rng(20)
    tables = _tables([(2, 3), (5, 1), (3000, 2000)], rng, special=False)
    want = _check(native, "very_big", tables, 0.9, False)
    assert (want[1] >= 0).sum() > 500
    _check(native, "very_big", tables, 0.9, True)


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 4097])
def test_k18_displacement_chain(native, n):
    """A_i = (i, 0, i + 50, 1), B_j = (j + 0.75, 0, j + 50.75, 1): IoU(A_j, B_j) = 49.25 / 50.75 and IoU(A_j+1, B_j) =
    49.75 / 50.25, both above 0.95, every other pair below.  In order every B box takes its first choice A_j+1 and the last
    finds it missing and A_n-1 taken; reversed, every B box but the first finds its first choice taken and falls back to A_j."""
    x = np.arange(n, dtype=np.float64)
    a = np.stack([x, np.zeros(n), x + 50.0, np.ones(n)], axis=1)
    b = np.stack([x + 0.75, np.zeros(n), x + 50.75, np.ones(n)], axis=1)
    cls = np.zeros(n, np.int32)
    off = np.array([0, n], np.int32)
    thr = 0.95
    am, bm, *_ = native.compare_boxes(a, off, cls, b, off, cls, 1, thr)
    assert bm.tolist() == list(range(1, n)) + [-1]
    assert am.tolist() == [-1] + list(range(n - 1))
    _check(native, ("chain", n), (a, off, cls, b, off, cls, 1), thr, False)
    rev = b[::-1].copy()
    am, bm, *_ = native.compare_boxes(a, off, cls, rev, off, cls, 1, thr)
    assert bm.tolist() == [n - 1 - k for k in range(n)]
    assert am.tolist() == [n - 1 - i for i in range(n)]
    _check(native, ("chain_rev", n), (a, off, cls, rev, off, cls, 1), thr, False)
    lead_a = np.array([[0.0, 0.0, 1.0, 1.0]] * 5)                         # the same chain behind a few small rows
    lead_b = np.array([[0.0, 0.0, 1.0, 1.0]] * 3)
    tables = (np.concatenate([lead_a, a]), np.array([0, 2, 5, 5 + n], np.int32), np.zeros(5 + n, np.int32),
              np.concatenate([lead_b, rev]), np.array([0, 3, 3, 3 + n], np.int32), np.zeros(3 + n, np.int32), 1)
    _check(native, ("chain_lead", n), tables, thr, False)


def test_k18_edges_of_the_entries(native):
    z4, zi, zo = np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros(1, np.int32)
    res = native.compare_boxes(z4, zo, zi, z4, zo, zi, 2, 0.5)
    assert [len(v) for v in res[:5]] == [0] * 5 and res[5].shape == (0, 4) and not res[6].any()
    off = np.zeros(4, np.int32)                                           # rows without boxes: counts and confusion are zeroed
    tables = (z4, off, zi, z4, off, zi, 2)
    same_outputs(_dev_call(native, *tables, 0.5, False), compare_rows(*tables, 0.5, False), "no boxes")
    assert native.lib().dyd_compare_boxes_dev(None, None, None, None, None, None, 0, 0, 0, 0, 0.5, 0, None, None, None, None,
                                              None, None, None, None) == 0
    one = np.array([[0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(native.NativeError, match="class id"):
        native.compare_boxes(one, [0, 1], [2], one, [0, 1], [0], 2, 0.5)
    with pytest.raises(native.NativeError, match="monotone"):
        _bad_offsets(native)
    many = 40                                                             # (C+1)^2 above the LDS budget: global atomics
    rng = np.random.default_rng(21)
    t = list(_tables(rng.integers(0, 30, (50, 2)), rng))
    t[2] = rng.integers(0, many, len(t[2])).astype(np.int32)
    t[5] = rng.integers(0, many, len(t[5])).astype(np.int32)
    t[6] = many
    _check(native, "many_classes", tuple(t), 0.5, False)


def _bad_offsets(native):
    one = np.array([[0.0, 0.0, 1.0, 1.0]] * 2)
    a_off = np.array([0, 2, 1, 2], np.int32)                              # ends right, dips in between
    cls = np.zeros(2, np.int32)
    out = [np.zeros(8, np.int64) for _ in range(7)]
    rc = native.lib().dyd_compare_boxes(native._ptr(one.reshape(-1)), native._ptr(a_off), native._ptr(cls),
                                        native._ptr(one.reshape(-1)), native._ptr(a_off), native._ptr(cls), 3, 1, 0.5, 0,
                                        *(native._ptr(o) for o in out))
    native.check(rc, "dyd_compare_boxes")


# ----------------------------------------------------------------------------------------------- step level
def ob(name, x1, y1, x2, y2):
    return {"name": name, "polygon": {"ptList": [{"x": x1, "y": y1}, {"x": x2, "y": y2}]}}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def test_by_label_semantics(native):
    """the known answers of test_box_compare_cpu.py through the real backend"""
    a = [cell(ob("cat", 0, 0, 10, 10)), cell(ob("a", 0, 0, 10, 10)), cell(ob("a", 0, 0, 10, 10), ob("a", 0, 0, 10, 10)),
         cell(ob("a", 5, 5, 5, 9)), cell(ob(3, 0, 0, 10, 10), ob("z", 20, 20, 30, 30)), None]
    b = [cell(ob("dog", 0, 0, 10, 10)), cell(ob("a", 0, 0, 10, 9), ob("a", 0, 0, 10, 10)), cell(ob("a", 0, 0, 10, 10)),
         cell(ob("a", 5, 5, 5, 9)), cell(ob("z", 0, 0, 10, 10), ob("z", 20, 20, 30, 30)), cell(ob("q", 1, 1, 2, 2))]
    for thr in (0.5, 0.0):
        for by_label in (False, True):
            res = P.compare_boxes_cells(a, b, thr, by_label)
            check_comparison(res, expected_comparison(a, b, thr, by_label))
    res = P.compare_boxes_cells(a, b, 0.5, False)
    d = res.differences
    assert d[d["row"] == 0][["kind", "a_name", "b_name", "iou"]].values.tolist() == [["relabelled", "cat", "dog", 1.0]]
    assert d[d["row"] == 1][["kind", "b_object", "best_iou"]].values.tolist() == [["extra", 1, 1.0]]
    assert d[d["row"] == 2][["kind", "a_object"]].values.tolist() == [["missing", 1]]
    assert d[d["row"] == 3]["kind"].tolist() == ["missing", "extra"]
    assert d[d["row"] == 4]["kind"].tolist() == ["relabelled"] and res.classes[-1] is None
    res = P.compare_boxes_cells(a, b, 0.5, True)
    d = res.differences
    assert d[d["row"] == 0][["kind", "best_iou"]].values.tolist() == [["missing", 1.0], ["extra", 1.0]]
    assert "relabelled" not in set(d["kind"])


def _replaced(n_rows, seed):
    df = synth.to_frame(synth.generate(n_rows, seed=seed, dup_prob=0.2))
    kept, _ = P.replace_ptlist_frame(df)
    kept = kept.reset_index(drop=True)
    kept["source"] = kept["source"] + "#" + kept.index.astype(str)        # synth repeats sources for the dedup step: one key per row
    return kept


def _other_cells(cells, rng, names=("猫", "new")):
    """about 10 % of the boxes dropped, 10 % jittered, 5 % renamed, one row in ten with its objects reversed"""
    out = []
    for c in cells:
        if not isinstance(c, str):
            out.append(c)
            continue
        doc = json.loads(c)
        objs = []
        for o in doc.get("objects", []):
            u = rng.random()
            if u < 0.10:
                continue
            o = json.loads(json.dumps(o))
            pts = o.get("polygon", {}).get("ptList") or []
            if u < 0.20 and len(pts) == 2 and isinstance(pts[1].get("y"), (int, float)):
                pts[1]["y"] = pts[1]["y"] + (2.5 if u < 0.15 else 400)
            elif u < 0.25:
                o["name"] = names[int(rng.integers(0, len(names)))]
            objs.append(o)
        if rng.random() < 0.1:
            objs.reverse()
        doc["objects"] = objs
        out.append(json.dumps(doc, ensure_ascii=False))
    return out


def test_step_level_20k(native):
    df = _replaced(20_000, 51)
    rng = np.random.default_rng(52)
    other = df.copy()
    other[COL] = pd.Series(_other_cells(df[COL].tolist(), rng), dtype=object)
    stats = {}
    res = P.compare_boxes_frame(df, other, stats=stats)
    want = expected_comparison(df[COL].tolist(), other[COL].tolist(), 0.5, False, df["source"].tolist())
    check_comparison(res, want)
    assert res.totals["missing"] > 100 and res.totals["extra"] > 100 and res.totals["relabelled"] > 100
    assert stats == res.totals and res.totals["rows_only_a"] == 0 and len(res.unpaired) == 0
    shuffled = other.sample(frac=1.0, random_state=3).reset_index(drop=True)       # the key brings the rows back together
    check_comparison(P.compare_boxes_frame(df, shuffled), want)
    twin = P.compare_boxes_frame(df, df, key=None)
    assert twin.totals["relabelled"] == 0 and twin.totals["missing"] == twin.totals["extra"]
    d = twin.differences                                                            # only a box of zero area misses its twin
    assert (((d["ax2"] - d["ax1"]) * (d["ay2"] - d["ay1"]) == 0) | ((d["bx2"] - d["bx1"]) * (d["by2"] - d["by1"]) == 0)).all()


def test_csv_path_mixed(native, tmp_path):
    df = _replaced(3000, 53)
    rng = np.random.default_rng(54)
    cells_a, cells_b = df[COL].tolist(), _other_cells(df[COL].tolist(), rng)
    cells_a[1], cells_b[2] = KNOWN["big_ints_tie"], KNOWN["big_ints_tie"]
    cells_a[3], cells_b[3] = KNOWN["undecodable"], KNOWN["non_ascii"]
    cells_a[4], cells_b[5] = None, None
    cells_a[6], cells_b[6] = KNOWN["repeated_key"], KNOWN["repeated_key"]
    cells_a[7], cells_b[8] = KNOWN["non_ascii"], KNOWN["undecodable"]
    a = df.assign(**{COL: pd.Series(cells_a, dtype=object)})
    b = df.assign(**{COL: pd.Series(cells_b, dtype=object)}).iloc[::-1]
    pa, pb = tmp_path / "a.csv", tmp_path / "b.csv"
    a.to_csv(pa, index=False, encoding="utf-8-sig")
    b.to_csv(pb, index=False, encoding="utf-8-sig")
    res = P.compare_boxes_csv(pa, pb, tmp_path / "out")
    back_a, back_b = pd.read_csv(pa, encoding="utf-8-sig"), pd.read_csv(pb, encoding="utf-8-sig").iloc[::-1]
    want = expected_comparison(back_a[COL].tolist(), back_b[COL].tolist(), 0.5, False, back_a["source"].tolist())
    assert {k: res[k] for k in want["totals"]} == want["totals"] and res["rows"] == 3000
    ref = tmp_path / "ref"
    ref.mkdir()
    want["confusion"].to_csv(ref / "confusion.csv", index_label="a_class", encoding="utf-8-sig")
    for k, nm in (("classes", "per_class"), ("differences", "differences"), ("rows", "per_row")):
        want[nm].to_csv(ref / f"{k}.csv", index=False, encoding="utf-8-sig")
    for k in ("confusion", "classes", "differences", "rows"):
        assert open(res["paths"][k], "rb").read() == (ref / f"{k}.csv").read_bytes(), k
    with np.load(res["paths"]["hist"]) as z:
        assert np.array_equal(z["hist_iou"], want["hist_iou"])


def test_sampled_200k(native):
    df = _replaced(200_000, 55)
    rng = np.random.default_rng(56)
    cells_a = df[COL].tolist()
    cells_b = list(cells_a)
    pick = np.sort(rng.choice(len(df), 3000, replace=False))
    for r, c in zip(pick.tolist(), _other_cells([cells_a[r] for r in pick.tolist()], rng)):
        cells_b[r] = c
    res = P.compare_boxes_cells(cells_a, cells_b)
    t = res.totals
    assert t["matched"] + t["missing"] == t["a_boxes"] and t["matched"] + t["extra"] == t["b_boxes"]
    assert t["matched"] == t["agree"] + t["relabelled"] and t["rows"] == len(df)
    want = expected_comparison([cells_a[r] for r in pick.tolist()], [cells_b[r] for r in pick.tolist()])
    got_rows = res.per_row.iloc[pick].drop(columns=["row"])
    assert records(got_rows) == records(want["per_row"].drop(columns=["row"]))
    got = res.differences[res.differences["row"].isin(pick)]
    exp = want["differences"].assign(row=pick[want["differences"]["row"].to_numpy()])
    assert list(got.columns) == list(exp.columns) and len(exp) > 100
    assert records(got) == records(exp)
