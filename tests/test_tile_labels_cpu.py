"""Tiled YOLO labels (core/processor.py: yolo_tile_label_texts, tile_yolo_frame, tile_yolo_csv), host side: the grid, the
visibility rule at equality, a vertex on a shared tile edge, the tile text against the segment step's own Python lines, detect
mode against K7's formula, class handling, the files written and the crops — driven by a test backend whose device stage is
the restatement of tests/tile_labels_ref.py; tests/test_gpu_tile_labels.py checks K20 itself.  Known answers are worked by
hand.  No GPU."""
import json
import math

import numpy as np
import pandas as pd
import pytest

import tile_labels_ref as R
from helpers import OracleBackend

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd.core import processor as P

COL = P.ANNOTATION_COL


class TileBackend(OracleBackend):
    def yolo_tile_lines(self, xy, pt_off, row_off, cls, width, height, tile_w, tile_h, step_x, step_y, min_visibility=0.1, mode=0,
                        max_tiles_per_row=4096):
        return R.tile_arrays(xy, pt_off, row_off, cls, width, height, tile_w, tile_h, step_x, step_y, min_visibility, mode,
                             max_tiles_per_row)


BE = TileBackend()


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def tiles_of(cells, widths, heights, **kw):
    return P.yolo_tile_label_texts(cells, widths, heights, backend=BE, **kw)


def boxes(res):
    return res.tiles[["row", "tile", "x0", "y0", "w", "h"]].values.tolist()


# ----------------------------------------------------------------------------------------------- the grid
def axis_through_the_package(L, T, S):
    """[(origin, extent)] of one axis of length L, from flatten.tile_grid / tile_boxes (the other axis is one tile)"""
    status, nx, ny = fl.tile_grid([L], [5], T, 5, S, 1)
    assert status.tolist() == [0] and ny.tolist() == [1]
    row, tile, x0, y0, w, h = fl.tile_boxes([L], [5], nx, ny, T, 5, S, 1)
    assert tile.tolist() == list(range(int(nx[0]))) and set(y0.tolist()) == {0} and set(h.tolist()) == {5}
    ys, _, ny2 = fl.tile_grid([5], [L], 5, T, 1, S)                                  # and the same axis as the image's height
    assert ny2.tolist() == nx.tolist()
    return list(zip(x0.tolist(), w.tolist()))


@pytest.mark.parametrize("L, T, S, want", [
    (10, 10, 8, [(0, 10)]), (7, 10, 8, [(0, 7)]),                                    # L <= T: one tile of extent L
    (11, 10, 10, [(0, 10), (1, 10)]),                                                # L = T + 1: origins 0 and 1
    (25, 10, 8, [(0, 10), (8, 10), (15, 10)]),                                       # the last tile moved back to the edge
    (30, 10, 10, [(0, 10), (10, 10), (20, 10)]),                                     # S = T: no overlap
    (26, 10, 8, [(0, 10), (8, 10), (16, 10)])])                                      # ends exactly at the edge
def test_axis_known_answers(L, T, S, want):
    assert axis_through_the_package(L, T, S) == want and R.axis(L, T, S) == want
    c = cell(ob("a", [(1, 1), (3, 1), (3, 3)]))
    res = tiles_of([c], [L], [5], tile=(T, 5), step=(S, 1))                          # and through the step
    assert list(zip(res.tiles["x0"].tolist(), res.tiles["w"].tolist())) == want


def test_grid_through_the_step_and_the_host_helpers():
    c = cell(ob("a", [(1, 1), (3, 1), (3, 3)]))
    res = tiles_of([c, c], [25, 11], [7, 25], tile=10, step=(8, 10))
    assert boxes(res) == [[0, 0, 0, 0, 10, 7], [0, 1, 8, 0, 10, 7], [0, 2, 15, 0, 10, 7],
                          [1, 0, 0, 0, 10, 10], [1, 1, 1, 0, 10, 10], [1, 2, 0, 10, 10, 10], [1, 3, 1, 10, 10, 10],
                          [1, 4, 0, 15, 10, 10], [1, 5, 1, 15, 10, 10]]
    assert res.row_status.tolist() == ["tiled", "tiled"]
    status, nx, ny = fl.tile_grid([25, 11], [7, 25], 10, 10, 8, 10)
    assert status.tolist() == [0, 0] and nx.tolist() == [3, 2] and ny.tolist() == [1, 3]
    assert [list(map(int, t)) for t in zip(*fl.tile_boxes([25, 11], [7, 25], nx, ny, 10, 10, 8, 10))] == boxes(res)


def test_default_step_from_the_overlap():
    assert P._tile_params(640, 0.2, None, 0.1, "segment", 4096)[:4] == (640, 640, 512, 512)
    assert P._tile_params((100, 7), 0.5, None, 0.1, "detect", 1)[:4] == (100, 7, 50, 4)
    assert P._tile_params(3, 0.99, None, 0, "segment", 1)[2:4] == (1, 1)
    assert P._tile_params(10, 0.9, (3, 4), 0, "segment", 1)[2:4] == (3, 4)          # a given step wins


def test_the_three_row_statuses_that_are_not_tiled():
    c = cell(ob("a", [(1, 1), (3, 1), (3, 3)]))
    res = tiles_of([c] * 6, [0, 20.5, 100, 20, math.nan, 2.0 ** 43], [10, 10, 100, 10, 5, 5], tile=10, step=10,
                   max_tiles_per_row=99)
    assert res.row_status.tolist() == ["no_size", "fractional_size", "too_many_tiles", "tiled", "no_size", "no_size"]
    assert res.tiles["row"].tolist() == [3, 3]
    assert res.polygons["action"].tolist() == ["no_size", "written", "written", "written", "no_size", "no_size"]
    t = res.totals
    assert (t["rows_no_size"], t["rows_fractional_size"], t["rows_too_many_tiles"], t["rows_tiled"]) == (3, 1, 1, 1)
    assert t["lost"] == 2                                # written in the image, in a row without tiles
    assert tiles_of([c], [100], [100], tile=10, step=10, max_tiles_per_row=100).row_status.tolist() == ["tiled"]


# ----------------------------------------------------------------------------------------------- visibility
BOX = cell(ob("a", [(5, 2), (15, 8)]))                   # two points: the box 5..15 x 2..8, A_img = 60, 30 in either tile


def test_visibility_at_equality_writes_both_tiles_and_both_are_cut():
    res = tiles_of([BOX], [20], [10], tile=10, step=10, min_visibility=0.5)
    assert res.tiles["lines"].tolist() == [1, 1]
    assert res.tiles["text"].tolist() == ["0 0.500000 0.200000 1.000000 0.200000 1.000000 0.800000 0.500000 0.800000",
                                          "0 0.000000 0.200000 0.500000 0.200000 0.500000 0.800000 0.000000 0.800000"]
    assert res.polygons[["tiles_written", "tiles_cut", "tiles_dropped"]].values.tolist() == [[2, 2, 0]]
    assert res.totals["lost"] == 0


def test_visibility_one_ulp_above_writes_neither_and_the_object_is_lost(tmp_path):
    mv = 0.5000000000000001
    assert mv > 0.5 and mv * 60.0 > 30.0
    res = tiles_of([BOX], [20], [10], tile=10, step=10, min_visibility=mv)
    assert res.tiles["lines"].tolist() == [0, 0] and res.tiles["text"].tolist() == ["", ""]
    assert res.polygons[["tiles_written", "tiles_cut", "tiles_dropped"]].values.tolist() == [[0, 0, 2]]
    assert res.per_class[["class", "polygons", "tiles_written", "tiles_cut", "tiles_dropped", "lost"]].values.tolist() == \
        [["a", 1, 0, 0, 2, 1]]
    df = pd.DataFrame({"source": ["/data/img one.png"], COL: [BOX], "width": [20], "height": [10]})
    out = P.tile_yolo_frame(df, tmp_path / "ds", tile=10, step=10, min_visibility=mv, lost_csv=tmp_path / "lost.csv", backend=BE)
    assert out["lost"] == 1 and out["label_files"] == 0 and not list((tmp_path / "ds" / "labels" / "train").iterdir())
    lost = pd.read_csv(tmp_path / "lost.csv", encoding="utf-8-sig")
    assert lost[["source", "row", "object", "name", "action", "tiles_dropped"]].values.tolist() == \
        [["/data/img one.png", 0, 0, "a", "written", 2]]


def test_zero_image_area_always_passes():
    # a bow-tie whose loops cancel: A_img == 0.0, so A_tile >= 1.0 * 0.0 holds in the tile that holds it
    bow = cell(ob("a", [(1, 1), (3, 3), (3, 1), (1, 3)]))
    res = tiles_of([bow], [20], [10], tile=10, step=10, min_visibility=1.0)
    assert res.tiles["lines"].tolist() == [1, 0]
    assert res.polygons[["tiles_written", "tiles_dropped"]].values.tolist() == [[1, 0]]


def test_vertex_exactly_on_a_shared_tile_edge():
    tri = cell(ob("a", [(5, 2), (10, 5), (5, 8)]))       # (10, 5) lies on x = 10, the edge tiles 0 and 1 share
    res = tiles_of([tri], [20], [10], tile=10, step=10, min_visibility=0.0)
    assert res.tiles["text"].tolist() == ["0 0.500000 0.200000 1.000000 0.500000 0.500000 0.800000", ""]
    assert res.polygons[["tiles_written", "tiles_cut", "tiles_dropped"]].values.tolist() == [[1, 0, 0]]   # empty in tile 1


# ----------------------------------------------------------------------------------------------- against the segment step
def random_cells(rng, n_rows, names=("a", "b", "c")):
    cells, W, H = [], [], []
    for _ in range(n_rows):
        w, h = int(rng.integers(20, 120)), int(rng.integers(20, 120))
        objs = []
        for _ in range(int(rng.integers(0, 6))):
            m = int(rng.integers(2, 9))
            far = rng.random() < 0.2
            pts = [(round(float(rng.uniform(-30 if far else 0, w + (30 if far else 0))), 2),
                    round(float(rng.uniform(-30 if far else 0, h + (30 if far else 0))), 2)) for _ in range(m)]
            objs.append(ob(str(rng.choice(names)), pts))
        cells.append(cell(*objs))
        W.append(w)
        H.append(h)
    return cells, W, H


def test_tile_text_is_the_segment_steps_text_of_the_moved_polygon():
    rng = np.random.default_rng(7)
    cells, W, H = random_cells(rng, 30)
    classes = ["a", "b", "c"]
    res = tiles_of(cells, W, H, classes=classes, tile=(32, 24), step=(20, 24), min_visibility=0.0)
    n_lines = 0
    for _, t in res.tiles.iterrows():
        want = []
        for o in json.loads(cells[t["row"]])["objects"]:
            pts = [(float(p["x"]), float(p["y"])) for p in o["polygon"]["ptList"]]
            if P._seg_lines_python([pts], 0, W[t["row"]], H[t["row"]])[1][0] > 1:
                continue                                 # not written or clipped in the image
            if len(pts) == 2:
                pts = R.vertices(pts)
            moved = [(x - float(t["x0"]), y - float(t["y0"])) for x, y in pts]
            want += P._seg_lines_python([moved], classes.index(o["name"]), float(t["w"]), float(t["h"]))[0]
        assert t["text"] == "\n".join(want) and t["lines"] == len(want)
        n_lines += len(want)
    assert n_lines > 100 and (res.tiles["lines"] == 0).any()


def test_detect_mode_is_k7s_line_of_the_part_inside_the_tile():
    res = tiles_of([BOX], [20], [10], tile=10, step=10, min_visibility=0.0, task="detect")
    assert res.tiles["text"].tolist() == ["0 0.750000 0.500000 0.500000 0.600000", "0 0.250000 0.500000 0.500000 0.600000"]
    assert res.tiles["text"].tolist() == [P._label_lines_python([("a", 5.0, 2.0, 10.0, 8.0)], 0, 10.0, 10.0)[0],
                                          P._label_lines_python([("a", 0.0, 2.0, 5.0, 8.0)], 0, 10.0, 10.0)[0]]
    rng = np.random.default_rng(11)
    cells, W, H = random_cells(rng, 12)
    seg = tiles_of(cells, W, H, tile=32, step=24, min_visibility=0.3)
    det = tiles_of(cells, W, H, tile=32, step=24, min_visibility=0.3, task="detect")
    assert seg.tiles["lines"].tolist() == det.tiles["lines"].tolist() and seg.polygons.equals(det.polygons)
    for s, d, tw, th in zip(seg.tiles["text"], det.tiles["text"], seg.tiles["w"], seg.tiles["h"]):
        for sl, dl in zip(s.split("\n") if s else [], d.split("\n") if d else []):
            v = sl.split()
            xs, ys = [float(a) for a in v[1::2]], [float(a) for a in v[2::2]]
            got = [float(a) for a in dl.split()[1:]]
            want = [(min(xs) + max(xs)) / 2, (min(ys) + max(ys)) / 2, max(xs) - min(xs), max(ys) - min(ys)]
            assert dl.split()[0] == v[0] and np.allclose(got, want, atol=2.1e-6)   # both texts are rounded to 1e-6


# ----------------------------------------------------------------------------------------------- classes
def test_classes_labels_and_unknown_class():
    tri = [(1, 1), (8, 1), (8, 8)]
    cells = [cell(ob("cat", tri), ob("dog", tri), ob(7, tri)), cell(ob("dog", tri), ob("bird", tri))]
    res = tiles_of(cells, [10, 10], [10, 10], tile=10)
    assert res.classes == ["cat", "dog", "bird"]          # first appearance, ids from 0
    assert [t.split()[0] for t in res.tiles["text"].tolist()[0].split("\n")] == ["0", "1"]
    assert res.totals["unmatchable_name_polygons"] == 1 and res.totals["unknown_class"] == 0 and res.totals["selected"] == 4
    res = tiles_of(cells, [10, 10], [10, 10], tile=10, classes=["dog", "cat"])
    assert res.classes == ["dog", "cat"] and res.totals["unknown_class"] == 1
    assert [t.split()[0] for t in "\n".join(res.tiles["text"]).split("\n")] == ["1", "0", "0"]
    res = tiles_of(cells, [10, 10], [10, 10], tile=10, labels=["dog", "dog"])
    assert res.classes == ["dog"] and res.polygons["object"].tolist() == [1, 0]
    with pytest.raises(ValueError):
        tiles_of(cells, [10, 10], [10, 10], classes=["a", "a"])
    with pytest.raises(ValueError):
        tiles_of(cells, [10, 10], [10, 10], labels=["dog"])


def test_a_backend_without_the_entry_is_a_type_error(tmp_path):
    with pytest.raises(TypeError):
        P.yolo_tile_label_texts([BOX], [20], [10], backend=OracleBackend())
    with pytest.raises(TypeError):
        P.tile_yolo_frame(pd.DataFrame({COL: [BOX], "width": [20], "height": [10]}), tmp_path, backend=OracleBackend())
    with pytest.raises(TypeError):
        P.tile_yolo_csv(tmp_path / "x.csv", tmp_path, backend=OracleBackend())


@pytest.mark.parametrize("kw", [dict(tile=0), dict(tile=(10, 2 ** 20 + 1)), dict(tile=10, step=11), dict(tile=10, step=0),
                                dict(tile=10.0), dict(tile=True), dict(overlap=1.0), dict(overlap=-0.1), dict(min_visibility=math.nan),
                                dict(min_visibility=1.5), dict(min_visibility=-0.0001), dict(task="obb"),
                                dict(max_tiles_per_row=0), dict(max_tiles_per_row=2 ** 20 + 1)])
def test_invalid_parameters(kw):
    with pytest.raises(ValueError):
        tiles_of([BOX], [20], [10], **kw)


# ----------------------------------------------------------------------------------------------- files
def _frame(n, seed):
    cells, W, H = random_cells(np.random.default_rng(seed), n)
    return pd.DataFrame({"source": [f"http://host/dir/im {k}.jpg?sig=1" for k in range(n)], COL: cells, "width": W, "height": H,
                         "note": "x"})


def test_csv_route_file_names_and_manifest(tmp_path, monkeypatch):
    df = _frame(40, 5)
    df.loc[3, "width"] = 0
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    kw = dict(tile=32, step=24, min_visibility=0.2, classes=["a", "b", "c"], backend=BE)
    res = P.tile_yolo_csv(src, tmp_path / "n", split="val", lost_csv=tmp_path / "n_lost.csv", **kw)
    assert P.LAST_IO_PATH["tile_yolo"] == "native"
    monkeypatch.setattr(P._fc, "enabled", lambda: False)
    res2 = P.tile_yolo_csv(src, tmp_path / "p", split="val", lost_csv=tmp_path / "p_lost.csv", **kw)
    assert P.LAST_IO_PATH["tile_yolo"] == "pandas"
    strip = ("output_dir", "manifest", "lost_output")
    assert {k: v for k, v in res.items() if k not in strip} == {k: v for k, v in res2.items() if k not in strip}
    names = sorted(p.name for p in (tmp_path / "n" / "labels" / "val").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "p" / "labels" / "val").iterdir()) and len(names) == res["label_files"] > 20
    for nm in names:
        assert (tmp_path / "n" / "labels" / "val" / nm).read_bytes() == (tmp_path / "p" / "labels" / "val" / nm).read_bytes()
    assert (tmp_path / "n" / "tiles_val.csv").read_bytes() == (tmp_path / "p" / "tiles_val.csv").read_bytes()
    assert (tmp_path / "n_lost.csv").read_bytes() == (tmp_path / "p_lost.csv").read_bytes()
    man = pd.read_csv(tmp_path / "n" / "tiles_val.csv", encoding="utf-8-sig", keep_default_na=False)
    assert man.columns.tolist() == ["source", "row", "tile", "x0", "y0", "w", "h", "lines", "status", "label_file", "image_file"]
    assert man[man["row"] == 3][["tile", "status", "label_file"]].values.tolist() == [[-1, "no_size", ""]]
    one = man[(man["lines"] > 0)].iloc[0]
    stem = P._safe_image_stem(df["source"][one["row"]], one["row"])
    assert stem.endswith(f"_{one['row']}") and one["label_file"] == f"labels/val/{stem}__x{one['x0']}_y{one['y0']}.txt"
    assert (man["label_file"] != "").sum() == len(names) and set(man[man["lines"] == 0]["label_file"]) == {""}
    text = (tmp_path / "n" / one["label_file"]).read_text()
    ref = tiles_of(df[COL].tolist(), df["width"].tolist(), df["height"].tolist(), tile=32, step=24, min_visibility=0.2,
                   classes=["a", "b", "c"]).tiles
    assert text == ref[(ref["row"] == one["row"]) & (ref["tile"] == one["tile"])]["text"].item()
    import yaml
    y = yaml.safe_load((tmp_path / "n" / "data.yaml").read_text(encoding="utf-8"))
    assert y["names"] == ["a", "b", "c"] and y["nc"] == 3
    assert res["rows"] == 40 and res["rows_no_size"] == 1 and res["classes"] == ["a", "b", "c"]


def test_csv_error_conventions(tmp_path, capsys):
    assert P.tile_yolo_csv(tmp_path / "nope.csv", tmp_path / "o", backend=BE) is None
    p = tmp_path / "x.csv"
    pd.DataFrame({"a": [1]}).to_csv(p, index=False)
    assert P.tile_yolo_csv(p, tmp_path / "o", backend=BE) is None
    assert f"错误：缺少必要列 {COL}" in capsys.readouterr().out


def test_keep_empty_tiles(tmp_path):
    df = pd.DataFrame({COL: [cell(ob("a", [(1, 1), (8, 1), (8, 8)]))], "width": [30], "height": [10]})
    a = P.tile_yolo_frame(df, tmp_path / "a", tile=10, step=10, backend=BE)
    b = P.tile_yolo_frame(df, tmp_path / "b", tile=10, step=10, keep_empty_tiles=True, backend=BE)
    assert sorted(p.name for p in (tmp_path / "a" / "labels" / "train").iterdir()) == ["img_0__x0_y0.txt"]
    assert sorted(p.name for p in (tmp_path / "b" / "labels" / "train").iterdir()) == \
        ["img_0__x0_y0.txt", "img_0__x10_y0.txt", "img_0__x20_y0.txt"]
    assert (tmp_path / "b" / "labels" / "train" / "img_0__x10_y0.txt").read_text() == ""
    assert (a["label_files"], b["label_files"], a["tiles"], b["tiles"]) == (1, 3, 3, 3)


def test_crops_are_the_tiles_boxes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    px = np.arange(32 * 32 * 3, dtype=np.uint32).reshape(32, 32, 3)
    px = ((px * 7) % 251).astype(np.uint8)
    src = tmp_path / "pic.png"
    Image.fromarray(px).save(src)
    big = cell(ob("a", [(1, 1), (31, 1), (31, 31), (1, 31)]))
    df = pd.DataFrame({"source": [str(src), str(tmp_path / "gone.png")], COL: [big, big], "width": [32, 32], "height": [32, 32]})
    res = P.tile_yolo_frame(df, tmp_path / "ds", tile=20, step=16, crop_images=True, min_visibility=0.0, backend=BE)
    assert res["images_written"] == 4 and res["images_missing"] == 1 and res["label_files"] == 8
    for x0, y0 in ((0, 0), (12, 0), (0, 12), (12, 12)):
        with Image.open(tmp_path / "ds" / "images" / "train" / f"pic_0__x{x0}_y{y0}.png") as im:
            assert np.array_equal(np.asarray(im), px[y0:y0 + 20, x0:x0 + 20])
        assert (tmp_path / "ds" / "labels" / "train" / f"pic_0__x{x0}_y{y0}.txt").exists()
        assert (tmp_path / "ds" / "labels" / "train" / f"gone_1__x{x0}_y{y0}.txt").exists()
    man = pd.read_csv(tmp_path / "ds" / "tiles_train.csv", encoding="utf-8-sig", keep_default_na=False)
    assert man["image_file"].tolist()[:4] == [f"images/train/pic_0__x{x}_y{y}.png" for y in (0, 12) for x in (0, 12)]
    assert man["image_file"].tolist()[4:] == [""] * 4
