"""Label masks (core/processor.py: polygon_masks, export_masks_frame; flatten.mask_rows and the order / batch helpers), host
side, and the K21 rule itself as restated in tests/polygon_raster_ref.py: known answers worked by hand, watertight shared edges,
agreement with exact rational arithmetic, the row rule, argument checks, paint order, instance numbering, value collisions,
batches, and the files written — driven by a test backend whose device stage is the restatement;
tests/test_gpu_polygon_raster.py checks K21 itself.  No GPU."""
import json
import math

import numpy as np
import pandas as pd
import pytest

import polygon_raster_ref as R
from helpers import OracleBackend

from deal_yolo_daya_amd import flatten as fl
from deal_yolo_daya_amd.core import processor as P

COL = P.ANNOTATION_COL


class RasterBackend(OracleBackend):
    def __init__(self):
        self.calls = []

    def rasterize_polygons(self, xy, pt_off, row_off, val, width, height, background=0, max_pixels_per_row=1 << 26):
        out = R.raster_arrays(xy, pt_off, row_off, val, width, height, background, max_pixels_per_row)
        self.calls.append((len(width), int(out[1][-1])))
        return out


def ob(name, pts, **extra):
    return {"name": name, "polygon": {"ptList": [{"x": x, "y": y} for x, y in pts]}, **extra}


def cell(*objs):
    return json.dumps({"objects": list(objs)}, ensure_ascii=False)


def masks_of(cells, widths, heights, **kw):
    return P.polygon_masks(cells, widths, heights, backend=kw.pop("backend", None) or RasterBackend(), **kw)


# ----------------------------------------------------------------------------------------------- the rule
def test_a_box_covers_the_pixels_whose_centres_it_holds():
    c = R.cover([(2, 3), (7, 9)], 12, 12)
    assert c.sum() == 30 and c[3:9, 2:7].all()
    assert R.cover([(7, 9), (2, 3)], 12, 12).sum() == 30                         # the two points in the other order


def test_shared_edges_are_watertight():
    """a quad split along a diagonal: every pixel is in exactly one triangle or in neither, as the quad says, bit for bit"""
    rng = np.random.default_rng(7)
    for trial in range(300):
        c = rng.uniform(4, 28, 2)
        ang = np.sort(rng.uniform(0, 2 * math.pi, 4))
        quad = c + rng.uniform(2, 14, (4, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=1)   # star-shaped: a simple quad
        if trial % 2:
            quad = quad[::-1]
        if trial % 3 == 0:
            quad = np.round(quad * 4) / 4
        s = trial % 4                                                             # the diagonal from vertex s to s + 2
        q = np.roll(quad, -s, axis=0)
        t1, t2 = q[[0, 1, 2]], q[[0, 2, 3]] if trial % 5 else q[[3, 0, 2]]
        assert np.array_equal(R.cover(quad, 32, 32), R.cover(t1, 32, 32) ^ R.cover(t2, 32, 32)), trial


def test_agreement_with_exact_arithmetic_on_a_grid_of_eighths():
    """coordinates in multiples of 1/8: a crossing equals a pixel centre or is at least 2^-15 away, so rounding decides nothing"""
    rng = np.random.default_rng(11)
    for trial in range(40):
        w, h = int(rng.integers(1, 21)), int(rng.integers(1, 19))
        m = int(rng.integers(3, 9))
        pts = rng.integers(-16, 8 * 22, (m, 2)) / 8.0
        assert np.array_equal(R.cover(pts, w, h), R.exact_cover(pts, w, h)), trial


def test_centres_on_edges_and_vertices():
    # vertices on pixel centres: left and top edges are in, right and bottom edges out
    c = R.cover([(1.5, 1.5), (4.5, 1.5), (4.5, 3.5), (1.5, 3.5)], 6, 5)
    want = np.zeros((5, 6), bool)
    want[1:3, 1:4] = True
    assert np.array_equal(c, want)
    # a diamond with its vertices on centres: the left vertex pixel is in, the others out
    d = R.cover([(2.5, 0.5), (4.5, 2.5), (2.5, 4.5), (0.5, 2.5)], 6, 6)
    assert d[2, 0] and not d[2, 4] and not d[4, 2] and d[0, 2] == R.exact_cover([(2.5, 0.5), (4.5, 2.5), (2.5, 4.5), (0.5, 2.5)], 6, 6)[0, 2]
    assert np.array_equal(d, R.exact_cover([(2.5, 0.5), (4.5, 2.5), (2.5, 4.5), (0.5, 2.5)], 6, 6))
    # horizontal edges at yc never cross: the L-shape's step at y = 2.5
    ell = [(0, 0), (6, 0), (6, 2.5), (3, 2.5), (3, 5), (0, 5)]
    assert np.array_equal(R.cover(ell, 6, 5), R.exact_cover(ell, 6, 5)) and R.cover(ell, 6, 5).sum() == 12 + 9


def test_outside_and_huge_polygons():
    assert not R.cover([(-9, -9), (-2, -9), (-2, -3)], 8, 8).any()
    assert not R.cover([(20, 1), (30, 1), (30, 7), (20, 7)], 8, 8).any()          # to the right
    assert R.cover([(-30, 1), (-20, 1), (-20, 7), (-30, 7)], 8, 8).sum() == 0     # to the left: an even number of crossings
    big = 2.0 ** 42
    assert R.cover([(-big, -big), (big, -big), (big, big), (-big, big)], 5, 4).all()
    tri = [(-big, -big), (big, -big), (-big, big)]
    assert np.array_equal(R.cover(tri, 5, 4), R.exact_cover(tri, 5, 4))


def test_every_output_of_the_restatement():
    xy = [2, 3, 7, 9,  0, 0, 10, 0, 10, 10, 0, 10,  1, 1, math.nan, 2, 3, 3,  5, 5,  3, 4, 5, 6,  0, 0, 4, 4]
    pt_off, row_off = [0, 2, 6, 9, 10, 12, 14], [0, 5, 5, 6]
    val = [7, 9, 3, 4, -1, 5]
    status, pix_off, action, covered, owned, pixels = R.raster_arrays(xy, pt_off, row_off, val, [10, 3, 4.5], [10, 2, 4], background=200)
    assert status.tolist() == [0, 0, 2] and pix_off.tolist() == [0, 100, 106, 106]
    assert action.tolist() == [0, 0, 2, 3, 255, 5]
    assert covered.tolist() == [30, 100, 0, 0, 0, 0] and owned.tolist() == [0, 100, 0, 0, 0, 0]     # the box is hidden
    assert (pixels[:100] == 9).all() and (pixels[100:] == 200).all() and pixels.dtype == np.uint8


# ----------------------------------------------------------------------------------------------- the host helpers
def test_mask_rows_against_the_status_rule():
    W = [0, math.nan, 2.5, 10, 10, 11, 200, 3, math.inf, 2.0 ** 43, -4]
    H = [5, 5, 5, 10, 10.5, 10, 1, 200, 5, 5, 5]
    status, pixels = fl.mask_rows(W, H, 100)
    assert status.tolist() == [1, 1, 2, 0, 2, 3, 3, 3, 1, 1, 1] and status.dtype == np.uint8
    assert pixels.tolist() == [0, 0, 0, 100, 0, 0, 0, 0, 0, 0, 0] and pixels.dtype == np.int64
    assert [R.row_size(w, h, 100)[0] for w, h in zip(W, H)] == status.tolist()
    status, pixels = fl.mask_rows([2.0 ** 31, 2.0 ** 42], [2.0 ** 31, 1], 1 << 30)           # nothing overflows
    assert status.tolist() == [3, 3] and pixels.tolist() == [0, 0]
    assert fl.mask_rows([], [], 5)[0].tolist() == []


def test_batches_by_pixels():
    assert fl.mask_batches([5, 5, 5, 20, 1, 1], 10) == [(0, 2), (2, 3), (3, 4), (4, 6)]
    assert fl.mask_batches([0, 0, 0], 1) == [(0, 3)] and fl.mask_batches([], 4) == []
    assert fl.mask_batches([4, 4, 4], 100) == [(0, 3)] and fl.mask_batches([7, 7], 1) == [(0, 1), (1, 2)]
    be = RasterBackend()
    c = cell(ob("a", [(0, 0), (3, 3)]))
    res = masks_of([c] * 5, [4, 4, 10, 4, 4], [4] * 5, batch_pixels=40, backend=be)
    assert be.calls == [(2, 32), (1, 40), (2, 32)]
    one = masks_of([c] * 5, [4, 4, 10, 4, 4], [4] * 5)
    assert all(np.array_equal(a, b) for a, b in zip(res.masks, one.masks)) and res.polygons.equals(one.polygons)
    assert res.totals == one.totals


def test_large_first_permutation_and_its_inverse():
    xy = np.array([0, 0, 1, 1,  0, 0, 5, 5, 2, math.nan,  0, 0, 3, 3,  7, 7, 9, 9,  1, 1, 2, 2], float)
    pt_off, row_off = [0, 2, 5, 5, 7, 9, 11], [0, 4, 6]
    perm = fl.large_first_order(xy, pt_off, row_off)
    assert perm.tolist() == [3, 0, 1, 2, 4, 5]            # areas 1, NaN -> 0, no points -> 0, 9 | 4, 1; ties keep their order
    new_xy, new_off = fl.permute_polygons(xy, pt_off, perm)
    assert new_off.tolist() == [0, 2, 4, 7, 7, 9, 11] and new_off.dtype == np.int32
    assert new_xy[:4].tolist() == [0, 0, 3, 3] and new_xy[4:8].tolist() == [0, 0, 1, 1]
    back = np.argsort(perm)
    old_xy, old_off = fl.permute_polygons(new_xy, new_off, back)
    assert old_off.tolist() == pt_off and np.array_equal(old_xy, xy, equal_nan=True)


def test_paint_order():
    small, large = ob("s", [(3, 3), (5, 5)]), ob("l", [(1, 1), (8, 8)])
    res = masks_of([cell(small, large)], [10], [10], classes=["s", "l"])
    assert res.polygons["result"].tolist() == ["hidden", "painted"] and res.polygons["owned"].tolist() == [0, 49]
    assert res.rows[["polygons", "painted", "hidden", "empty"]].values.tolist() == [[2, 1, 1, 0]]
    res = masks_of([cell(small, large)], [10], [10], classes=["s", "l"], order="large_first")
    assert res.polygons["name"].tolist() == ["s", "l"]    # the tables stay in annotation order
    assert res.polygons["result"].tolist() == ["painted", "painted"] and res.polygons["owned"].tolist() == [4, 45]
    assert res.masks[0][3, 3] == 1 and res.masks[0][1, 1] == 2 and res.masks[0][0, 0] == 0


def test_classes_values_and_collisions():
    c = cell(ob("a", [(0, 0), (2, 2)]), ob("b", [(2, 2), (4, 4)]), ob("zz", [(0, 0), (4, 4)]), ob(5, [(0, 0), (1, 1)]))
    res = masks_of([c], [4], [4], classes=["b", "a"], class_offset=10, background=255)
    assert res.polygons[["name", "class_id", "value"]].values.tolist() == [["a", 1, 11], ["b", 0, 10]]
    assert res.totals["unknown_class"] == 1 and res.totals["unmatchable_name_polygons"] == 1
    assert sorted(np.unique(res.masks[0]).tolist()) == [10, 11, 255]
    assert res.per_class[["class", "value", "polygons", "painted", "pixels"]].values.tolist() == [["b", 10, 1, 1, 4], ["a", 11, 1, 1, 4]]
    assert res.per_class["share"].tolist() == [0.25, 0.25] and res.totals["background_pixels"] == 8
    res = masks_of([c], [4], [4], labels=["b"])
    assert res.polygons["name"].tolist() == ["b"] and res.classes == ["b"]
    with pytest.raises(ValueError, match="background"):
        masks_of([c], [4], [4], classes=["a", "b"], background=2)
    with pytest.raises(ValueError, match="uint8"):
        masks_of([c], [4], [4], classes=["a", "b"], class_offset=255)
    masks_of([c], [4], [4], classes=["a", "b"], class_offset=255, mode="instance")            # instance values do not use it
    be = RasterBackend()
    with pytest.raises(ValueError, match="background"):                                          # by appearance: at the chunk
        masks_of([c], [4], [4], background=3, backend=be)
    assert be.calls == []


def test_instance_numbering_and_a_row_of_256_polygons():
    objs = [ob("a", [(k % 16, k // 16), (k % 16 + 1, k // 16 + 1)]) for k in range(256)]
    cells = [cell(*objs), cell(*objs[:255]), cell(ob("a", [(0, 0), (2, 2)]), ob(7, [(0, 0), (1, 1)]), ob("b", [(1, 1), (3, 3)]))]
    res = masks_of(cells, [16, 16, 4], [16, 16, 4], mode="instance")
    assert res.rows["status"].tolist() == ["too_many_instances", "rasterised", "rasterised"]
    assert res.masks[0] is None and res.masks[1].shape == (16, 16)
    assert res.masks[1].reshape(-1)[:255].tolist() == list(range(1, 256)) and res.masks[1][15, 15] == 0
    first = res.polygons[res.polygons["row"] == 0]
    assert (first["result"] == "too_many_instances").all() and (first["value"] == -1).all() and len(first) == 256
    assert res.polygons[res.polygons["row"] == 2]["value"].tolist() == [1, 2]                   # the unnamed one takes no number
    assert res.masks[2].tolist() == [[1, 1, 0, 0], [1, 2, 2, 0], [0, 2, 2, 0], [0, 0, 0, 0]]
    assert res.totals["rows_too_many_instances"] == 1 and res.totals["pixels"] == 256 + 16 and res.totals["too_many_instances"] == 256


def test_results_per_polygon_and_rows_that_are_not_rasterised():
    c = cell(ob("a", [(0, 0), (4, 4)]), ob("a", [(0.6, 0.6), (0.9, 0.9)]), ob("a", [(1, 1)]), ob("a", [(0, 0), (1e300, 1)]),
             ob("a", [(0, 0), (4, 0), (4, 4), (0, 4)]))
    res = masks_of([c, c, c, "not json"], [4, 0, 4.5, 4], [4, 4, 4, 4], max_pixels_per_row=16)
    assert res.polygons[res.polygons["row"] == 0]["result"].tolist() == ["hidden", "empty", "too_few_points", "bad_coords", "painted"]
    assert res.rows["status"].tolist() == ["rasterised", "no_size", "fractional_size", "rasterised"]
    assert [m is None for m in res.masks] == [False, True, True, False] and not res.masks[3].any()
    assert set(res.polygons[res.polygons["row"] > 0]["result"]) == {"no_raster"}
    res = masks_of([c], [4], [5], max_pixels_per_row=16, keep_masks=False)
    assert res.rows["status"].tolist() == ["too_large"] and res.masks == [None]
    res = masks_of([], [], [])
    assert res.masks == [] and len(res.rows) == 0 and res.totals["pixels"] == 0 and len(res.per_class) == 0


@pytest.mark.parametrize("bad", [dict(mode="panoptic"), dict(order="small_first"), dict(background=256), dict(background=-1),
                                 dict(background=1.0), dict(class_offset=-1), dict(max_pixels_per_row=0),
                                 dict(max_pixels_per_row=2 ** 30 + 1), dict(batch_pixels=0), dict(background=True),
                                 dict(classes=["a", "a"]), dict(labels=["a", "b"])])
def test_argument_validation(bad):
    with pytest.raises(ValueError):
        masks_of([cell(ob("a", [(0, 0), (2, 2)]))], [4], [4], **bad)


def test_a_backend_without_the_entry_and_a_device_that_disagrees():
    with pytest.raises(TypeError, match="rasterize_polygons"):
        P.polygon_masks([], [], [], backend=OracleBackend())

    class Off(RasterBackend):
        def rasterize_polygons(self, *a, **k):
            out = list(super().rasterize_polygons(*a, **k))
            out[0] = out[0] ^ 1
            return out

    with pytest.raises(RuntimeError, match="differ"):
        masks_of([cell(ob("a", [(0, 0), (2, 2)]))], [4], [4], backend=Off())


# ----------------------------------------------------------------------------------------------- the files
def frame():
    cells = [cell(ob("cat", [(1, 1), (6, 1), (6, 5), (1, 5)]), ob("dog", [(4, 3), (9, 7)])),
             cell(ob("dog", [(0, 0), (3, 3)])), cell(), cell(ob("cat", [(0, 0), (2, 2)])),
             cell(ob("cat", [(0, 0), (9, 9)]), ob("dog", [(2, 2), (4, 4)]), ob("dog", [(1, 1)]))]
    return pd.DataFrame({"source": ["http://x/a.jpg", "http://y/a.jpg?k=1", "b.png", "c.png", "dir/d.png"], COL: cells,
                         "width": [10, 4, 5, 3.5, 10], "height": [8, 4, 2, 3, 10]})


@pytest.mark.parametrize("png_mode", ["L", "P"])
def test_export_masks_frame_end_to_end(tmp_path, png_mode):
    from PIL import Image

    df = frame()
    out = tmp_path / "ds"
    stats = {}
    res = P.export_masks_frame(df, out, split="val", classes=["cat", "dog"], png_mode=png_mode, problems_csv=tmp_path / "p.csv",
                               backend=RasterBackend(), stats=stats)
    want = masks_of(df[COL], df["width"], df["height"], classes=["cat", "dog"])
    stems = [P._safe_image_stem(s, i) for i, s in enumerate(df["source"])]
    assert len(set(stems)) == 5 and stems[0] != stems[1]                                        # equal file names, distinct stems
    files = sorted(p.name for p in (out / "masks" / "val").iterdir())
    assert files == sorted(f"{stems[i]}.png" for i in (0, 1, 2, 4))
    for i in (0, 1, 2, 4):
        with Image.open(out / "masks" / "val" / f"{stems[i]}.png") as im:
            assert im.mode == png_mode and np.array_equal(np.asarray(im), want.masks[i])
            if png_mode == "P":
                assert im.getpalette()[:9] == [0, 0, 0, 128, 0, 0, 0, 128, 0]
    assert want.masks[3] is None and not want.masks[2].any()
    manifest = pd.read_csv(out / "masks_val.csv", encoding="utf-8-sig", keep_default_na=False)
    assert manifest.columns.tolist() == ["source", "row", "width", "height", "status", "polygons", "painted", "hidden", "empty", "mask_file"]
    assert manifest["status"].tolist() == ["rasterised", "rasterised", "rasterised", "fractional_size", "rasterised"]
    assert manifest["mask_file"].tolist() == [f"masks/val/{stems[i]}.png" if i != 3 else "" for i in range(5)]
    assert manifest[["polygons", "painted", "hidden", "empty"]].values.tolist() == [[2, 2, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [3, 2, 0, 0]]
    classes = pd.read_csv(out / "mask_classes.csv", encoding="utf-8-sig")
    assert classes.columns.tolist() == ["class", "value", "polygons", "painted", "hidden", "empty", "bad_coords", "too_few_points", "pixels", "share"]
    assert classes["class"].tolist() == ["cat", "dog"] and classes["value"].tolist() == [1, 2]
    cat = int(sum((m == 1).sum() for m in want.masks if m is not None))
    dog = int(sum((m == 2).sum() for m in want.masks if m is not None))
    assert classes["pixels"].tolist() == [cat, dog] and cat > 0 and dog > 0
    assert np.allclose(classes["share"], [cat / 206, dog / 206]) and res["pixels"] == 206
    problems = pd.read_csv(tmp_path / "p.csv", encoding="utf-8-sig")
    assert problems[["row", "object", "result"]].values.tolist() == [[4, 2, "too_few_points"]]
    assert res["mask_files"] == 4 and res["classes"] == ["cat", "dog"] and stats == res
    assert res["paths"]["manifest"] == str(out / "masks_val.csv") and res["paths"]["classes"] == str(out / "mask_classes.csv")


def test_export_leaves_out_empty_masks_on_request_and_reads_a_csv(tmp_path):
    df = frame()
    res = P.export_masks_frame(df, tmp_path / "a", keep_empty_masks=False, backend=RasterBackend())
    assert res["mask_files"] == 3 and not list((tmp_path / "a" / "masks" / "train").glob("b_2*"))
    src = tmp_path / "in.csv"
    df.to_csv(src, index=False, encoding="utf-8-sig")
    res2 = P.export_masks_csv(src, tmp_path / "b", keep_empty_masks=False, backend=RasterBackend())
    strip = ("output_dir", "paths", "python_cells")
    assert {k: v for k, v in res2.items() if k not in strip} == {k: v for k, v in res.items() if k not in strip}
    assert (tmp_path / "a" / "masks_train.csv").read_bytes() == (tmp_path / "b" / "masks_train.csv").read_bytes()
    assert P.export_masks_csv(tmp_path / "none.csv", tmp_path / "c", backend=RasterBackend()) is None
    pd.DataFrame({"source": ["a"]}).to_csv(tmp_path / "nocol.csv", index=False)
    assert P.export_masks_csv(tmp_path / "nocol.csv", tmp_path / "c", backend=RasterBackend()) is None
    with pytest.raises(ValueError, match="png_mode"):
        P.export_masks_frame(df, tmp_path / "d", png_mode="RGB", backend=RasterBackend())


# ----------------------------------------------------------------------------------------------- the mapping
@pytest.mark.parametrize("strip, capacity", [(1024, 256), (17, 3), (64, 1)])
def test_the_kernels_mapping_changes_nothing(strip, capacity):
    """strips, the box cull, the crossing list's flushes and the ownership hand-over of K21, in Python, against the rule"""
    rng = np.random.default_rng(5)
    xy, pt_off, row_off, val, W, H = [], [0], [0], [], [], []
    for _ in range(25):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 24))
        for _ in range(int(rng.integers(0, 6))):
            m = int(rng.integers(1, 80)) if rng.random() < 0.2 else int(rng.integers(2, 9))
            pts = np.stack([rng.uniform(-0.3 * w, 1.3 * w, m), rng.uniform(-0.3 * h, 1.3 * h, m)], axis=1)
            pts = np.round(pts) + (0.5 if rng.random() < 0.3 else 0.0) if rng.random() < 0.5 else pts
            xy += pts.reshape(-1).tolist()
            pt_off.append(pt_off[-1] + m)
            val.append(-1 if rng.random() < 0.1 else int(rng.integers(1, 200)))
        row_off.append(len(val))
        W.append(w if rng.random() > 0.1 else w + 0.5)
        H.append(h)
    t = (np.asarray(xy), np.asarray(pt_off), np.asarray(row_off), np.asarray(val), np.asarray(W, np.float64), np.asarray(H, np.float64))
    want = R.raster_arrays(*t, 250, 4096)
    got = R.paint_by_items(*t, 250, 4096, strip=strip, capacity=capacity)
    assert (want[3] > want[4]).any() and len(want[-1]) > 5000
    for g, w_, what in zip(got, want, ("row_status", "pix_off", "action", "covered", "owned", "pixels")):
        assert np.array_equal(g, w_), what


def _mapping_at_the_defaults(t, background):
    want = R.raster_arrays(*t, background)
    got = R.paint_by_items(*t, background, strip=1024, capacity=256)
    for g, w_, what in zip(got, want, ("row_status", "pix_off", "action", "covered", "owned", "pixels")):
        assert np.array_equal(g, w_), what
    return want


def test_the_mapping_on_full_default_strips():
    """the table of test_gpu_polygon_raster.test_default_strip_widths: rows of 1023, 1024, 1025 and 2049 columns"""
    from test_gpu_polygon_raster import full_strip_rows, table

    want = _mapping_at_the_defaults(table(full_strip_rows()), 5)
    assert (want[3] > 0).all() and (want[4] < want[3]).any() and want[1][-1] == 3 * (1023 + 1024 + 1025 + 2049)


def test_the_mapping_on_more_crossings_than_the_default_list_holds():
    """the table of test_gpu_polygon_raster.test_more_crossings_than_the_default_list_holds: 300 crossings per scanline"""
    from test_gpu_polygon_raster import full_list_rows, table

    want = _mapping_at_the_defaults(table(full_list_rows()), 0)
    assert want[3][0] > 3000 and want[4][0] < want[3][0]
