"""Every `_dev` entry of include/dyd.h on a side stream that is still busy with a delay when the entry is called (the harness
of tests/stream_contract.py): the inputs hold decoys until the delay ends, the outputs are filled with their sentinels when it
ends, so a launch, copy, memset or allocation that strays onto another stream (the null stream, the library's own) gives other
bytes than the reference of the real table.  Exact comparison against the references the steps' own modules use.

ENTRIES maps every entry that takes a stream to the test that runs it and CASES holds the real and the decoy inputs with their
reference; tests/test_stream_contract_cpu.py checks both without a GPU (every entry registered, every decoy a valid table whose
outputs differ from the real table's in every array).  The three interleaving tests at the end put calls on two streams one
right after the other.  Needs a real MI355X."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import box_audit_ref
import box_compare_ref
import box_repair_ref
import coco_ref
import long_tables as LT
import polygon_audit_ref
import polygon_compare_ref
import polygon_raster_ref
import polygon_simplify_ref
import test_gpu_box_audit as k10
import test_gpu_box_compare as k18
import test_gpu_box_repair as k11
import test_gpu_box_suppress as k9
import test_gpu_coco as k16
import test_gpu_polygon_audit as k14
import test_gpu_polygon_compare as k22
import test_gpu_polygon_raster as k21
import test_gpu_polygon_simplify as k19
import test_gpu_tile_labels as k20
import test_gpu_yolo_obb as k17
import test_gpu_yolo_seg as k13
import tile_labels_ref
import yolo_obb_ref
import yolo_seg_ref
from helpers import random_polygons
from oracle import lib as olib
from stream_contract import (Gate, Harness, box_table_decoy, calibrate, moved, other_stream, poly_table_decoy, rev, rev_off, rot_cls,
                             side_stream)
from test_box_suppress_cpu import suppress_rows

pytestmark = pytest.mark.gpu

ENTRIES = {}                   # entry of include/dyd.h that takes a stream -> the name of the test that runs it
CASES = {}                     # entry (or entry:variant) -> function that builds its Case
N_LONG = 2502                  # rows of the long sparse table: the smallest n that keeps the row of 700 polygons (row 2500) apart
                               # from the last row, which the generator gives one polygon (tests/test_stream_contract_cpu.py)
BLOCKING = ("dyd_sync", "dyd_device_status", "dyd_yolo_lines_dev", "dyd_yolo_seg_lines_dev", "dyd_coco_annotations_dev",
            "dyd_yolo_obb_lines_dev", "dyd_yolo_tile_lines_dev", "dyd_rasterize_polygons_dev", "dyd_compare_polygons_dev",
            "dyd_mt19937_permutation_dev", "dyd_split_ids_seeded_dev", "dyd_split_ids_dev", "dyd_split_ids_sharded_dev")


def covers(*entries):
    def mark(fn):
        for e in entries:
            assert e not in ENTRIES, e
            ENTRIES[e] = fn.__name__
        return fn
    return mark


class Case:
    """real / decoy: the entry's device inputs in the order in which its helper arms them; ref(inputs) -> the outputs;
    offsets: positions of offset arrays; classes: position -> n_classes of class-id arrays; may_equal: {output position: why}
    for the one output that a decoy cannot change (checked to be at most one)"""

    def __init__(self, real, decoy, ref, offsets=(), classes=None, may_equal=None):
        self.real, self.decoy, self.ref = tuple(real), tuple(decoy), ref
        self.offsets, self.classes, self.may_equal = offsets, classes or {}, may_equal or {}
        self._want = None

    def want(self):
        if self._want is None:
            self._want = self.ref(self.real)
        return self._want


def case(name):
    return CASES[name]()


def builds(name):
    def mark(fn):
        CASES[name] = functools.lru_cache(maxsize=None)(fn)
        return CASES[name]
    return mark


def eq(got, want):
    """bit equality; NaN where the reference has NaN (the oracle's NaN payload is not the device's)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


@pytest.fixture(scope="module", autouse=True)
def warm(native):
    """the shared scratch and the queue of big rows exist and are large before the first armed call: growing the scratch waits for
    the whole device (csrc/dyd_context.hip), which would hide whether an asynchronous entry returned while its stream was busy"""
    h = np.arange(1 << 21, dtype=np.uint64).reshape(-1, 2)
    native.dedup(h, "first")
    box = np.tile(np.array([[0.0, 0.0, 1.0, 1.0]]), (4, 1))
    native.iou_any_ge(box, np.array([0, 4], np.int32), 2, 0.5)
    units, ms = calibrate()
    side_stream()
    t0 = time.perf_counter()
    yield
    print(f"test_gpu_streams: {time.perf_counter() - t0:.1f} s wall, delay {units} units = {ms:.1f} ms")


def all_pending(hz, entry):
    """an asynchronous entry returns while its stream is still busy; the entries of BLOCKING wait for the stream themselves"""
    assert entry not in BLOCKING
    assert hz.pending and all(hz.pending), f"{entry} waited for its stream"


# =========================================================================================== K1, K2, K12: polygons -> boxes -> flags
def _bigrow_table(seed, big=(300, 1500), mid=(100, 200), n_rows=300):
    """rows of up to 19 boxes with rows above K2_BIG_ROW = 256 boxes (`big`) and rows the sparse kernel defers to the mid list
    (65..256 boxes, `mid`) among them -> (xy, pt_off, box_off)"""
    rng = np.random.default_rng(seed)
    nb = rng.integers(0, 20, size=n_rows)
    where = rng.choice(n_rows, len(big) + len(mid), replace=False)
    nb[where] = list(big) + list(mid)
    box_off = np.zeros(n_rows + 1, np.int32)
    np.cumsum(nb, out=box_off[1:])
    xy, pt_off = random_polygons(rng, int(box_off[-1]), 6, special=False)
    for r in range(n_rows):                                         # the last polygon of a row repeats its first: HIGH rows
        s, e = box_off[r], box_off[r + 1]
        if e - s >= 2 and r % 3 == 0:
            a, b, c, d = pt_off[s], pt_off[s + 1], pt_off[e - 1], pt_off[e]
            k = min(b - a, d - c)
            xy[c:c + k] = xy[a:a + k]
    return xy, pt_off, box_off


@builds("dyd_bbox_minmax_dev")
def _case_k1():
    xy, pt_off, _ = _bigrow_table(1)
    return Case((xy, pt_off), (moved(xy), rev_off(pt_off)), lambda t: olib.bbox_minmax(*t), offsets=(1,))


def _k2_params():
    return ((2, 0.98), (3, 0.5))


@builds("dyd_iou_any_ge_dev")
def _case_k2(seed=1, big=(300, 1500)):
    xy, pt_off, box_off = _bigrow_table(seed, big)
    box = olib.bbox_minmax(xy, pt_off)[0]
    return Case((box, box_off), (moved(box, 4), rev_off(box_off)),
                lambda t: tuple(olib.iou_any_ge(t[0], t[1], mb, thr) for mb, thr in _k2_params()), offsets=(1,))


@builds("dyd_bbox_iou_fused_dev")
def _case_k12(seed=1, big=(300, 1500)):
    xy, pt_off, box_off = _bigrow_table(seed, big)
    return Case((xy, pt_off, box_off), (moved(xy), rev_off(pt_off), rev_off(box_off)),
                lambda t: olib.bbox_iou_chain(*t, 2, 0.98), offsets=(1, 2))


def _k1_dev(native, c, hz):
    import torch

    xy, pt_off = c.real
    B = len(pt_off) - 1
    d_xy, d_po = hz.up(xy, c.decoy[0]), hz.up(pt_off, c.decoy[1])
    arg = hz.out(np.int32, 4 * B, -7)
    box = torch.full((4 * B,), -7.0, dtype=torch.float64, device=d_xy.device)     # 16-byte aligned: no guard element in front
    hz.watch(box)
    native.check(hz.call(native.lib().dyd_bbox_minmax_dev, d_xy.data_ptr(), d_po.data_ptr(), B, len(xy), box.data_ptr(),
                         hz.ptr(arg)), "k1")
    hz.restore()
    return box.cpu().numpy().reshape(B, 4), hz.payload(arg).reshape(B, 4)


@covers("dyd_bbox_minmax_dev")
def test_k1(native):
    c = case("dyd_bbox_minmax_dev")
    hz = Harness()
    box, arg = _k1_dev(native, c, hz)
    obox, oarg = c.want()
    assert np.array_equal(arg, oarg) and eq(box, obox)
    all_pending(hz, "dyd_bbox_minmax_dev")


def _k2_dev(native, c, hz, params=None):
    """dyd_iou_any_ge_dev once per (min_boxes, thr): consecutive calls take the two queues of big rows in turn"""
    box, box_off = c.real
    n = len(box_off) - 1
    d_box, d_off = hz.up(box, c.decoy[0]), hz.up(box_off, c.decoy[1])
    L = native.lib()
    highs = [hz.out(np.uint8, n, 9) for _ in (params or _k2_params())]
    for high, (mb, thr) in zip(highs, params or _k2_params()):
        native.check(hz.call(L.dyd_iou_any_ge_dev, d_box.data_ptr(), d_off.data_ptr(), n, len(box), mb, thr, hz.ptr(high), None), "k2")
        hz.retire(high)
    hz.restore()
    return tuple(hz.payload(h) for h in highs)


@covers("dyd_iou_any_ge_dev")
def test_k2(native):
    c = case("dyd_iou_any_ge_dev")
    counts = np.diff(c.real[1])
    assert (counts > 256).sum() >= 2 and ((counts > 64) & (counts <= 256)).sum() >= 2
    hz = Harness()
    got = _k2_dev(native, c, hz)
    for g, w in zip(got, c.want()):
        assert np.array_equal(g, w)
    assert hz.fired == 2                                           # two calls: both queues of ctx().bigq
    all_pending(hz, "dyd_iou_any_ge_dev")


def _k12_dev(native, c, hz, mb=2, thr=0.98):
    import torch

    xy, pt_off, box_off = c.real
    n, B = len(box_off) - 1, len(pt_off) - 1
    d_xy, d_po, d_bo = (hz.up(a, d) for a, d in zip(c.real, c.decoy))
    box = torch.full((4 * B,), -7.0, dtype=torch.float64, device=d_xy.device)
    hz.watch(box)
    arg, high = hz.out(np.int32, 4 * B, -7), hz.out(np.uint8, n, 9)
    native.check(hz.call(native.lib().dyd_bbox_iou_fused_dev, d_xy.data_ptr(), d_po.data_ptr(), d_bo.data_ptr(), n, B, len(xy), mb,
                         thr, box.data_ptr(), hz.ptr(arg), hz.ptr(high)), "fused")
    hz.restore()
    return box.cpu().numpy().reshape(B, 4), hz.payload(arg).reshape(B, 4), hz.payload(high)


@covers("dyd_bbox_iou_fused_dev")
def test_k12(native):
    c = case("dyd_bbox_iou_fused_dev")
    hz = Harness()
    box, arg, high = _k12_dev(native, c, hz)
    obox, oarg, ohigh = c.want()
    assert np.array_equal(arg, oarg) and eq(box, obox) and np.array_equal(high, ohigh)
    assert 0 < ohigh.sum() < len(ohigh) and (np.diff(c.real[2]) > 256).sum() >= 2
    all_pending(hz, "dyd_bbox_iou_fused_dev")


# =========================================================================================== K9, K10, K11, K18: the box steps
@builds("dyd_suppress_boxes_dev")
def _case_k9(seed=9):
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([[70, 130, 300, 64, 65], rng.integers(0, 40, 200)])
    rng.shuffle(sizes)
    box4, row_off, names = k9._rows_table(sizes, rng, special=True)
    return Case((box4, row_off, names), (moved(box4, 4), rev_off(row_off), rev(names)),
                lambda t: suppress_rows(t[0], t[1], 0.5, t[2]), offsets=(1,))


@covers("dyd_suppress_boxes_dev")
def test_k9(native):
    c = case("dyd_suppress_boxes_dev")
    assert (np.diff(c.real[1]) > 64).sum() >= 3                    # the list of big rows in the shared scratch is not empty
    hz = Harness(c.decoy)
    keep, partner = k9._dev_call(native, c.real[0], c.real[1], 0.5, c.real[2], hz=hz)
    want = c.want()
    assert np.array_equal(keep, want[0]) and np.array_equal(partner, want[1])
    all_pending(hz, "dyd_suppress_boxes_dev")


def _box_table(seed):
    rng = np.random.default_rng(seed)
    return k10._table(np.concatenate([k10.SIZES[:10] + k10.SIZES[11:], rng.integers(0, 40, 300)]), 20, rng)


@builds("dyd_box_audit_dev")
def _case_k10():
    t = _box_table(10)
    return Case(t, box_table_decoy(*t, 20), lambda t: box_audit_ref.audit_arrays(*t, 20, 16), offsets=(1,), classes={2: 20})


@covers("dyd_box_audit_dev")
def test_k10(native):
    c = case("dyd_box_audit_dev")
    hz = Harness(c.decoy)
    k10._same(k10._dev_call(*c.real, 20, 16, hz=hz), c.want())
    all_pending(hz, "dyd_box_audit_dev")


@builds("dyd_repair_boxes_dev")
def _case_k11():
    t = k11._with_edges(_box_table(11), np.random.default_rng(12))
    return Case(t, box_table_decoy(*t, 20), lambda t: box_repair_ref.repair_arrays(*t, 20, 0.5, 4.0), offsets=(1,), classes={2: 20})


@covers("dyd_repair_boxes_dev")
def test_k11(native):
    c = case("dyd_repair_boxes_dev")
    hz = Harness(c.decoy)
    k11._same(k11._dev_call(*c.real, 20, 0.5, 4.0, hz=hz), c.want())
    all_pending(hz, "dyd_repair_boxes_dev")


@builds("dyd_compare_boxes_dev")
def _case_k18(seed=18):
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.asarray([(65, 3), (3, 65), (64, 300), (129, 70), (257, 256), (70, 130)]), rng.integers(0, 40, (30, 2))])
    rng.shuffle(sizes)
    t = k18._tables(sizes, rng)[:6]
    nc = k18.N_CLASSES
    decoy = (moved(t[0], 4), rev_off(t[1]), rot_cls(t[2], nc), moved(t[3], 4), rev_off(t[4]), rot_cls(t[5], nc))
    return Case(t, decoy, lambda t: box_compare_ref.compare_rows(*t, nc, 0.5, False), offsets=(1, 4), classes={2: nc, 5: nc})


@covers("dyd_compare_boxes_dev")
def test_k18(native):
    c = case("dyd_compare_boxes_dev")
    assert (np.diff(c.real[1]) > 64).any() and (np.diff(c.real[4]) > 128).any()      # rows that leave the tile kernel
    hz = Harness(c.decoy)
    box_compare_ref.same_outputs(k18._dev_call(native, *c.real, k18.N_CLASSES, 0.5, False, hz=hz), c.want(), "delayed stream")
    all_pending(hz, "dyd_compare_boxes_dev")


# =========================================================================================== K3, K4, K5: hashes and key tables
def _cells(seed, n=3000, distinct=1000):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, distinct, n)
    cells = [b"http://img.example/%d.jpg" % k * (1 + k % 3) for k in ids.tolist()]
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(c) for c in cells], out=off[1:])
    return np.frombuffer(b"".join(cells), np.uint8).copy(), off


@builds("dyd_hash128_dev")
def _case_k3():
    data, off = _cells(3)
    return Case((data, off), (rev(data), rev_off(off)), lambda t: (olib.hash128(*t),), offsets=(1,))


def _keys(seed):
    return np.ascontiguousarray(olib.hash128(*_cells(seed)), np.uint64).reshape(-1, 2)


@builds("dyd_dedup_dev")
def _case_k4():
    h = _keys(4)
    return Case((h,), (rev(h),), lambda t: tuple(olib.dedup(t[0], mode) for mode in (0, 1, 2)))


@builds("dyd_isin_dev")
def _case_k5():
    h, ref_h = _keys(4), _keys(5)[:700]
    return Case((h, ref_h), (rev(h), rev(ref_h)), lambda t: (olib.isin(t[0], t[1]),))


GLOBAL_SHARD = (1000, 800)                                           # first_global, n_local


@builds("dyd_dedup_global_dev")
def _case_k4_global():
    h = _keys(6)
    lo, m = GLOBAL_SHARD
    return Case((h,), (rev(h),), lambda t: tuple(olib.dedup(t[0], mode)[lo:lo + m] for mode in (0, 1, 2)))


def _hash_dev(native, c, hz):
    data, off = c.real
    n = len(off) - 1
    d_data, d_off = hz.up(data, c.decoy[0]), hz.up(off, c.decoy[1])
    out = hz.out(np.uint64, 2 * n, 0xDEADBEEF12345678)
    native.check(hz.call(native.lib().dyd_hash128_dev, d_data.data_ptr(), d_off.data_ptr(), n, hz.ptr(out)), "k3")
    hz.restore()
    return hz.payload(out)


def _dedup_dev(native, h, decoy, hz, modes=(0, 1, 2), shard=None):
    """dyd_dedup_dev (or dyd_dedup_global_dev on `shard`) per keep mode, then dyd_device_status on the same stream"""
    n = len(h)
    d_h = hz.up(h, decoy)
    L = native.lib()
    keeps = [hz.out(np.uint8, shard[1] if shard else n, 7) for _ in modes]
    for keep, mode in zip(keeps, modes):
        if shard:
            rc = hz.call(L.dyd_dedup_global_dev, d_h.data_ptr(), n, shard[0], shard[1], mode, hz.ptr(keep))
        else:
            rc = hz.call(L.dyd_dedup_dev, d_h.data_ptr(), n, mode, hz.ptr(keep))
        native.check(rc, "k4")
        hz.retire(keep)
    assert L.dyd_device_status(C.c_void_p(hz.s.cuda_stream)) == 0, L.dyd_last_error()
    status_waited = hz.s.query()
    hz.restore()
    return tuple(hz.payload(k) for k in keeps), status_waited


@covers("dyd_hash128_dev")
def test_k3(native):
    c = case("dyd_hash128_dev")
    hz = Harness()
    got = _hash_dev(native, c, hz)
    assert np.array_equal(got.reshape(-1, 2), np.asarray(c.want()[0], np.uint64).reshape(-1, 2))
    all_pending(hz, "dyd_hash128_dev")


@covers("dyd_dedup_dev", "dyd_device_status")
def test_k4_every_keep_mode_then_the_status_word(native):
    c = case("dyd_dedup_dev")
    hz = Harness()
    got, status_waited = _dedup_dev(native, c.real[0], c.decoy[0], hz)
    for g, w in zip(got, c.want()):
        assert np.array_equal(g, w) and 0 < w.sum() < len(w)
    all_pending(hz, "dyd_dedup_dev")
    assert status_waited                                           # dyd_device_status returns when the stream has finished


@covers("dyd_isin_dev")
def test_k5(native):
    c = case("dyd_isin_dev")
    hz = Harness()
    h, ref_h = c.real
    d_h, d_r = hz.up(h, c.decoy[0]), hz.up(ref_h, c.decoy[1])
    mask = hz.out(np.uint8, len(h), 7)
    L = native.lib()
    native.check(hz.call(L.dyd_isin_dev, d_h.data_ptr(), len(h), d_r.data_ptr(), len(ref_h), hz.ptr(mask)), "k5")
    assert L.dyd_device_status(C.c_void_p(hz.s.cuda_stream)) == 0, L.dyd_last_error()
    hz.restore()
    want = c.want()[0]
    assert np.array_equal(hz.payload(mask), want) and 0 < want.sum() < len(want)
    all_pending(hz, "dyd_isin_dev")


@covers("dyd_dedup_global_dev")
def test_k4_global(native):
    c = case("dyd_dedup_global_dev")
    hz = Harness()
    got, _ = _dedup_dev(native, c.real[0], c.decoy[0], hz, shard=GLOBAL_SHARD)
    for g, w in zip(got, c.want()):
        assert np.array_equal(g, w)
    all_pending(hz, "dyd_dedup_global_dev")


# =========================================================================================== K6, K8: the split
def _split_inputs(seed, n, p):
    """cat in -1 .. len(p) - 2 drawn with the shares p -> (cat, sizes, cat_off, n_train, n_val)"""
    rng = np.random.default_rng(seed)
    n_cat = len(p) - 1
    cat = rng.choice(np.arange(-1, n_cat), size=n, p=p).astype(np.int32)
    sizes = np.bincount(cat[cat >= 0], minlength=n_cat).astype(np.int64)
    off = np.zeros(n_cat + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    return cat, sizes, off, (sizes * 0.8).astype(np.int64), (sizes * 0.1).astype(np.int64)


def _perms(seed, sizes):
    return np.concatenate([np.random.RandomState(seed).permutation(int(s)) for s in sizes]).astype(np.int64)


def _mirror(perm, sizes):
    """every category's permutation mirrored (size - 1 - p): still a permutation of the category"""
    return np.concatenate([s - 1 - perm[o:o + s] for o, s in zip(np.cumsum(sizes) - sizes, sizes)]).astype(np.int64)


SPLIT_SHARD = (5000, 12000)
SEEDED = (8, 60000, (0.05, 0.6, 0.25, 0.1))


@builds("dyd_split_ids_dev")
def _case_k6():
    cat, sizes, off, tr, va = _split_inputs(6, 20000, [0.1, 0.4, 0.3, 0.15, 0.05])
    perm = _perms(7, sizes)
    # cat_off stays: it holds the categories' sizes, and the reversed `cat` has the same ones (a table with other sizes would
    # send a kernel that mixes real and decoy arrays past the end of the permutation)
    return Case((cat, perm, off, tr, va), (rev(cat), _mirror(perm, sizes), off, va, tr), lambda t: olib.split_ids(*t), offsets=(2,))


@builds("dyd_split_ids_sharded_dev")
def _case_k6_sharded():
    cat, sizes, off, tr, va = _split_inputs(6, 20000, [0.1, 0.4, 0.3, 0.15, 0.05])
    perm = _perms(7, sizes)
    lo, hi = SPLIT_SHARD
    count = lambda a: np.bincount(a[a >= 0], minlength=len(sizes)).astype(np.int64)      # noqa: E731
    base, here = count(cat[:lo]), count(cat[lo:hi])

    def ref(t):
        """the shard's rows of the split of the whole table: the rows before the shard are any rows with `base` members per
        category, the shard's own come next"""
        shard, p, o, a, b, rank_base = t
        before = np.repeat(np.arange(len(rank_base), dtype=np.int32), rank_base)
        s, pos = olib.split_ids(np.concatenate([before, shard]), p, o, a, b)
        return s[len(before):], pos[len(before):]

    return Case((cat[lo:hi], perm, off, tr, va, base), (rev(cat[lo:hi]), _mirror(perm, sizes), off, va, tr, sizes - base - here), ref,
                offsets=(2,))


@builds("dyd_split_ids_seeded_dev")
def _case_k6_seeded():
    cat, sizes, off, tr, va = _split_inputs(*SEEDED)
    assert sizes[0] >= 1 << 15 > sizes[1]                          # one category through K8 on the device, the others by the host loop

    def ref(t):
        return olib.split_ids(t[0], _perms(42, sizes), off, tr, va)

    return Case((cat,), (rev(cat),), ref)


def _split_dev(native, c, hz, entry):
    """the three device entries of the split; the seeded one takes its sizes and cuts as host arrays, which are not armed"""
    ins = [hz.up(a, d) for a, d in zip(c.real, c.decoy)]
    n = len(c.real[0])
    split, pos = hz.out(np.uint8, n, 77), hz.out(np.int64, n, -7)
    L, p = native.lib(), [t.data_ptr() for t in ins]
    if entry == "dyd_split_ids_seeded_dev":
        _, sizes, _, tr, va = _split_inputs(*SEEDED)
        rc = hz.call(L.dyd_split_ids_seeded_dev, p[0], n, 42, sizes.ctypes.data, tr.ctypes.data, va.ctypes.data, len(sizes),
                     None, hz.ptr(split), hz.ptr(pos))
    elif entry == "dyd_split_ids_sharded_dev":
        rc = hz.call(L.dyd_split_ids_sharded_dev, p[0], n, *p[1:5], len(c.real[2]) - 1, p[5], hz.ptr(split), hz.ptr(pos))
    else:
        rc = hz.call(L.dyd_split_ids_dev, p[0], n, *p[1:5], len(c.real[2]) - 1, hz.ptr(split), hz.ptr(pos))
    native.check(rc, entry)
    hz.restore()
    return hz.payload(split), hz.payload(pos)


@pytest.mark.parametrize("entry", ["dyd_split_ids_dev", "dyd_split_ids_sharded_dev", "dyd_split_ids_seeded_dev"])
def test_k6(native, entry):
    c = case(entry)
    split, pos = _split_dev(native, c, Harness(), entry)
    want = c.want()
    assert np.array_equal(split, want[0]) and np.array_equal(pos, want[1]) and {0, 1, 2, 255} <= set(want[0].tolist())


for _e in ("dyd_split_ids_dev", "dyd_split_ids_sharded_dev", "dyd_split_ids_seeded_dev"):
    ENTRIES[_e] = "test_k6"


def _perm_dev(native, n, hz, seed=42):
    perm, inv = hz.out(np.int64, n, -7), hz.out(np.int64, n, -7)
    native.check(hz.call(native.lib().dyd_mt19937_permutation_dev, seed, n, hz.ptr(perm), hz.ptr(inv)), "k8")
    hz.restore()
    return hz.payload(perm), hz.payload(inv)


@covers("dyd_mt19937_permutation_dev")
@pytest.mark.parametrize("n", [65_537, 1_000_003])
def test_k8(native, n):
    """no device input: only the delayed sentinels apply"""
    perm, inv = _perm_dev(native, n, Harness())
    want = np.random.RandomState(42).permutation(n).astype(np.int64)
    assert np.array_equal(perm, want)
    assert np.array_equal(inv[want], np.arange(n))


# =========================================================================================== K7: label lines
def _k7_table(seed):
    """3000 rows of up to 4 boxes: a dozen of the box kernel's tiles of 480 boxes, three of the row kernels' tiles of 1024 rows"""
    import test_gpu_yolo as k7

    return k7._random_case(np.random.default_rng(seed), 3000, 4, True, special=False)


@builds("dyd_yolo_lines_dev")
def _case_k7_rows():
    box, _, sel, w, h, cid = _k7_table(70)                          # some 6,000 boxes: the first 3,000, one to a row
    n = len(w)
    t = (box[:n].copy(), np.arange(n + 1, dtype=np.int32), sel[:n].copy(), w, h, cid)
    decoy = (moved(t[0], 4), t[1], rev(t[2]), rev(t[3]), rev(t[4]), rev(t[5]))
    # row_off stays: with one box per row its reverse is itself
    return Case(t, decoy, lambda t: olib.yolo_lines(*t), offsets=(1,))


@builds("dyd_yolo_lines_dev:by_box")
def _case_k7_boxes():
    t = _k7_table(71)
    decoy = (moved(t[0], 4), rev_off(t[1]), rev(t[2]), rev(t[3]), rev(t[4]), rev(t[5]))
    return Case(t, decoy, lambda t: olib.yolo_lines(*t), offsets=(1,))


def _k7_dev(native, c, hz):
    """the two calls of dyd_yolo_lines_dev: measure, then print into a buffer of that size; armed anew for each"""
    import torch

    box4, row_off, sel, w, h, cid = c.real
    n, nb = len(row_off) - 1, len(box4)
    ins = [hz.up(a, d) for a, d in zip(c.real, c.decoy)]
    toff, flag = hz.out(np.int64, n + 1, -7), hz.out(np.uint8, n, 9)
    total = C.c_int64(-1)
    L = native.lib()
    args = (*(t.data_ptr() for t in ins), n, nb, hz.ptr(toff), hz.ptr(flag))
    native.check(hz.call(L.dyd_yolo_lines_dev, *args, None, 0, C.byref(total)), "measure")
    T = total.value
    text = torch.full((T + 64,), 0xAB, dtype=torch.uint8, device=ins[0].device)
    hz.watch(text)
    native.check(hz.call(L.dyd_yolo_lines_dev, *args, text.data_ptr() + 32, T, C.byref(total)), "print")
    hz.restore()
    b = text.cpu().numpy()
    assert total.value == T and (b[:32] == 0xAB).all() and (b[32 + T:] == 0xAB).all()
    return hz.payload(toff), hz.payload(flag), b[32:32 + T].tobytes()


@covers("dyd_yolo_lines_dev")
@pytest.mark.parametrize("layout", ["rows", "by_box"])
def test_k7(native, layout):
    c = case("dyd_yolo_lines_dev" if layout == "rows" else "dyd_yolo_lines_dev:by_box")
    L = native.lib()
    native.check(L.dyd_set_option(b"k7_variant", 22 if layout == "rows" else 30), "opt")
    try:
        hz = Harness()
        off, flag, text = _k7_dev(native, c, hz)
    finally:
        native.check(L.dyd_set_option(b"k7_variant", -1), "opt")
    ooff, oflag, otext = c.want()
    assert np.array_equal(off, ooff) and np.array_equal(flag, oflag) and text == otext
    assert hz.fired == 2 and len(otext) > 3 * 480 * 20 and {0, 1} <= set(oflag.tolist())


# =========================================================================================== the polygon steps on the long table
def _long(seed=0):
    return LT.long_sparse(seed, N_LONG)


def _poly(extra_real, extra_decoy, ref, classes=None, seed=0):
    """the long table with a step's own columns: (xy, pt_off, row_off, *extra[:1], W, H, *extra[1:])"""
    xy, pt_off, row_off, W, H = _long(seed)
    dxy, dpt, drow, dW, dH = poly_table_decoy(xy, pt_off, row_off, W, H)
    real = (xy, pt_off, row_off, extra_real[0], W, H, *extra_real[1:])
    decoy = (dxy, dpt, drow, extra_decoy[0], dW, dH, *extra_decoy[1:])
    return Case(real, decoy, ref, offsets=(1, 2), classes=classes)


def _nb():
    return len(_long()[1]) - 1


@builds("dyd_yolo_seg_lines_dev")
def _case_k13():
    sel, cid = LT.k13_sel(_nb()), LT.class_ids(N_LONG)
    return _poly((sel, cid), (rev(sel), rev(cid)), lambda t: yolo_seg_ref.seg_arrays(*t))


@builds("dyd_yolo_obb_lines_dev")
def _case_k17():
    sel, cid = LT.k13_sel(_nb()), LT.class_ids(N_LONG)
    return _poly((sel, cid), (rev(sel), rev(cid)), lambda t: yolo_obb_ref.obb_arrays(*t))


@builds("dyd_audit_polygons_dev")
def _case_k14():
    cls = LT.k14_cls(_nb())
    W, H = _long()[3:]
    st = LT.size_status(W, H)
    return _poly((cls, st), (rot_cls(cls, 4), rev(st)), lambda t: polygon_audit_ref.audit_arrays(*t, 4), classes={3: 4})


@builds("dyd_coco_annotations_dev")
def _case_k16():
    cat = LT.k16_cat(_nb())
    W, H = _long()[3:]
    st = LT.size_status(W, H)
    return _poly((cat, st), (rot_cls(cat, 4), rev(st)), lambda t: coco_ref.coco_arrays(*t, 1, 1, 1), classes={3: 4})


@builds("dyd_yolo_tile_lines_dev")
def _case_k20():
    cls = LT.k20_cls(_nb())
    return _poly((cls,), (rev(cls),), lambda t: tile_labels_ref.tile_arrays(*t, *LT.k20_params()), classes={3: 101})


@builds("dyd_rasterize_polygons_dev")
def _case_k21():
    val = LT.k21_val(_nb())
    return _poly((val,), (rev(val),), lambda t: polygon_raster_ref.raster_arrays(*t, 9, 1 << 20), classes={3: 201})


K22 = dict(n_classes=3, thr=0.5, by_label=False, max_pixels_per_row=1 << 20, max_pairs_per_row=1 << 20)


@builds("dyd_compare_polygons_dev")
def _case_k22():
    a, b = _long(0), _long(1)
    cls = (np.arange(_nb()) % 4 - 1).astype(np.int32)
    b_cls = (np.arange(_nb()) % 3).astype(np.int32)
    da, db = poly_table_decoy(*a), poly_table_decoy(*b)
    real = (a[0], a[1], a[2], cls, b[0], b[1], b[2], b_cls, a[3], a[4])
    decoy = (da[0], da[1], da[2], rot_cls(cls, 3), db[0], db[1], db[2], rot_cls(b_cls, 3), da[3], da[4])
    return Case(real, decoy, lambda t: polygon_compare_ref.compare_arrays(*t, **K22), offsets=(1, 2, 5, 6), classes={3: 3, 7: 3})


@covers("dyd_yolo_seg_lines_dev")
def test_k13(native):
    c = case("dyd_yolo_seg_lines_dev")
    hz = Harness(c.decoy)
    got = k13.check_dev(*c.real, hz=hz)
    want = c.want()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[3] == want[3] and hz.fired == 3


@covers("dyd_yolo_obb_lines_dev")
def test_k17(native):
    c = case("dyd_yolo_obb_lines_dev")
    hz = Harness(c.decoy)
    k17.same(k17.check_dev(*c.real, hz=hz), c.want())
    assert hz.fired == 3


@covers("dyd_audit_polygons_dev")
def test_k14(native):
    c = case("dyd_audit_polygons_dev")
    hz = Harness(c.decoy)
    k14.same(k14.run_dev((*c.real, 4), hz=hz), c.want())
    all_pending(hz, "dyd_audit_polygons_dev")


@covers("dyd_coco_annotations_dev")
def test_k16(native):
    c = case("dyd_coco_annotations_dev")
    hz = Harness(c.decoy)
    k16.same(k16.run_dev(c.real, hz=hz), c.want())
    assert hz.fired == 3


@covers("dyd_yolo_tile_lines_dev")
def test_k20(native):
    c = case("dyd_yolo_tile_lines_dev")
    hz = Harness(c.decoy)
    got, rc, total = k20.run_dev(c.real, LT.k20_params(), hz=hz)
    assert rc == 0 and total == len(c.want()[-1])
    k20.same(got, c.want())
    assert hz.fired == 2


@covers("dyd_rasterize_polygons_dev")
def test_k21(native):
    c = case("dyd_rasterize_polygons_dev")
    hz = Harness(c.decoy)
    got, rc, total = k21.run_dev(c.real, 9, 1 << 20, hz=hz)
    assert rc == 0 and total == len(c.want()[-1])
    k21.same(got, c.want())
    assert hz.fired == 2


@covers("dyd_compare_polygons_dev")
@pytest.mark.parametrize("pairs", ["own", "null"])
def test_k22(native, pairs):
    c = case("dyd_compare_polygons_dev")
    want = c.want()
    hz = Harness(c.decoy)
    got, rc = k22.run_dev(c.real, pairs=pairs, n_pairs=want[1][-1], hz=hz, **K22)
    assert rc == 0, native.lib().dyd_last_error()
    k22.same(got[:15], want[:15])
    if pairs == "own":
        k22.same(got[15:], want[15:], k22.NAMES[15:])
        assert len(want[15]) > 700 * 700


# =========================================================================================== K19: one polygon per tier
@builds("dyd_simplify_polygons_dev")
def _case_k19():
    rng = np.random.default_rng(19)
    polys = []
    for m in (20, 500, 1500):                                       # a lane, a workgroup's LDS, the queues in global memory
        a = np.linspace(0, 2 * np.pi, m, endpoint=False)
        r = 200 + 30 * np.sin(7 * a) + rng.uniform(-3, 3, m)
        polys.append(np.stack([400.25 + r * np.cos(a), 300.75 + r * np.sin(a)], 1))
    xy = np.concatenate(polys).reshape(-1)
    pt_off = np.asarray([0, 20, 520, 2020], np.int32)
    decoy = moved(xy)
    decoy[7] = 2.0 ** 44                                            # beyond the step's limit: another action code for that polygon
    return Case((xy, pt_off), (decoy, rev_off(pt_off)), lambda t: polygon_simplify_ref.simplify_arrays(*t, 2.5), offsets=(1,))


@covers("dyd_simplify_polygons_dev")
def test_k19(native):
    c = case("dyd_simplify_polygons_dev")
    counts = np.diff(c.real[1])
    assert counts[0] <= k19.LANE_POINTS < counts[1] <= k19.LDS_POINTS < counts[2] and (c.real[0] != np.round(c.real[0])).all()
    hz = Harness(c.decoy)
    k19.same(k19.run_dev(*c.real, 2.5, hz=hz), c.want())
    all_pending(hz, "dyd_simplify_polygons_dev")


# =========================================================================================== membench and dyd_sync
@covers("dyd_membench_dev")
def test_membench_copy(native):
    import torch

    rng = np.random.default_rng(0)
    real, decoy = rng.integers(0, 256, 1 << 20).astype(np.uint8), rng.integers(0, 256, 1 << 20).astype(np.uint8)
    hz = Harness()
    src = hz.up(real, decoy)
    dst = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=src.device)
    hz.watch(dst)
    native.check(hz.call(native.lib().dyd_membench_dev, 0, src.data_ptr(), dst.data_ptr(), 1 << 20, 64), "membench")
    hz.restore()
    assert np.array_equal(dst.cpu().numpy(), real)
    all_pending(hz, "dyd_membench_dev")


@covers("dyd_sync")
def test_sync_returns_after_the_delay(native):
    hz = Harness()
    sp = hz.fire()                                                 # asserts that the stream is busy
    assert native.lib().dyd_sync(C.c_void_p(sp)) == 0
    assert hz.s.query()


# =========================================================================================== the harness itself
def test_the_harness_detects_a_wrong_stream(native):
    """the switch hands the entry the null stream while `s` is armed as always: an entry that reads its input (K1) works on the
    decoy and has its outputs overwritten by the delayed fill, the permutation only the latter — both must come out unequal"""
    c = case("dyd_bbox_minmax_dev")
    hz = Harness(wrong_stream=True)
    box, arg = _k1_dev(native, c, hz)
    obox, oarg = c.want()
    assert not np.array_equal(arg, oarg) and not eq(box, obox)
    assert (arg == -7).all(), "the delayed fill came last"
    perm, inv = _perm_dev(native, 65_537, Harness(wrong_stream=True))
    assert not np.array_equal(perm, np.random.RandomState(42).permutation(65_537)) and (perm == -7).all()
    box, arg = _k1_dev(native, c, Harness())                       # and the same call on the right stream
    assert np.array_equal(arg, oarg) and eq(box, obox)


# =========================================================================================== calls on two streams, interleaved
def _side_streams():
    a = side_stream()
    return a, other_stream(a)


def test_the_scratch_goes_from_stream_to_stream(native):
    """K18 on A (behind the delay), K9 on B, K7 on A, K4 on B, K22 on A, K13 on B, each called as soon as the one before has
    returned; all of them keep state in the one scratch buffer of the context (csrc/dyd_context.hip).  Catches gross errors
    only — contents the other stream's step left in the scratch, a step that does not wait for the scratch's last user and
    meets it every time; it cannot prove that no race exists."""
    A, B = _side_streams()
    gate = Gate()
    on = lambda s: Harness(stream=s, delay=False, sync=False, gate=gate)      # noqa: E731
    c18, c9, c7, c4, c22, c13 = (case(k) for k in ("dyd_compare_boxes_dev", "dyd_suppress_boxes_dev", "dyd_yolo_lines_dev:by_box",
                                                   "dyd_dedup_dev", "dyd_compare_polygons_dev", "dyd_yolo_seg_lines_dev"))
    for c in (c18, c9, c7, c4, c22, c13):
        c.want()                                                   # the references first: no host work between the calls
    n_pairs = c22.want()[1][-1]
    with gate:
        jobs = [gate.start(k18._dev_call, native, *c18.real, k18.N_CLASSES, 0.5, False, hz=Harness(c18.decoy, stream=A, gate=gate)),
                gate.start(k9._dev_call, native, c9.real[0], c9.real[1], 0.5, c9.real[2], hz=on(B)),
                gate.start(_k7_dev, native, c7, on(A)),
                gate.start(_dedup_dev, native, c4.real[0], None, on(B)),
                gate.start(k22.run_dev, c22.real, n_pairs=n_pairs, hz=on(A), **K22),
                gate.start(k13.check_dev, *c13.real, hz=on(B))]
    got = [gate.result(j) for j in jobs]
    box_compare_ref.same_outputs(got[0], c18.want(), "K18 on A")
    assert np.array_equal(got[1][0], c9.want()[0]) and np.array_equal(got[1][1], c9.want()[1])
    assert np.array_equal(got[2][0], c7.want()[0]) and np.array_equal(got[2][1], c7.want()[1]) and got[2][2] == c7.want()[2]
    for g, w in zip(got[3][0], c4.want()):
        assert np.array_equal(g, w)
    assert got[4][1] == 0
    k22.same(got[4][0], c22.want())
    w13 = c13.want()
    assert all(np.array_equal(g, w) for g, w in zip(got[5][:3], w13[:3])) and got[5][3] == w13[3]


BIG_ROWS = (0, 3, 1, 5, 0, 2)


def _bigq_case(k, fused):
    big = tuple(257 + 40 * j for j in range(BIG_ROWS[k]))
    return (_case_k12 if fused else _case_k2)(seed=20 + k, big=big)


def test_the_queue_of_big_rows_goes_from_stream_to_stream(native):
    """dyd_bbox_iou_fused_dev and dyd_iou_any_ge_dev in turn on A, B, A, B, B, A with 0, 3, 1, 5, 0 and 2 rows above 256 boxes:
    the two queues of ctx().bigq alternate and every call's drain kernel empties the other one.  Catches gross errors only —
    rows the other stream's call left in a queue; it cannot prove that no race exists."""
    A, B = _side_streams()
    gate = Gate()
    cases = [_bigq_case(k, fused=k % 2 == 0) for k in range(6)]
    for k, c in enumerate(cases):
        c.want()
        assert (np.diff(c.real[-1]) > 256).sum() == BIG_ROWS[k]
    jobs = []
    with gate:
        for k, (c, s) in enumerate(zip(cases, (A, B, A, B, B, A))):
            hz = Harness(stream=s, gate=gate) if k == 0 else Harness(stream=s, delay=False, sync=False, gate=gate)
            jobs.append(gate.start(_k12_dev, native, c, hz) if k % 2 == 0 else gate.start(_k2_dev, native, c, hz, ((2, 0.98),)))
    wrong = []                                                     # every call is looked at: which of them differ tells more than the first
    for k, (c, j) in enumerate(zip(cases, jobs)):
        try:
            got = gate.result(j)
        except AssertionError as e:
            wrong.append((k, str(e)))
            continue
        if k % 2 == 0:
            obox, oarg, ohigh = c.want()
            if not (np.array_equal(got[1], oarg) and eq(got[0], obox) and np.array_equal(got[2], ohigh)):
                wrong.append((k, "fused outputs differ"))
        elif not np.array_equal(got[0], c.want()[0]):
            wrong.append((k, "flags differ"))
    assert not wrong, wrong


def test_a_host_call_between_two_device_calls(native):
    """K9 on A behind the delay, then the host-pointer dyd_dedup (the library's own stream, the same scratch) while A is still
    busy, then K18 on A.  Catches gross errors only; it cannot prove that no race exists."""
    A, _ = _side_streams()
    gate = Gate()
    c9, c4, c18 = case("dyd_suppress_boxes_dev"), case("dyd_dedup_dev"), case("dyd_compare_boxes_dev")
    for c in (c9, c4, c18):
        c.want()
    first = Harness(c9.decoy, stream=A, gate=gate)
    with gate:
        j9 = gate.start(k9._dev_call, native, c9.real[0], c9.real[1], 0.5, c9.real[2], hz=first)
        pending = list(first.pending)
        host = native.dedup(c4.real[0], "first")
        j18 = gate.start(k18._dev_call, native, *c18.real, k18.N_CLASSES, 0.5, False,
                         hz=Harness(stream=A, delay=False, sync=False, gate=gate))
    assert pending == [True]                                       # A was busy when the host call began
    assert np.array_equal(np.asarray(host).astype(np.uint8), c4.want()[0])
    keep, partner = gate.result(j9)
    assert np.array_equal(keep, c9.want()[0]) and np.array_equal(partner, c9.want()[1])
    box_compare_ref.same_outputs(gate.result(j18), c18.want(), "K18 on A after the host call")
