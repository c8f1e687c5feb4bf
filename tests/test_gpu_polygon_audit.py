"""K14 (polygon audit, csrc/k14_poly_audit.hip) through both C-ABI entries and audit_polygons_csv, against the restatement in
tests/polygon_audit_ref.py.  Bit-exact.  Needs a real MI355X."""
import math

import numpy as np
import pandas as pd
import pytest

import polygon_audit_ref as R
import yolo_seg_ref as S
from test_polygon_audit_cpu import BE, _table
from deal_yolo_daya_amd import synth
from deal_yolo_daya_amd.core import processor as P

pytestmark = pytest.mark.gpu

LANE_EDGES = 64                  # K14_LANE_EDGES: above it the wave tier decides self_intersecting


def random_table(rng, n_rows, n_classes=7, max_polys=6, max_pts=45):
    """small integer grids (many crossings, repeats, collinear edges) with special values and sizes"""
    xy, pt_off, row_off = [], [0], [0]
    W = rng.choice([40.0, 25.0, 100.0, 17.5], size=n_rows)
    H = rng.choice([40.0, 30.0, 100.0], size=n_rows)
    st = rng.choice([0, 0, 0, 0, 1, 2], size=n_rows).astype(np.uint8)
    k = rng.integers(0, n_rows, size=max(1, n_rows // 15))
    W[k[::2]] = rng.choice([np.nan, -1.0, 0.0, np.inf, 2.0 ** 43, -0.0], size=len(k[::2]))
    H[k[1::2]] = rng.choice([np.nan, -5.0, 0.0, 2.0 ** 43], size=len(k[1::2]))
    cls = []
    for i in range(n_rows):
        for _ in range(int(rng.integers(0, max_polys + 1))):
            n = int(rng.integers(0, max_pts + 1)) if rng.random() < 0.3 else int(rng.integers(0, 9))
            span = rng.choice([10, 30, 60])
            pts = rng.integers(-5, span, size=(n, 2)).astype(np.float64)
            if n and rng.random() < 0.3:
                j = rng.integers(0, n)
                pts[j] = pts[j - 1]                                       # a repeat (cyclic)
            if n and rng.random() < 0.08:
                pts[rng.integers(0, n), rng.integers(0, 2)] = rng.choice([np.nan, np.inf, -np.inf, 2.0 ** 43, -0.0])
            xy.append(pts.reshape(-1))
            pt_off.append(pt_off[-1] + n)
            cls.append(int(rng.integers(-1, n_classes)))
        row_off.append(len(pt_off) - 1)
    xy = np.concatenate(xy) if xy else np.zeros(0)
    return (xy, np.asarray(pt_off, np.int32), np.asarray(row_off, np.int32), np.asarray(cls, np.int32), W, H, st, n_classes)


def same(got, want):
    cat, dfc, area, cc, hist = got
    assert np.array_equal(cat, want[0])
    assert np.array_equal(dfc, want[1])
    assert np.array_equal(np.isnan(area), np.isnan(want[2]))
    ok = ~np.isnan(want[2])
    assert np.array_equal(area[ok].view(np.uint64), np.asarray(want[2])[ok].view(np.uint64))
    assert np.array_equal(cc, want[3]) and np.array_equal(hist, want[4])


def run_dev(table, min_area=1.0, offset=1, hz=None):
    """the _dev entry on torch tensors, every output at an odd offset inside a guarded buffer.
    hz: the harness of tests/stream_contract.py (its decoys in the table's order, xy to size_status); without one the call goes
    to torch's current stream"""
    import torch
    from deal_yolo_daya_amd import _native
    from stream_contract import PLAIN

    hz = hz or PLAIN
    xy, pt_off, row_off, cls, W, H, st, nc = table
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    xy_buf = torch.zeros(len(xy) + 4, dtype=torch.float64, device=dev)
    xy_buf[2:2 + len(xy)] = t(xy, np.float64)                                  # 16-B aligned, not at the allocation's start
    nb, n = len(cls), len(row_off) - 1
    guard = 0xA5
    u8 = lambda k: torch.full((k + 2 * offset,), guard, dtype=torch.uint8, device=dev)   # noqa: E731
    cat, dfc = u8(nb), u8(nb)
    area = torch.full((nb + 2 * offset,), -7.0, dtype=torch.float64, device=dev)
    cc = torch.full((nc * 14 + 2 * offset,), -7, dtype=torch.int64, device=dev)
    hist = torch.full((nc * 11 + 2 * offset,), -7, dtype=torch.int64, device=dev)
    keep = [t(pt_off, np.int32), t(row_off, np.int32), t(cls, np.int32), t(W, np.float64), t(H, np.float64), t(st, np.uint8)]
    L = _native.lib()
    hz.arm([xy_buf[2:2 + len(xy)]] + keep)
    hz.watch(cat, dfc, area, cc, hist)
    _native.check(hz.call(L.dyd_audit_polygons_dev, xy_buf.data_ptr() + 16, *(a.data_ptr() for a in keep), n, nb, len(xy) // 2, nc,
                          float(min_area), cat.data_ptr() + offset, dfc.data_ptr() + offset, area.data_ptr() + 8 * offset,
                          cc.data_ptr() + 8 * offset, hist.data_ptr() + 8 * offset), "dyd_audit_polygons_dev")
    hz.restore()
    out = [a.cpu().numpy() for a in (cat, dfc, area, cc, hist)]
    for a, fill in zip(out, (guard, guard, -7.0, -7, -7)):
        assert (a[:offset] == fill).all() and (a[len(a) - offset:] == fill).all(), "write outside the outputs"
    return (out[0][offset:-offset], out[1][offset:-offset], out[2][offset:-offset], out[3][offset:-offset].reshape(nc, 14),
            out[4][offset:-offset].reshape(nc, 11))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(native, seed):
    table = random_table(np.random.default_rng(seed), 700)
    want = R.audit_arrays(*table)
    same(native.audit_polygons(*table), want)
    same(run_dev(table), want)
    assert (want[1] & R.SELFX).any() and (want[1] & R.DUP).any() and len(set(want[0].tolist())) == 7


def _one(raw, W=1e9, H=1e9, cls=0):
    xy = np.asarray(raw, np.float64).reshape(-1)
    return (xy, np.asarray([0, len(raw)], np.int32), np.asarray([0, 1], np.int32), np.asarray([cls], np.int32),
            np.asarray([W]), np.asarray([H]), np.zeros(1, np.uint8), 1)


def _expect_big(raw, W, H, selfx):
    """the restatement of one large polygon with its self_intersecting bit given (the pair test is O(m^2) in Python)"""
    V = [(float(x), float(y)) for x, y in raw]
    act, _ = S.polygon(V, W, H, 0)
    C_ = R.clipped(V, W, H)
    a = R.area(C_)
    bits = (R.DUP if any(V[k] == V[k - 1] for k in range(len(V))) else 0) | (R.SELFX if selfx else 0) | (R.TINY if a < 1.0 else 0)
    return S.ACTIONS.index(act), bits, a


@pytest.mark.parametrize("shape", ["star", "convex", "first_last"])
def test_10000_vertex_polygons(native, shape):
    n = 10_000
    if shape == "star":                                  # a {n/3} star: every edge crosses others
        th = 2 * np.pi * 3 * np.arange(n) / n
        raw, W, H, selfx = np.stack([5000 + 4000 * np.cos(th), 5000 + 4000 * np.sin(th)], 1), 1e4, 1e4, True
    elif shape == "convex":                              # (k, k^2): exactly convex, no three points collinear
        k = np.arange(n, dtype=np.float64)
        raw, W, H, selfx = np.stack([k, k * k], 1), 1e4, 1e8, False
    else:                                                # e_0 = (V0, V1) crosses only (V[n-2], V[n-1]), the last edge but one
        th = np.linspace(0.0, np.pi, n - 3)
        arc = np.stack([4.5 + 5.5 * np.cos(th), 1.0 + 1000.0 * np.sin(th)], 1)
        raw, W, H, selfx = np.concatenate([[[0.0, 0.0], [10.0, 0.0]], arc, [[5.0, -1.0]]]), 2000.0, 2000.0, True
    raw = [tuple(p) for p in raw.tolist()]
    if shape == "first_last":                            # the restatement agrees on a smaller copy of the same shape
        th = np.linspace(0.0, np.pi, 60)
        small = [(0.0, 0.0), (10.0, 0.0), *[(4.5 + 5.5 * math.cos(t), 1.0 + 1000.0 * math.sin(t)) for t in th], (5.0, -1.0)]
        assert R.self_intersecting(small) and not R.self_intersecting(small[:-1])
    table = _one(raw, W, H)
    cat, dfc, area, cc, hist = native.audit_polygons(*table)
    want = _expect_big(raw, W, H, selfx)
    assert (int(cat[0]), int(dfc[0])) == want[:2]
    assert area[0] == want[2]
    assert cc[0, 9] == int(selfx) and hist[0, 10] == 1
    same(run_dev(table), (cat, dfc, area, cc, hist))


def _ring(m, cross):
    """m distinct vertices (m edges of U): a convex ring, with the last two swapped when cross (a bow-tie at the end)"""
    th = 2 * np.pi * np.arange(m) / m
    pts = [(float(round(500 + 400 * math.cos(t))), float(round(500 + 400 * math.sin(t)))) for t in th]
    if cross:
        pts[-1], pts[-2] = pts[-2], pts[-1]
    return pts


def test_tier_thresholds(native):
    xy, pt_off, cls = [], [0], []
    for m in (LANE_EDGES - 1, LANE_EDGES, LANE_EDGES + 1):
        for cross in (False, True):
            for dup in (False, True):
                pts = _ring(m, cross)
                if dup:
                    pts.insert(5, pts[5])                # one repeat: len(V) = m + 1, still m edges of U
                xy.extend(np.asarray(pts).reshape(-1).tolist())
                pt_off.append(pt_off[-1] + len(pts))
                cls.append(len(cls) % 3)
    table = (np.asarray(xy), np.asarray(pt_off, np.int32), np.asarray([0, len(cls)], np.int32), np.asarray(cls, np.int32),
             np.asarray([1000.0]), np.asarray([1000.0]), np.zeros(1, np.uint8), 3)
    want = R.audit_arrays(*table)
    assert ((want[1] & R.SELFX) != 0).tolist() == [False, False, True, True] * 3
    same(native.audit_polygons(*table), want)
    same(run_dev(table), want)


def test_categories_equal_k13_actions(native):
    xy, pt_off, row_off, cls, W, H, st, nc = random_table(np.random.default_rng(9), 1500)
    cat = native.audit_polygons(xy, pt_off, row_off, cls, W, H, st, nc)[0]
    w13, h13 = np.where(st == 0, W, 0.0), np.where(st == 0, H, 0.0)
    action = native.yolo_seg_lines(xy, pt_off, row_off, None, w13, h13, np.zeros(len(W), np.int32))[2]
    m = cls >= 0
    assert m.sum() > 1000 and np.array_equal(cat[m], action[m])


def test_dev_on_10m_rows(native):
    import torch
    from deal_yolo_daya_amd import _native

    dev = torch.device("cuda", 0)
    d = synth.generate_device(10_000_000, 4, dev)
    xy, pt_off, row_off = d["xy"].contiguous(), d["pt_off"].to(torch.int32), d["box_off"].to(torch.int32)
    N, B, P_ = row_off.numel() - 1, pt_off.numel() - 1, xy.shape[0]
    nc = 20
    W = torch.full((N,), 1920.0, dtype=torch.float64, device=dev)
    H = torch.full((N,), 1080.0, dtype=torch.float64, device=dev)
    st = torch.zeros(N, dtype=torch.uint8, device=dev)
    cls = (torch.arange(B, device=dev, dtype=torch.int32) % (nc + 1) - 1).contiguous()      # every 21st unmatchable
    cat = torch.empty(B, dtype=torch.uint8, device=dev)
    dfc = torch.empty(B, dtype=torch.uint8, device=dev)
    area = torch.empty(B, dtype=torch.float64, device=dev)
    cc = torch.empty((nc, 14), dtype=torch.int64, device=dev)
    hist = torch.empty((nc, 11), dtype=torch.int64, device=dev)
    L, sp = _native.lib(), torch.cuda.current_stream().cuda_stream
    _native.check(L.dyd_audit_polygons_dev(xy.data_ptr(), pt_off.data_ptr(), row_off.data_ptr(), cls.data_ptr(), W.data_ptr(),
                                           H.data_ptr(), st.data_ptr(), N, B, P_, nc, 1.0, cat.data_ptr(), dfc.data_ptr(),
                                           area.data_ptr(), cc.data_ptr(), hist.data_ptr(), sp), "dyd_audit_polygons_dev")
    torch.cuda.synchronize()
    cc, hist, cls_h = cc.cpu().numpy(), hist.cpu().numpy(), cls.cpu().numpy()
    cat_h, dfc_h, area_h = cat.cpu().numpy(), dfc.cpu().numpy(), area.cpu().numpy()
    matched = int((cls_h >= 0).sum())
    assert B > 100_000_000 and cc[:, 0].sum() == matched and cc[:, 2:8].sum() == matched
    assert hist.sum() == matched and (cat_h == 255).sum() == B - matched
    for j, bit in enumerate((R.DUP, R.SELFX, R.TINY)):
        assert cc[:, 8 + j].sum() == int(((dfc_h & bit) != 0).sum())
    for k in range(6):
        assert cc[:, 2 + k].sum() == int((cat_h == k).sum())
    pt_h, row_h = pt_off.cpu().numpy(), row_off.cpu().numpy()
    rng = np.random.default_rng(0)
    for b in rng.choice(B, 5000, replace=False).tolist():
        r = int(np.searchsorted(row_h, b, side="right") - 1)
        raw = [tuple(p) for p in xy[int(pt_h[b]):int(pt_h[b + 1])].cpu().numpy().tolist()]
        if cls_h[b] < 0:
            assert cat_h[b] == 255
            continue
        code, bits, a = R.polygon(raw, 1920.0, 1080.0)
        assert (cat_h[b], dfc_h[b]) == (code, bits), (b, r)
        assert (math.isnan(a) and math.isnan(area_h[b])) or area_h[b] == a


def test_audit_polygons_csv_end_to_end(native, tmp_path):
    df = _table(1500, 8)
    path = tmp_path / "t.csv"
    df.to_csv(path, index=False, encoding="utf-8-sig")
    got = P.audit_polygons_csv(str(path), tmp_path / "gpu")
    want = P.audit_polygons_csv(str(path), tmp_path / "ref", backend=BE)
    assert {k: v for k, v in got.items() if k != "paths"} == {k: v for k, v in want.items() if k != "paths"}
    for k in ("classes", "problems"):
        a = pd.read_csv(got["paths"][k], encoding="utf-8-sig", keep_default_na=False)
        b = pd.read_csv(want["paths"][k], encoding="utf-8-sig", keep_default_na=False)
        assert a.equals(b), k
    ha, hb = np.load(got["paths"]["hist"]), np.load(want["paths"]["hist"])
    assert np.array_equal(ha["hist_vertices"], hb["hist_vertices"]) and got["self_intersecting"] > 0
