#!/usr/bin/env python3
"""Per-kernel micro-benchmarks on one MI355X (device-resident inputs, HIP-event timing,
interleaved A/B rounds in one process).  Prints one JSON line per kernel/variant.

    python tools/kbench.py [--rows 1000000] [--iters 20] [--only k1,k2,...]   (k9: suppression, k10: box audit, k11: box repair, each against K2 alone; k18: box comparison beside K2 and K9; k24: scored evaluation beside K18; k13: segmentation lines beside K7;
     k14: polygon audit; k14tier: its in-lane / wave threshold; simplify: polygon simplification (K19) beside K14 on rings of 8, 64 and 1024 points; k16: COCO annotation objects beside K13; k17: oriented-box lines beside K13; tile: tiled label lines (K20) beside K13;
     k21: label masks (K21) on many small and few large images, beside Pillow on one core; k22: polygon comparison (K22) on the same
     two tables, interleaved with K21 over either side; k23: COCO run-length masks (K23) on the same two tables, measure-only and
     full, interleaved with K21 over the same table; k25: scored polygon evaluation (K25) at T = 1 and T = 10 beside K22 on the same
     two tables, through the host entries)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="k1,k2,k3,k4,k5,k6")
    ap.add_argument("--bpr", type=int, default=0, help="fixed boxes per row (0 = U{1..32})")
    ap.add_argument("--tile", type=int, default=640, help="tile size of the `tile` entry")
    ap.add_argument("--overlap", type=float, default=0.2, help="tile overlap of the `tile` entry")
    args = ap.parse_args()
    only = set(args.only.split(","))

    import torch
    from deal_yolo_daya_amd import _native, synth

    dev = torch.device("cuda", 0)
    L = _native.lib()
    sp = torch.cuda.current_stream().cuda_stream
    ck = _native.check

    def timeit(fn, iters=args.iters, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(np.min(ts))

    def timeit_b2b(fn, n=100, warm=10):
        """ms per launch when the launches are queued back to back (what bench.py times): one event pair around n launches"""
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record(); b.synchronize()
        return a.elapsed_time(b) / n

    def report(name, nbytes, med, mn, **kw):
        print(json.dumps({"kernel": name, "ms_median": round(med, 4), "ms_min": round(mn, 4),
                          "alg_GB": round(nbytes / 1e9, 4), "GBs_median": round(nbytes / med / 1e6, 1),
                          "frac_of_8TBs": round(nbytes / med / 1e6 / 8000, 4), **kw}), flush=True)

    rows = args.rows
    parts = []
    for ci, s in enumerate(range(0, rows, 1_000_000)):
        parts.append(synth.generate(min(1_000_000, rows - s), seed=synth.SEED + ci,
                                    boxes_per_row=args.bpr or None))
    xy = torch.cat([torch.from_numpy(t.xy) for t in parts]).to(dev)
    npts = torch.cat([torch.from_numpy(np.diff(t.pt_off)) for t in parts]).to(dev)
    nbox = torch.cat([torch.from_numpy(np.diff(t.box_off)) for t in parts]).to(dev)
    url_id = np.concatenate([t.url_id for t in parts])
    labels = torch.cat([torch.from_numpy(t.label) for t in parts]).to(dev)
    del parts
    P, B, N = xy.shape[0], npts.shape[0], nbox.shape[0]
    pt_off = torch.zeros(B + 1, dtype=torch.int32, device=dev); pt_off[1:] = torch.cumsum(npts, 0).to(torch.int32)
    box_off = torch.zeros(N + 1, dtype=torch.int32, device=dev); box_off[1:] = torch.cumsum(nbox, 0).to(torch.int32)
    out_box = torch.empty((B, 4), dtype=torch.float64, device=dev)
    out_arg = torch.empty((B, 4), dtype=torch.int32, device=dev)
    out_high = torch.empty(N, dtype=torch.uint8, device=dev)
    print(json.dumps({"rows": N, "boxes": B, "points": P, "device": _native.device_name()}), flush=True)

    if "k1" in only:
        k1_bytes = 16 * P + 4 * (B + 1) + 48 * B
        res = {}
        for rnd in range(2):                      # interleaved rounds (guide rule 24)
            for variant in (0, 1):
                ck(L.dyd_set_option(b"k1_variant", variant), "opt")
                med, mn = timeit(lambda: ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P,
                                                                   out_box.data_ptr(), out_arg.data_ptr(), sp), "k1"))
                res.setdefault(variant, []).append((med, mn))
        ck(L.dyd_set_option(b"k1_variant", -1), "opt")
        for variant, name in ((0, "k1_bbox_lds"), (1, "k1_bbox_direct")):
            med = float(np.median([r[0] for r in res[variant]])); mn = min(r[1] for r in res[variant])
            report(name, k1_bytes, med, mn, rows_per_s=round(N / med * 1e3))
        # streaming ceilings of this box on a comparable byte count (each array 1.4 GB >> 256 MiB L3)
        nb_ = k1_bytes // 2 // 16 * 16
        src = torch.empty(nb_ // 8, dtype=torch.float64, device=dev).normal_(); dst = torch.empty_like(src)
        for blocks in (2048, 8192):
            for mode, nm, tot in ((0, "copy", 2 * nb_), (1, "read", nb_), (2, "write", nb_), (3, "copy_nt", 2 * nb_),
                                  (4, "read_nt", nb_), (5, "write_nt", nb_)):
                med, mn = timeit(lambda: ck(L.dyd_membench_dev(mode, src.data_ptr(), dst.data_ptr(), nb_, blocks, sp), "mb"))
                report(f"membench_{nm}_b{blocks}", tot, med, mn)
        med, mn = timeit(lambda: dst.copy_(src))
        report("torch_d2d_copy", 2 * nb_, med, mn)
        del src, dst
    if "rand" in only:
        # random-access ceilings (one 8-byte word per lane, every word of the table once): what K4/K5/K6 are quoted against
        for mib in (32, 64, 128, 256, 512, 1024, 2048):          # around the 256 MiB Infinity Cache
            table = torch.zeros(mib << 17, dtype=torch.int64, device=dev)
            for mode, nm, word in ((6, "scatter", 8), (9, "scatter4", 4), (7, "gather", 8), (8, "atomic_min", 8)):
                words = (mib << 20) // word
                med, mn = timeit(lambda: ck(L.dyd_membench_dev(mode, table.data_ptr(), table.data_ptr(), mib << 20, 8192, sp), "mb"))
                print(json.dumps({"kernel": f"membench_random_{nm}_{mib}MiB", "ms_median": round(med, 4), "ms_min": round(mn, 4),
                                  "words": words, "G_words_per_s": round(words / med / 1e6, 2), "useful_GBs": round(word * words / med / 1e6, 1)}), flush=True)
            del table

    if "k2" in only:
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        k2_bytes = 32 * B + 4 * (N + 1) + N
        nb64 = nbox.to(torch.int64)
        pairs = int((nb64 * (nb64 - 1) // 2).sum().item())
        for variant, nm in ((0, "k2_iou<16,256>"), (1, "k2_iou<8,128>"), (2, "k2f_iou<16,256> (f32 filter)"),
                            (3, "k2f_iou<8,128> (f32 filter)"), (4, "k2_wave64 (the fused kernel's pair stage)"), (-1, "k2 auto")):
            ck(L.dyd_set_option(b"k2_variant", variant), "opt")
            med, mn = timeit(lambda: ck(L.dyd_iou_any_ge_dev(out_box.data_ptr(), box_off.data_ptr(), N, B, 2, 0.98,
                                                              out_high.data_ptr(), None, sp), "k2"))
            report(nm, k2_bytes, med, mn, rows_per_s=round(N / med * 1e3), pairs=pairs,
                   gpairs_per_s=round(pairs / med / 1e6, 2), high=int(out_high.sum().item()))
        ck(L.dyd_set_option(b"k2_variant", 3), "opt")
        mx = torch.empty(N, dtype=torch.float64, device=dev)
        med, mn = timeit(lambda: ck(L.dyd_iou_any_ge_dev(out_box.data_ptr(), box_off.data_ptr(), N, B, 2, 0.98,
                                                          out_high.data_ptr(), mx.data_ptr(), sp), "k2max"))
        report("k2_iou_want_max", k2_bytes + 8 * N, med, mn, gpairs_per_s=round(pairs / med / 1e6, 2))

    if "k9" in only:
        # K9 (duplicate-box suppression) against K2 alone on the same device buffers, interleaved rounds
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        keep = torch.empty(B, dtype=torch.uint8, device=dev)
        partner = torch.empty(B, dtype=torch.int32, device=dev)
        names = labels.to(torch.int32).contiguous()
        legs = {"k2 auto (dyd_iou_any_ge_dev)": (32 * B + 4 * (N + 1) + N, lambda: ck(L.dyd_iou_any_ge_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, 2, 0.98, out_high.data_ptr(), None, sp), "k2")),
                "k9_suppress": (32 * B + 4 * (N + 1) + 5 * B, lambda: ck(L.dyd_suppress_boxes_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, None, 0.98, keep.data_ptr(), partner.data_ptr(), sp), "k9")),
                "k9_suppress by_label": (36 * B + 4 * (N + 1) + 5 * B, lambda: ck(L.dyd_suppress_boxes_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, names.data_ptr(), 0.98, keep.data_ptr(), partner.data_ptr(),
                    sp), "k9"))}
        res = {}
        for rnd in range(2):
            for nm, (_, fn) in legs.items():
                res.setdefault(nm, []).append(timeit(fn))
        for nm, (nbytes, _) in legs.items():
            med = float(np.median([r[0] for r in res[nm]])); mn = min(r[1] for r in res[nm])
            report(nm, nbytes, med, mn, rows_per_s=round(N / med * 1e3))
        legs["k9_suppress"][1]()
        torch.cuda.synchronize()
        print(json.dumps({"kernel": "k9_suppress", "dropped": int((keep == 0).sum().item())}), flush=True)

    if "k10" in only:
        # K10 (box audit) against K2 alone on the same device buffers, interleaved rounds: 20 classes at nb = 16 (LDS histograms)
        # and nb = 64 (global), 5,000 classes at nb = 16 (global class counters and histograms)
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        g = torch.Generator(device=dev).manual_seed(10)
        cls20 = (labels.to(torch.int64) % 20).to(torch.int32).contiguous()
        cls5k = torch.randint(0, 5000, (B,), generator=g, device=dev, dtype=torch.int32)
        wdt = torch.full((N,), 1280.0, dtype=torch.float64, device=dev)
        hgt = torch.full((N,), 720.0, dtype=torch.float64, device=dev)
        st = torch.zeros(N, dtype=torch.uint8, device=dev)
        flag = torch.empty(B, dtype=torch.uint8, device=dev)
        rowc = torch.empty((N, 6), dtype=torch.int32, device=dev)
        bpi = torch.empty(257, dtype=torch.int64, device=dev)
        outs = {}

        def k10(cls, nc, nb):
            if (nc, nb) not in outs:
                outs[(nc, nb)] = (torch.empty((nc, 9), dtype=torch.int64, device=dev),
                                  torch.empty(nc * nb * nb, dtype=torch.int64, device=dev),
                                  torch.empty(nc * nb * nb, dtype=torch.int64, device=dev))
            cc, wh, hxy = outs[(nc, nb)]
            return lambda: ck(L.dyd_box_audit_dev(out_box.data_ptr(), box_off.data_ptr(), N, B, cls.data_ptr(), wdt.data_ptr(),
                                                  hgt.data_ptr(), st.data_ptr(), nc, nb, flag.data_ptr(), rowc.data_ptr(),
                                                  cc.data_ptr(), wh.data_ptr(), hxy.data_ptr(), bpi.data_ptr(), sp), "k10")

        audit_bytes = 32 * B + 4 * B + B + 4 * (N + 1) + 17 * N + 24 * N
        legs = {"k2 auto (dyd_iou_any_ge_dev)": (32 * B + 4 * (N + 1) + N, lambda: ck(L.dyd_iou_any_ge_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, 2, 0.98, out_high.data_ptr(), None, sp), "k2")),
                "k10_audit c20 nb16": (audit_bytes, k10(cls20, 20, 16)),
                "k10_audit c20 nb64": (audit_bytes, k10(cls20, 20, 64)),
                "k10_audit c5000 nb16": (audit_bytes, k10(cls5k, 5000, 16))}
        res = {}
        for rnd in range(2):
            for nm, (_, fn) in legs.items():
                res.setdefault(nm, []).append(timeit(fn))
        for nm, (nbytes, _) in legs.items():
            med = float(np.median([r[0] for r in res[nm]])); mn = min(r[1] for r in res[nm])
            report(nm, nbytes, med, mn, rows_per_s=round(N / med * 1e3))
        legs["k10_audit c20 nb16"][1]()
        torch.cuda.synchronize()
        cc = outs[(20, 16)][0]
        print(json.dumps({"kernel": "k10_audit", "writable": int(cc[:, 3].sum().item()), "boxes": int(cc[:, :4].sum().item()),
                          "images": int(cc[:, 8].sum().item())}), flush=True)

    if "k11" in only:
        # K11 (box repair) against K2 alone and K10 (c20 nb16) on the same device buffers, interleaved rounds: 20 classes (LDS
        # class counters) with the default and with strict parameters, 5,000 classes (global class counters)
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        g = torch.Generator(device=dev).manual_seed(11)
        cls20 = (labels.to(torch.int64) % 20).to(torch.int32).contiguous()
        cls5k = torch.randint(0, 5000, (B,), generator=g, device=dev, dtype=torch.int32)
        wdt = torch.full((N,), 1280.0, dtype=torch.float64, device=dev)
        hgt = torch.full((N,), 720.0, dtype=torch.float64, device=dev)
        st = torch.zeros(N, dtype=torch.uint8, device=dev)
        act = torch.empty(B, dtype=torch.uint8, device=dev)
        rbox = torch.empty((B, 4), dtype=torch.float64, device=dev)
        rrows = torch.empty((N, 8), dtype=torch.int32, device=dev)
        rcc = {20: torch.empty((20, 8), dtype=torch.int64, device=dev), 5000: torch.empty((5000, 8), dtype=torch.int64, device=dev)}
        flag = torch.empty(B, dtype=torch.uint8, device=dev)
        arows = torch.empty((N, 6), dtype=torch.int32, device=dev)
        acc_ = torch.empty((20, 9), dtype=torch.int64, device=dev)
        awh = torch.empty(20 * 16 * 16, dtype=torch.int64, device=dev)
        axy = torch.empty(20 * 16 * 16, dtype=torch.int64, device=dev)
        bpi = torch.empty(257, dtype=torch.int64, device=dev)

        def k11(cls, nc, mv, ms):
            return lambda: ck(L.dyd_repair_boxes_dev(out_box.data_ptr(), box_off.data_ptr(), N, B, cls.data_ptr(), wdt.data_ptr(),
                                                     hgt.data_ptr(), st.data_ptr(), nc, mv, ms, act.data_ptr(), rbox.data_ptr(),
                                                     rrows.data_ptr(), rcc[nc].data_ptr(), sp), "k11")

        # bytes K11 needs: per box 32 in + 4 class + 1 action + 32 out; per row offset, W, H, status and 8 i32 counts
        repair_bytes = (32 + 4 + 1 + 32) * B + 4 * (N + 1) + (8 + 8 + 1 + 32) * N
        audit_bytes = 32 * B + 4 * B + B + 4 * (N + 1) + 17 * N + 24 * N
        legs = {"k2 auto (dyd_iou_any_ge_dev)": (32 * B + 4 * (N + 1) + N, lambda: ck(L.dyd_iou_any_ge_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, 2, 0.98, out_high.data_ptr(), None, sp), "k2")),
                "k10_audit c20 nb16": (audit_bytes, lambda: ck(L.dyd_box_audit_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, cls20.data_ptr(), wdt.data_ptr(), hgt.data_ptr(), st.data_ptr(),
                    20, 16, flag.data_ptr(), arows.data_ptr(), acc_.data_ptr(), awh.data_ptr(), axy.data_ptr(), bpi.data_ptr(),
                    sp), "k10")),
                "k11_repair c20": (repair_bytes, k11(cls20, 20, 0.0, 0.0)),
                "k11_repair c20 mv0.5 ms4": (repair_bytes, k11(cls20, 20, 0.5, 4.0)),
                "k11_repair c5000": (repair_bytes, k11(cls5k, 5000, 0.0, 0.0))}
        res = {}
        for rnd in range(2):
            for nm, (_, fn) in legs.items():
                res.setdefault(nm, []).append(timeit(fn))
        for nm, (nbytes, _) in legs.items():
            med = float(np.median([r[0] for r in res[nm]])); mn = min(r[1] for r in res[nm])
            report(nm, nbytes, med, mn, rows_per_s=round(N / med * 1e3))
        legs["k11_repair c20"][1]()
        torch.cuda.synchronize()
        cc = rcc[20]
        print(json.dumps({"kernel": "k11_repair", "boxes": int(cc.sum().item()),
                          **{a: int(cc[:, k].sum().item()) for k, a in enumerate(
                              ("keep", "clip", "no_size", "bad_coords", "degenerate", "outside", "low_visibility", "small"))}}),
              flush=True)

    def compare_table():
        """A = the K1 boxes with 20 classes; B = a copy with 10 % of the boxes dropped, 10 % jittered and 5 % put into another
        class -> (cls20, b_box, b_off, b_cls, Bb, u of the kept boxes): the table of the k18 and k24 legs"""
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        g = torch.Generator(device=dev).manual_seed(18)
        cls20 = (labels.to(torch.int64) % 20).to(torch.int32).contiguous()
        u = torch.rand(B, generator=g, device=dev)
        kept = u >= 0.10
        b_box = out_box[kept].clone()
        ub = u[kept]
        b_box[:, 3] += torch.where(ub < 0.20, 2.0, 0.0).to(torch.float64)
        b_cls = torch.where(ub >= 0.95, (cls20[kept] + 1) % 20, cls20[kept]).to(torch.int32).contiguous()
        row = torch.repeat_interleave(torch.arange(N, device=dev), nbox.to(torch.int64))
        b_off = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        b_off[1:] = torch.cumsum(torch.bincount(row[kept], minlength=N), 0).to(torch.int32)
        return cls20, b_box, b_off, b_cls, b_box.shape[0], ub

    if "k18" in only:
        # K18 (box comparison) beside K2 alone and K9 on the same device buffers, interleaved rounds, on compare_table()
        cls20, b_box, b_off, b_cls, Bb, _ = compare_table()
        keep = torch.empty(B, dtype=torch.uint8, device=dev)
        partner = torch.empty(B, dtype=torch.int32, device=dev)
        a_match = torch.empty(B, dtype=torch.int32, device=dev)
        a_best = torch.empty(B, dtype=torch.float64, device=dev)
        b_match = torch.empty(Bb, dtype=torch.int32, device=dev)
        b_iou = torch.empty(Bb, dtype=torch.float64, device=dev)
        b_best = torch.empty(Bb, dtype=torch.float64, device=dev)
        crow = torch.empty((N, 4), dtype=torch.int32, device=dev)
        conf = torch.empty((21, 21), dtype=torch.int64, device=dev)

        def k18(by_label):
            return lambda: ck(L.dyd_compare_boxes_dev(
                out_box.data_ptr(), box_off.data_ptr(), cls20.data_ptr(), b_box.data_ptr(), b_off.data_ptr(), b_cls.data_ptr(), N, B,
                Bb, 20, 0.5, by_label, a_match.data_ptr(), b_match.data_ptr(), b_iou.data_ptr(), a_best.data_ptr(),
                b_best.data_ptr(), crow.data_ptr(), conf.data_ptr(), sp), "k18")

        # bytes K18 needs: per box 32 + 4 class in; 12 out per A box, 20 per B box; two offsets in and 16 out per row
        k18_bytes = 36 * (B + Bb) + 12 * B + 20 * Bb + 8 * (N + 1) + 16 * N
        legs = {"k2 auto (dyd_iou_any_ge_dev)": (32 * B + 4 * (N + 1) + N, lambda: ck(L.dyd_iou_any_ge_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, 2, 0.98, out_high.data_ptr(), None, sp), "k2")),
                "k9_suppress": (32 * B + 4 * (N + 1) + 5 * B, lambda: ck(L.dyd_suppress_boxes_dev(
                    out_box.data_ptr(), box_off.data_ptr(), N, B, None, 0.98, keep.data_ptr(), partner.data_ptr(), sp), "k9")),
                "k18_compare": (k18_bytes, k18(0)),
                "k18_compare by_label": (k18_bytes, k18(1))}
        res = {}
        for rnd in range(2):
            for nm, (_, fn) in legs.items():
                res.setdefault(nm, []).append(timeit(fn))
        for nm, (nbytes, _) in legs.items():
            med = float(np.median([r[0] for r in res[nm]])); mn = min(r[1] for r in res[nm])
            report(nm, nbytes, med, mn, rows_per_s=round(N / med * 1e3))
        legs["k18_compare"][1]()
        torch.cuda.synchronize()
        print(json.dumps({"kernel": "k18_compare", "a_boxes": B, "b_boxes": Bb, "matched": int((b_match >= 0).sum().item()),
                          "agree": int(conf[:20, :20].diagonal().sum().item()), "missing": int(conf[:20, 20].sum().item()),
                          "extra": int(conf[20, :20].sum().item())}), flush=True)

    if "k24" in only:
        # K24 (scored evaluation) through its host entries on compare_table() with a score per B box, kernel time from
        # dyd_last_kernel_ms; K18 by_label through its host entry on the same table, timed the same way, is the yardstick: K24
        # at T = 1 does K18's pair work within the classes plus the ranking.  Then the accumulation alone on the T = 10 result.
        cls20, b_box, b_off, b_cls, Bb, ub = compare_table()
        host = [t.cpu().numpy() for t in (out_box, box_off, cls20, b_box, b_off, b_cls)]
        score = np.round(ub.cpu().numpy() * 0.37 % 1.0, 3)               # three decimals: ties within and across rows
        thr10 = np.linspace(0.5, 0.95, 10)

        def kernel_ms(fn, iters=max(3, args.iters // 4)):
            fn()
            ts = []
            for _ in range(iters):
                fn()
                ts.append(_native.last_kernel_ms())
            return float(np.median(ts)), float(np.min(ts))

        k24_bytes = 36 * B + 44 * Bb + 8 * (N + 1) + 12 * B + 32 * Bb
        k18_bytes = 36 * (B + Bb) + 12 * B + 20 * Bb + 8 * (N + 1) + 16 * N
        legs = {"k18_compare by_label (host entry)": (k18_bytes, lambda: _native.compare_boxes(*host, 20, 0.5, True)),
                "k24_match T=1": (k24_bytes, lambda: _native.eval_match_boxes(*host, score, 20, [0.5], 100)),
                "k24_match T=10": (k24_bytes, lambda: _native.eval_match_boxes(*host, score, 20, thr10, 100))}
        res = {}
        for rnd in range(2):
            for nm, (_, fn) in legs.items():
                res.setdefault(nm, []).append(kernel_ms(fn))
        for nm, (nbytes, _) in legs.items():
            med = float(np.median([r[0] for r in res[nm]])); mn = min(r[1] for r in res[nm])
            report(nm, nbytes, med, mn, rows_per_s=round(N / med * 1e3))
        state, tp, *_ = _native.eval_match_boxes(*host, score, 20, thr10, 100)
        ev = state == 0
        npig = np.bincount(host[2], minlength=20).astype(np.int64)
        acc = lambda: _native.eval_accumulate(host[5][ev], score[ev], tp[ev], 20, 10, npig, np.linspace(0, 1, 101))   # noqa: E731
        med, mn = kernel_ms(acc)
        n_ev = int(ev.sum())
        report("k24_accumulate C=20 T=10", 16 * n_ev + 2 * 8 * 20 * 10 * 101, med, mn, detections_per_s=round(n_ev / med * 1e3))
        ap = acc()[3]
        print(json.dumps({"kernel": "k24_eval", "gt_boxes": B, "detections": Bb, "evaluated": n_ev,
                          "tp_at_0.5": int((tp[ev] & 1).sum()), "map": round(float(np.nanmean(ap)), 6),
                          "map50": round(float(np.nanmean(ap[:, 0])), 6)}), flush=True)

    if "k12" in only:
        k12_bytes = 16 * P + 4 * (B + 1) + 48 * B + 4 * (N + 1) + N
        res = {}
        for rnd in range(2):
            for variant in (1, 4, 6, 9, 10):
                ck(L.dyd_set_option(b"fused_variant", variant), "opt")
                med, mn = timeit(lambda: ck(L.dyd_bbox_iou_fused_dev(xy.data_ptr(), pt_off.data_ptr(), box_off.data_ptr(),
                                                                      N, B, P, 2, 0.98, out_box.data_ptr(), out_arg.data_ptr(),
                                                                      out_high.data_ptr(), sp), "k12"))
                res.setdefault(variant, []).append((med, mn))
        ck(L.dyd_set_option(b"fused_variant", -1), "opt")
        for variant, name in ((4, "k12_wave_kernel"), (10, "k12_wave_dense_kernel"), (6, "k12_fused<1024,8,128,filter>"),
                              (9, "k12_fused<1024,8,256,filter>"), (1, "k1_then_k2_two_launches")):
            med = float(np.median([r[0] for r in res[variant]])); mn = min(r[1] for r in res[variant])
            report(name, k12_bytes, med, mn, rows_per_s=round(N / med * 1e3), high=int(out_high.sum().item()))

    if only & {"k3", "k4", "k5"}:
        urls = [f"http://img.example/{k}.jpg".encode() for k in url_id.tolist()]
        off_np = np.zeros(N + 1, np.int64); np.cumsum([len(u) for u in urls], out=off_np[1:])
        data = torch.from_numpy(np.frombuffer(b"".join(urls), np.uint8).copy()).to(dev)
        off = torch.from_numpy(off_np).to(dev)
        h = torch.empty((N, 2), dtype=torch.int64, device=dev)
        k3_bytes = int(off_np[-1]) + 8 * (N + 1) + 16 * N
        med, mn = timeit(lambda: ck(L.dyd_hash128_dev(data.data_ptr(), off.data_ptr(), N, h.data_ptr(), sp), "k3"))
        if "k3" in only:
            report("k3_hash128", k3_bytes, med, mn, rows_per_s=round(N / med * 1e3))
        keep = torch.empty(N, dtype=torch.uint8, device=dev)
        U = len(np.unique(url_id))
        if "k4" in only:
            for mode, nm in ((0, "first"), (1, "last"), (2, "none")):
                med, mn = timeit(lambda: ck(L.dyd_dedup_dev(h.data_ptr(), N, mode, keep.data_ptr(), sp), "k4"))
                report(f"k4_dedup_{nm}", 16 * N + N + 48 * U, med, mn, rows_per_s=round(N / med * 1e3),
                       kept=int(keep.sum().item()), distinct=U)
        if "k5" in only:
            R = max(1, N // 10)
            ref = h[torch.randperm(N, device=dev)[:R]].contiguous()
            med, mn = timeit(lambda: ck(L.dyd_isin_dev(h.data_ptr(), N, ref.data_ptr(), R, keep.data_ptr(), sp), "k5"))
            report("k5_isin", 16 * N + N + 16 * R, med, mn, rows_per_s=round(N / med * 1e3), hits=int(keep.sum().item()))

    if "k6" in only:
        E = B
        cat = torch.where(labels < 10, 0, torch.where(labels < 18, 1, -1)).to(torch.int32).contiguous()
        sizes = [int((cat == c).sum().item()) for c in (0, 1)]
        perm = torch.from_numpy(np.concatenate([_native.mt19937_permutation(42, s) for s in sizes])).to(dev)
        cat_off = torch.tensor([0, sizes[0], sizes[0] + sizes[1]], dtype=torch.int64, device=dev)
        n_train = torch.tensor([int(s * 0.8) for s in sizes], dtype=torch.int64, device=dev)
        n_val = torch.tensor([int(s * 0.1) for s in sizes], dtype=torch.int64, device=dev)
        split = torch.empty(E, dtype=torch.uint8, device=dev); pos = torch.empty(E, dtype=torch.int64, device=dev)
        med, mn = timeit(lambda: ck(L.dyd_split_ids_dev(cat.data_ptr(), E, perm.data_ptr(), cat_off.data_ptr(),
                                                         n_train.data_ptr(), n_val.data_ptr(), 2, split.data_ptr(),
                                                         pos.data_ptr(), sp), "k6"))
        report("k6_split_ids", 21 * E, med, mn, expanded_rows=E, rows_per_s=round(E / med * 1e3))

    if "k3len" in only:
        # K3 against the cell length (signed CDN URLs run to hundreds of bytes): ~1 GB of text per table
        g = torch.Generator(device=dev).manual_seed(8)
        for L_ in (30, 100, 400, 2000):
            n3 = max(1000, 1_000_000_000 // L_)
            lens = torch.randint(max(1, L_ // 2), L_ * 3 // 2 + 1, (n3,), generator=g, device=dev)
            off3 = torch.zeros(n3 + 1, dtype=torch.int64, device=dev)
            off3[1:] = torch.cumsum(lens, 0)
            tot3 = int(off3[-1].item())
            data3 = torch.randint(32, 127, (tot3,), generator=g, device=dev, dtype=torch.uint8)
            h3 = torch.empty((n3, 2), dtype=torch.int64, device=dev)
            med, mn = timeit(lambda: ck(L.dyd_hash128_dev(data3.data_ptr(), off3.data_ptr(), n3, h3.data_ptr(), sp), "k3"), iters=8, warm=2)
            report(f"k3_hash128_len{L_}", tot3 + 8 * (n3 + 1) + 16 * n3, med, mn, rows=n3, text_GB=round(tot3 / 1e9, 3))
            del lens, off3, data3, h3

    if "k6cats" in only:
        # K6 against the number of categories (the columns of the rules sheet): 16.5 M expanded rows, uniform labels
        g = torch.Generator(device=dev).manual_seed(4)
        E6 = 16_500_000
        for ncat in (2, 16, 128, 1000, 5000):
            cat6 = torch.randint(-1, ncat, (E6,), generator=g, device=dev, dtype=torch.int32)
            sizes6 = torch.bincount(cat6[cat6 >= 0].to(torch.int64), minlength=ncat)
            cat_off6 = torch.zeros(ncat + 1, dtype=torch.int64, device=dev)
            cat_off6[1:] = torch.cumsum(sizes6, 0)
            perm6 = torch.cat([torch.randperm(int(sz), generator=g, device=dev) for sz in sizes6.tolist()]).contiguous() if ncat <= 1000 else \
                torch.arange(int(cat_off6[-1].item()), device=dev) - torch.repeat_interleave(cat_off6[:-1], sizes6)
            ntr6 = (sizes6 * 8 // 10).contiguous(); nva6 = (sizes6 // 10).contiguous()
            sp6 = torch.empty(E6, dtype=torch.uint8, device=dev); pos6 = torch.empty(E6, dtype=torch.int64, device=dev)
            med, mn = timeit(lambda: ck(L.dyd_split_ids_dev(cat6.data_ptr(), E6, perm6.data_ptr(), cat_off6.data_ptr(), ntr6.data_ptr(),
                                                             nva6.data_ptr(), ncat, sp6.data_ptr(), pos6.data_ptr(), sp), "k6"), iters=8, warm=2)
            report(f"k6_split_ids_{ncat}_categories", 21 * E6, med, mn, expanded_rows=E6)
            del cat6, perm6, sp6, pos6

    if "k5big" in only:
        # the 10 M-row pipeline's K4 / K5 on random 128-bit keys: 10 M rows (60 % distinct), 1 M reference keys, 10 % hits
        Nk = 10_000_000
        g = torch.Generator(device=dev).manual_seed(5)
        base = torch.randint(-2**62, 2**62, (6_000_000, 2), generator=g, device=dev, dtype=torch.int64)
        hk = base[torch.randint(0, base.shape[0], (Nk,), generator=g, device=dev)].contiguous()
        refk = torch.cat([base[:100_000], torch.randint(-2**62, 2**62, (900_000, 2), generator=g, device=dev, dtype=torch.int64)]).contiguous()
        keepk = torch.empty(Nk, dtype=torch.uint8, device=dev)
        med, mn = timeit(lambda: ck(L.dyd_dedup_dev(hk.data_ptr(), Nk, 0, keepk.data_ptr(), sp), "k4"))
        report("k4_dedup_first_10M", 16 * Nk + Nk + 48 * 6_000_000, med, mn, rows_per_s=round(Nk / med * 1e3), kept=int(keepk.sum().item()))
        med, mn = timeit(lambda: ck(L.dyd_isin_dev(hk.data_ptr(), Nk, refk.data_ptr(), refk.shape[0], keepk.data_ptr(), sp), "k5"))
        report("k5_isin_10M_vs_1M", 16 * Nk + Nk + 16 * refk.shape[0], med, mn, rows_per_s=round(Nk / med * 1e3), hits=int(keepk.sum().item()))
        # the other extreme: one key (a constant column, or all NaN), and 1000 keys — every row contends for few slots
        for distinct in (1, 1000):
            few = base[torch.randint(0, distinct, (Nk,), generator=g, device=dev)].contiguous()
            for mode, nm in ((0, "first"), (1, "last"), (2, "none")):
                med, mn = timeit(lambda: ck(L.dyd_dedup_dev(few.data_ptr(), Nk, mode, keepk.data_ptr(), sp), "k4"), iters=5, warm=1)
                report(f"k4_dedup_{nm}_10M_rows_{distinct}_keys", 16 * Nk + Nk, med, mn, rows_per_s=round(Nk / med * 1e3), kept=int(keepk.sum().item()))
            del few
        del base, hk, refk, keepk

    if "k6big" in only:
        # the 10 M-row pipeline's K6 (165 M expanded rows): the inverse-permutation table no longer fits the Infinity Cache
        E = int(os.environ.get("K6_ROWS", 165_000_000))
        g = torch.Generator(device=dev).manual_seed(3)
        lab = torch.randint(0, 20, (E,), generator=g, device=dev, dtype=torch.int32)
        cat = torch.where(lab < 10, 0, torch.where(lab < 18, 1, -1)).to(torch.int32).contiguous()
        del lab
        sizes = [int((cat == c).sum().item()) for c in (0, 1)]
        perm = torch.cat([torch.randperm(s, generator=g, device=dev) for s in sizes]).contiguous()
        cat_off = torch.tensor([0, sizes[0], sizes[0] + sizes[1]], dtype=torch.int64, device=dev)
        n_train = torch.tensor([int(s * 0.8) for s in sizes], dtype=torch.int64, device=dev)
        n_val = torch.tensor([int(s * 0.1) for s in sizes], dtype=torch.int64, device=dev)
        split = torch.empty(E, dtype=torch.uint8, device=dev); pos = torch.empty(E, dtype=torch.int64, device=dev)
        ref = None
        for mib in [int(v) for v in os.environ.get("K6V", "0,1,0,1").split(",")]:   # 0 = 64-bit inverse table, 1 = 32-bit (default)
            ck(L.dyd_set_option(b"k6_variant", mib), "opt")
            med, mn = timeit(lambda: ck(L.dyd_split_ids_dev(cat.data_ptr(), E, perm.data_ptr(), cat_off.data_ptr(), n_train.data_ptr(),
                                                             n_val.data_ptr(), 2, split.data_ptr(), pos.data_ptr(), sp), "k6"), iters=10, warm=2)
            chk = (int(pos.sum().item()), int(split.to(torch.int64).sum().item()))
            ref = ref or chk
            report(f"k6_split_ids_165M_{'32' if mib else '64'}bit_inverse", 21 * E, med, mn, expanded_rows=E, same_as_first=(chk == ref))
        ck(L.dyd_set_option(b"k6_variant", 1), "opt")
        del cat, perm, split, pos

    if "k7" in only:
        import ctypes as C
        # the shape of a split sheet: one labelled box per expanded row; boxes = K1's output for the synthetic polygons
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        E = B
        one = torch.arange(E + 1, dtype=torch.int32, device=dev)
        w = torch.full((E,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((E,), 1080.0, dtype=torch.float64, device=dev)
        cid = (torch.arange(E, device=dev, dtype=torch.int32) % 20).contiguous()
        toff = torch.empty(E + 1, dtype=torch.int64, device=dev); flag = torch.empty(E, dtype=torch.uint8, device=dev)
        total = C.c_int64()
        ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), one.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), E, E,
                                toff.data_ptr(), flag.data_ptr(), None, 0, C.byref(total), sp), "k7 measure")
        T = total.value
        text = torch.empty(T, dtype=torch.uint8, device=dev)
        modes = os.environ.get("K7MODE", "full,measure").split(",")
        for variant in [int(v) for v in os.environ.get("K7V", "2,22,30,-1").split(",")]:
            ck(L.dyd_set_option(b"k7_variant", variant), "opt")
            if "full" in modes:
              med, mn = timeit(lambda: ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), one.data_ptr(), None, w.data_ptr(), h.data_ptr(),
                                                              cid.data_ptr(), E, E, toff.data_ptr(), flag.data_ptr(), text.data_ptr(), T,
                                                              C.byref(total), sp), "k7"))
              report(f"k7_yolo_lines_rpt{variant}", 32 * E + 4 * (E + 1) + 20 * E + 8 * (E + 1) + E + T, med, mn, rows=E, text_bytes=T,
                   rows_per_s=round(E / med * 1e3), no_line_rows=int((flag == 1).sum().item()))
            if "measure" not in modes:
                continue
            med, mn = timeit(lambda: ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), one.data_ptr(), None, w.data_ptr(), h.data_ptr(),
                                                              cid.data_ptr(), E, E, toff.data_ptr(), flag.data_ptr(), None, 0,
                                                              C.byref(total), sp), "k7"))
            report(f"k7_measure_only_rpt{variant}", 32 * E + 4 * (E + 1) + 20 * E + 8 * (E + 1) + E, med, mn, rows=E)
        # rows of many boxes (unsplit sheets: 1..32 lines per row): the generic path of the kernel
        wr = torch.full((N,), 1920.0, dtype=torch.float64, device=dev); hr = torch.full((N,), 1080.0, dtype=torch.float64, device=dev)
        cidr = (torch.arange(N, device=dev, dtype=torch.int32) % 20).contiguous()
        toffr = torch.empty(N + 1, dtype=torch.int64, device=dev); flagr = torch.empty(N, dtype=torch.uint8, device=dev)
        ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), box_off.data_ptr(), None, wr.data_ptr(), hr.data_ptr(), cidr.data_ptr(), N, B,
                                toffr.data_ptr(), flagr.data_ptr(), None, 0, C.byref(total), sp), "k7 measure")
        Tr = total.value
        textr = torch.empty(Tr, dtype=torch.uint8, device=dev)
        for variant in [int(v) for v in os.environ.get("K7VM", "30,-1").split(",")]:   # 22: 330 ms per launch
            ck(L.dyd_set_option(b"k7_variant", variant), "opt")
            med, mn = timeit(lambda: ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), box_off.data_ptr(), None, wr.data_ptr(), hr.data_ptr(),
                                                              cidr.data_ptr(), N, B, toffr.data_ptr(), flagr.data_ptr(), textr.data_ptr(), Tr,
                                                              C.byref(total), sp), "k7"))
            report(f"k7_yolo_lines_multi_box_rows_v{variant}", 32 * B + 4 * (N + 1) + 20 * N + 8 * (N + 1) + N + Tr, med, mn, rows=N, lines=B,
                   text_bytes=Tr, lines_per_s=round(B / med * 1e3))
        ck(L.dyd_set_option(b"k7_variant", -1), "opt")
    if "k13" in only:
        import ctypes as C
        # K13 beside K7 on the same polygons.  Shapes: the split's record shape (one polygon per row: the 10 M-row table's 165 M
        # polygons as 165 M rows, K7's "165 M records") and the synthetic rows as they are (U{1..32} polygons per row).
        # Bytes: in 16*P + 4*(B+1) + B + 4*(N+1) + 20*N, out 8*(N+1) + N + B + T.
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        total = C.c_int64()
        act = torch.empty(B, dtype=torch.uint8, device=dev)

        def shapes():
            one = torch.arange(B + 1, dtype=torch.int32, device=dev)
            yield "records", one, B
            yield "rows", box_off, N

        for shape, roff, nr in shapes():
            w = torch.full((nr,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((nr,), 1080.0, dtype=torch.float64, device=dev)
            cid = (torch.arange(nr, device=dev, dtype=torch.int32) % 20).contiguous()
            toff = torch.empty(nr + 1, dtype=torch.int64, device=dev); flag = torch.empty(nr, dtype=torch.uint8, device=dev)
            seg_args = (xy.data_ptr(), pt_off.data_ptr(), roff.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), nr, B, P,
                        toff.data_ptr(), flag.data_ptr(), act.data_ptr())
            ck(L.dyd_yolo_seg_lines_dev(*seg_args, None, 0, C.byref(total), sp), "k13 measure")
            T13 = total.value
            text = torch.empty(T13, dtype=torch.uint8, device=dev)
            counts = torch.bincount(act.to(torch.int64), minlength=256)[:6].tolist()
            ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), roff.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), nr, B,
                                    toff.data_ptr(), flag.data_ptr(), None, 0, C.byref(total), sp), "k7 measure")
            T7 = total.value
            text7 = torch.empty(T7, dtype=torch.uint8, device=dev)
            res = {}
            for rnd in range(2):                      # interleaved rounds
                res.setdefault("k7", []).append(timeit(lambda: ck(L.dyd_yolo_lines_dev(
                    out_box.data_ptr(), roff.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), nr, B, toff.data_ptr(),
                    flag.data_ptr(), text7.data_ptr(), T7, C.byref(total), sp), "k7")))
                res.setdefault("k13", []).append(timeit(lambda: ck(L.dyd_yolo_seg_lines_dev(*seg_args, text.data_ptr(), T13,
                                                                                            C.byref(total), sp), "k13")))
            k7_bytes = 32 * B + 4 * (nr + 1) + 20 * nr + 8 * (nr + 1) + nr + T7
            k13_bytes = 16 * P + 4 * (B + 1) + B + 4 * (nr + 1) + 20 * nr + 8 * (nr + 1) + nr + B + T13
            med7, mn7 = min(res["k7"])
            med13, mn13 = min(res["k13"])
            report(f"k7_yolo_lines_{shape}", k7_bytes, med7, mn7, rows=nr, lines=B, text_bytes=T7)
            report(f"k13_yolo_seg_lines_{shape}", k13_bytes, med13, mn13, rows=nr, polygons=B, points=P, text_bytes=T13,
                   actions=dict(zip(("written", "clipped", "bad_coords", "too_few_points", "empty", "no_size"), counts)),
                   bytes_per_s_vs_k7=round((k13_bytes / med13) / (k7_bytes / med7), 3))
            del text, text7
        # every polygon clipped: the same polygons moved 60 px left, record shape
        xs = xy.clone(); xs[:, 0] -= 60.0
        first = pt_off[:-1].to(torch.int64)
        xs[first, 0] = torch.clamp(xs[first, 0], max=-1.0)          # each polygon's first vertex outside
        one = torch.arange(B + 1, dtype=torch.int32, device=dev)
        w = torch.full((B,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((B,), 1080.0, dtype=torch.float64, device=dev)
        cid = (torch.arange(B, device=dev, dtype=torch.int32) % 20).contiguous()
        toff = torch.empty(B + 1, dtype=torch.int64, device=dev); flag = torch.empty(B, dtype=torch.uint8, device=dev)
        seg_args = (xs.data_ptr(), pt_off.data_ptr(), one.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), B, B, P,
                    toff.data_ptr(), flag.data_ptr(), act.data_ptr())
        ck(L.dyd_yolo_seg_lines_dev(*seg_args, None, 0, C.byref(total), sp), "k13 measure")
        T13 = total.value
        text = torch.empty(T13, dtype=torch.uint8, device=dev)
        med, mn = timeit(lambda: ck(L.dyd_yolo_seg_lines_dev(*seg_args, text.data_ptr(), T13, C.byref(total), sp), "k13"))
        counts = torch.bincount(act.to(torch.int64), minlength=256)[:6].tolist()
        report("k13_yolo_seg_lines_records_all_clipped", 16 * P + 4 * (B + 1) + B + 4 * (B + 1) + 20 * B + 8 * (B + 1) + B + B + T13,
               med, mn, rows=B, text_bytes=T13,
               actions=dict(zip(("written", "clipped", "bad_coords", "too_few_points", "empty", "no_size"), counts)))
        del xs, text
    if "tile" in only:
        import ctypes as C
        # K20 (tiled label lines) beside K13 on the same device buffers: the synthetic rows as they are, every image 1920 x 1080,
        # tile 640 with overlap 0.2 (step 512): a grid of 4 x 2 tiles per row.  K13 reads the same polygons once and prints each
        # once; K20 clips a polygon once per tile it reaches and prints it in each.  pairs = tile-polygon pairs with a part in the tile.
        tile, step = args.tile, max(1, args.tile - int(args.tile * args.overlap))
        total, n_tiles = C.c_int64(), C.c_int64()
        w = torch.full((N,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((N,), 1080.0, dtype=torch.float64, device=dev)
        cid = (torch.arange(N, device=dev, dtype=torch.int32) % 20).contiguous()
        cls = (torch.arange(B, device=dev, dtype=torch.int32) % 20).contiguous()
        toff = torch.empty(N + 1, dtype=torch.int64, device=dev); flag = torch.empty(N, dtype=torch.uint8, device=dev)
        act = torch.empty(B, dtype=torch.uint8, device=dev)
        seg_args = (xy.data_ptr(), pt_off.data_ptr(), box_off.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), N, B, P,
                    toff.data_ptr(), flag.data_ptr(), act.data_ptr())
        ck(L.dyd_yolo_seg_lines_dev(*seg_args, None, 0, C.byref(total), sp), "k13 measure")
        T13 = total.value
        text13 = torch.empty(T13, dtype=torch.uint8, device=dev)
        nx = 1 if 1920 <= tile else -((tile - 1920) // step) + 1
        ny = 1 if 1080 <= tile else -((tile - 1080) // step) + 1
        cap = N * nx * ny
        status = torch.empty(N, dtype=torch.uint8, device=dev); tile_off = torch.empty(N + 1, dtype=torch.int64, device=dev)
        lines = torch.empty(cap, dtype=torch.int32, device=dev); xoff = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        act20 = torch.empty(B, dtype=torch.uint8, device=dev)
        wr, cut, drop = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
        for mode, task in ((0, "segment"), (1, "detect")):
            a20 = (xy.data_ptr(), pt_off.data_ptr(), box_off.data_ptr(), cls.data_ptr(), w.data_ptr(), h.data_ptr(), N, B, P, tile, tile,
                   step, step, 0.1, mode, 4096, cap, status.data_ptr(), tile_off.data_ptr(), lines.data_ptr(), xoff.data_ptr(),
                   act20.data_ptr(), wr.data_ptr(), cut.data_ptr(), drop.data_ptr(), C.byref(n_tiles))
            ck(L.dyd_yolo_tile_lines_dev(*a20, None, 0, C.byref(total), sp), "k20 measure")
            T20 = total.value
            text20 = torch.empty(T20, dtype=torch.uint8, device=dev)
            res = {}
            for rnd in range(2):                      # interleaved rounds
                res.setdefault("k13", []).append(timeit(lambda: ck(L.dyd_yolo_seg_lines_dev(*seg_args, text13.data_ptr(), T13,
                                                                                            C.byref(total), sp), "k13")))
                res.setdefault("k20m", []).append(timeit(lambda: ck(L.dyd_yolo_tile_lines_dev(*a20, None, 0, C.byref(total), sp),
                                                                    "k20 measure")))
                res.setdefault("k20", []).append(timeit(lambda: ck(L.dyd_yolo_tile_lines_dev(*a20, text20.data_ptr(), T20,
                                                                                             C.byref(total), sp), "k20")))
            pairs = int(wr.sum().item() + drop.sum().item())
            k13_bytes = 16 * P + 4 * (B + 1) + B + 4 * (N + 1) + 20 * N + 8 * (N + 1) + N + B + T13
            k20_bytes = 16 * P + 4 * (B + 1) + 4 * B + 4 * (N + 1) + 16 * N + N + 8 * (N + 1) + 12 * n_tiles.value + 13 * B + T20
            med13, mn13 = min(res["k13"])
            med20, mn20 = min(res["k20"])
            medm, mnm = min(res["k20m"])
            report("k13_yolo_seg_lines_rows", k13_bytes, med13, mn13, rows=N, polygons=B, points=P, text_bytes=T13)
            report(f"k20_yolo_tile_lines_{task}_measure_only", k20_bytes - T20, medm, mnm, rows=N, tiles=n_tiles.value)
            report(f"k20_yolo_tile_lines_{task}", k20_bytes, med20, mn20, rows=N, polygons=B, points=P, tile=tile, step=step,
                   tiles=n_tiles.value, pairs=pairs, lines=int(wr.sum().item()), lines_cut=int(cut.sum().item()), text_bytes=T20,
                   ms_vs_k13=round(med20 / med13, 3), pairs_per_polygon=round(pairs / B, 3), text_vs_k13=round(T20 / max(T13, 1), 3))
            del text20
        del text13
    def raster_shapes():
        """the two tables of the k21 and k22 legs -> (name, xy, pt_off, row_off, rows, polygons, points, W, H)"""
        nr = min(N, 8192)
        nb_s = int(box_off[nr].item()); np_s = int(pt_off[nb_s].item())
        xs = (xy[:np_s] * torch.tensor([256.0 / 1920.0, 144.0 / 1080.0], dtype=torch.float64, device=dev)).contiguous()
        yield "small_images", xs, pt_off[:nb_s + 1].contiguous(), box_off[:nr + 1].contiguous(), nr, nb_s, np_s, 256, 144
        del xs
        rng = np.random.default_rng(21)
        m, rings = 2000, []
        for q in range(32):
            ang = np.sort(rng.uniform(0, 2 * np.pi, m))
            rad = rng.uniform(600, 1800, 1) * (1 + 0.3 * np.sin(ang * rng.integers(3, 40)) + rng.uniform(-0.05, 0.05, m))
            c = rng.uniform(1000, 3096, 2)
            rings.append(np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], axis=1))
        xl = torch.from_numpy(np.concatenate(rings)).to(dev)
        ptl = torch.arange(0, 32 * m + 1, m, dtype=torch.int32, device=dev)
        rol = torch.arange(0, 33, 4, dtype=torch.int32, device=dev)
        yield "large_images", xl, ptl, rol, 8, 32, 32 * m, 4096, 4096

    def compare_polygon_tables(xy_, pt_, roff, nr, nb, nc):
        """table B of the k22 and k25 legs from table A: 10 % of the polygons dropped, 10 % with jittered vertices, 5 % put into
        another class -> (A's row_off, A's cls, B's xy [P, 2], pt_off, row_off, cls, the draw u of the kept polygons), numpy"""
        rng = np.random.default_rng(22)
        hx, hp, hr = xy_.cpu().numpy().reshape(-1, 2), pt_.cpu().numpy().astype(np.int64), roff.cpu().numpy().astype(np.int64)
        u = rng.random(nb)
        keep = np.flatnonzero(u >= 0.10)
        cls_a = (np.arange(nb) % nc).astype(np.int32)
        cls_b = np.where(u[keep] >= 0.95, (cls_a[keep] + 1) % nc, cls_a[keep]).astype(np.int32)
        cnt = np.diff(hp)[keep]
        pb = np.concatenate([[0], np.cumsum(cnt)])
        src = np.repeat(hp[:-1][keep] - pb[:-1], cnt) + np.arange(int(pb[-1]))
        xb = hx[src].copy()
        jit = np.repeat((u[keep] >= 0.10) & (u[keep] < 0.20), cnt)
        xb[jit] += rng.uniform(-2.0, 2.0, (int(jit.sum()), 2))
        rb = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(hr, keep, side="right") - 1, minlength=nr))])
        return hr, cls_a, xb, pb, rb, cls_b, u[keep]

    if "k21" in only:
        import ctypes as C
        import time
        # K21 (label masks): measure-only and full, ms, pixels/s and bytes moved (1 byte written per pixel, the table read once,
        # the small outputs), on two tables: many small images (the first rows of the synthetic table, the k20 leg's polygon mix,
        # scaled from 1920 x 1080 to 256 x 144) and few large images (8 of 4096 x 4096 with 4 outlines of 2000 vertices each).
        # Beside them, as a yardstick of time only (its fill rule differs, so its pixels are not compared), Pillow's
        # ImageDraw.polygon over the same tables on one core.
        total = C.c_int64()

        def k21_leg(name, xy_, pt_, roff, nr, nb, npts, W, H):
            w = torch.full((nr,), float(W), dtype=torch.float64, device=dev); h = torch.full((nr,), float(H), dtype=torch.float64, device=dev)
            val = (torch.arange(nb, device=dev, dtype=torch.int32) % 20 + 1).contiguous()
            status = torch.empty(nr, dtype=torch.uint8, device=dev); poff = torch.empty(nr + 1, dtype=torch.int64, device=dev)
            act = torch.empty(nb, dtype=torch.uint8, device=dev)
            cov = torch.empty(nb, dtype=torch.int64, device=dev); own = torch.empty(nb, dtype=torch.int64, device=dev)
            a21 = (xy_.data_ptr(), pt_.data_ptr(), roff.data_ptr(), val.data_ptr(), w.data_ptr(), h.data_ptr(), nr, nb, npts, 0, 1 << 26,
                   status.data_ptr(), poff.data_ptr(), act.data_ptr(), cov.data_ptr(), own.data_ptr())
            ck(L.dyd_rasterize_polygons_dev(*a21, None, 0, C.byref(total), sp), "k21 measure")
            T = total.value
            pix = torch.empty(T, dtype=torch.uint8, device=dev)
            medm, mnm = timeit(lambda: ck(L.dyd_rasterize_polygons_dev(*a21, None, 0, C.byref(total), sp), "k21 measure"))
            med, mn = timeit(lambda: ck(L.dyd_rasterize_polygons_dev(*a21, pix.data_ptr(), T, C.byref(total), sp), "k21"))
            table_bytes = 16 * npts + 4 * (nb + 1) + 4 * nb + 4 * (nr + 1) + 16 * nr
            small_out = nr + 8 * (nr + 1) + nb
            report(f"k21_rasterize_{name}_measure_only", table_bytes + small_out, medm, mnm, rows=nr, pixels=T)
            painted = int((pix != 0).sum().item())
            # Pillow on one core over the same table
            from PIL import Image, ImageDraw
            hx, hp, hr, hv = xy_.cpu().numpy(), pt_.cpu().numpy(), roff.cpu().numpy(), val.cpu().numpy()
            t0 = time.perf_counter()
            for i in range(nr):
                im = Image.new("L", (W, H), 0)
                draw = ImageDraw.Draw(im)
                for q in range(hr[i], hr[i + 1]):
                    pts = hx[hp[q]:hp[q + 1]]
                    if len(pts) == 2:
                        draw.rectangle([tuple(pts.min(0)), tuple(pts.max(0))], fill=int(hv[q]))
                    elif len(pts) > 2:
                        draw.polygon(pts.reshape(-1).tolist(), fill=int(hv[q]))
            pillow_ms = (time.perf_counter() - t0) * 1e3
            report(f"k21_rasterize_{name}", table_bytes + small_out + 16 * nb + T, med, mn, rows=nr, polygons=nb, points=npts, width=W,
                   height=H, pixels=T, painted_pixels=painted, covered_pixels=int(cov.sum().item()), Gpixels_per_s=round(T / med / 1e6, 2),
                   byte_floor_GB=round((table_bytes + T) / 1e9, 4), pillow_one_core_ms=round(pillow_ms, 1),
                   pillow_over_k21=round(pillow_ms / med, 1))

        for shape in raster_shapes():
            k21_leg(*shape)
    if "k22" in only:
        import ctypes as C
        # K22 (polygon comparison by mask IoU) on the k21 leg's two tables.  B is A with 10 % of the polygons dropped, 10 % with
        # jittered vertices and 5 % put into another class (the k18 leg's proportions).  K22 runs interleaved with K21 over A and
        # K21 over B on the same device buffers, which is what the comparison would cost by two mask exports; the two mask
        # downloads that route also needs are timed beside them.  Byte floor: both tables read once, the pair table written.
        total = C.c_int64()
        nc = 20

        def k22_leg(name, xy_, pt_, roff, nr, nb, npts, W, H):
            hr, cls_a, xb, pb, rb, cls_b, _ = compare_polygon_tables(xy_, pt_, roff, nr, nb, nc)
            nbb, npb = len(cls_b), int(pb[-1])
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)   # noqa: E731
            b_xy, b_pt, b_row, d_ca, d_cb = up(xb.reshape(-1), np.float64), up(pb, np.int32), up(rb, np.int32), up(cls_a, np.int32), up(cls_b, np.int32)
            w = torch.full((nr,), float(W), dtype=torch.float64, device=dev); h = torch.full((nr,), float(H), dtype=torch.float64, device=dev)
            e = lambda n_, dt: torch.empty(max(n_, 1), dtype=dt, device=dev)                   # noqa: E731
            status, poff = e(nr, torch.uint8), e(nr + 1, torch.int64)
            outs_a = (e(nb, torch.uint8), e(nb, torch.int64), e(nb, torch.int32), e(nb, torch.float64))
            outs_b = (e(nbb, torch.uint8), e(nbb, torch.int64), e(nbb, torch.int32), e(nbb, torch.float64))
            b_iou, rows_, rpix = e(nbb, torch.float64), e(4 * nr, torch.int32), e(2 * nr, torch.int64)
            conf, pconf = e((nc + 1) ** 2, torch.int64), e((nc + 1) ** 2, torch.int64)
            n_pairs = int((np.diff(hr) * np.diff(rb)).sum())
            pairs = e(n_pairs, torch.int32)
            a22 = (xy_.data_ptr(), pt_.data_ptr(), roff.data_ptr(), d_ca.data_ptr(), b_xy.data_ptr(), b_pt.data_ptr(), b_row.data_ptr(),
                   d_cb.data_ptr(), w.data_ptr(), h.data_ptr(), nr, nb, npts, nbb, npb, nc, 0.5, 0, 1 << 26, 1 << 20, status.data_ptr(),
                   poff.data_ptr(), outs_a[0].data_ptr(), outs_b[0].data_ptr(), outs_a[1].data_ptr(), outs_b[1].data_ptr(),
                   outs_a[2].data_ptr(), outs_b[2].data_ptr(), b_iou.data_ptr(), outs_a[3].data_ptr(), outs_b[3].data_ptr(),
                   rows_.data_ptr(), conf.data_ptr(), pconf.data_ptr(), rpix.data_ptr(), pairs.data_ptr(), n_pairs, sp)
            T = nr * W * H
            pix = torch.empty(T, dtype=torch.uint8, device=dev)
            s21, p21 = torch.empty(nr, dtype=torch.uint8, device=dev), torch.empty(nr + 1, dtype=torch.int64, device=dev)
            val_a, val_b = d_ca + 1, d_cb + 1

            keepalive = []

            def k21_call(x, p, r, v, n_, np_):
                act_, own_ = e(n_, torch.uint8), e(n_, torch.int64)
                cov_ = e(n_, torch.int64)
                keepalive.extend([act_, own_, cov_])
                args21 = (x.data_ptr(), p.data_ptr(), r.data_ptr(), v.data_ptr(), w.data_ptr(), h.data_ptr(), nr, n_, np_, 0, 1 << 26,
                          s21.data_ptr(), p21.data_ptr(), act_.data_ptr(), cov_.data_ptr(), own_.data_ptr(), pix.data_ptr(), T,
                          C.byref(total), sp)
                return lambda: ck(L.dyd_rasterize_polygons_dev(*args21), "k21")

            legs = {"k21_a": k21_call(xy_, pt_, roff, val_a, nb, npts), "k21_b": k21_call(b_xy, b_pt, b_row, val_b, nbb, npb),
                    "k22": lambda: ck(L.dyd_compare_polygons_dev(*a22), "k22")}
            res = {}
            for rnd in range(2):                  # interleaved rounds (guide rule 24)
                for key, fn in legs.items():
                    res.setdefault(key, []).append(timeit(fn))
            med = {k: float(np.median([r[0] for r in v])) for k, v in res.items()}
            mn = {k: min(r[1] for r in v) for k, v in res.items()}
            host = torch.empty(T, dtype=torch.uint8).pin_memory()
            dl, _ = timeit(lambda: host.copy_(pix, non_blocking=True), iters=5, warm=1)
            table_bytes = 16 * (npts + npb) + 4 * (nb + nbb + 2) + 4 * (nb + nbb) + 8 * (nr + 1) + 16 * nr
            report(f"k22_compare_polygons_{name}", table_bytes + 4 * n_pairs + 29 * (nb + nbb) + 41 * nr, med["k22"], mn["k22"], rows=nr,
                   a_polygons=nb, b_polygons=nbb, a_points=npts, b_points=npb, width=W, height=H, pixels=T, pairs=n_pairs,
                   pairs_hit=int((pairs[:n_pairs] != 0).sum().item()) if n_pairs else 0, matched=int((outs_b[2][:nbb] >= 0).sum().item()),
                   Gpixels_per_s=round(T / med["k22"] / 1e6, 2), byte_floor_GB=round((table_bytes + 4 * n_pairs) / 1e9, 4),
                   k21_a_ms=round(med["k21_a"], 4), k21_b_ms=round(med["k21_b"], 4), mask_download_ms=round(dl, 4),
                   k22_over_two_k21=round(med["k22"] / (med["k21_a"] + med["k21_b"]), 3),
                   k22_over_two_k21_and_downloads=round(med["k22"] / (med["k21_a"] + med["k21_b"] + 2 * dl), 3))

        for shape in raster_shapes():
            k22_leg(*shape)
    if "k25" in only:
        # K25 (scored polygon evaluation) through its host entry on the k22 leg's two tables, B with a score of three decimals per
        # polygon, at T = 1 and T = 10; K22 through its host entry on the same tables in the same interleaved rounds is the
        # yardstick: K25 does K22's paint without the owners, the class-pair pass and the pairs of different classes, plus the
        # ranking.  Kernel time from dyd_last_kernel_ms, as in the k24 leg.
        nc = 20
        thr10 = np.linspace(0.5, 0.95, 10)

        def k25_leg(name, xy_, pt_, roff, nr, nb, npts, W, H):
            hr, cls_a, xb, pb, rb, cls_b, ub = compare_polygon_tables(xy_, pt_, roff, nr, nb, nc)
            nbb, npb = len(cls_b), int(pb[-1])
            score = np.round(ub * 0.37 % 1.0, 3)                         # three decimals: ties within and across rows
            tabs = (xy_.cpu().numpy().reshape(-1), pt_.cpu().numpy(), roff.cpu().numpy(), cls_a, xb.reshape(-1), pb.astype(np.int32),
                    rb.astype(np.int32), cls_b)
            w, h = np.full(nr, float(W)), np.full(nr, float(H))

            def kernel_ms(fn, iters=max(3, args.iters // 4)):
                fn()
                ts = []
                for _ in range(iters):
                    fn()
                    ts.append(_native.last_kernel_ms())
                return float(np.median(ts)), float(np.min(ts))

            legs = {"k22": lambda: _native.compare_polygons(*tabs, w, h, nc, 0.5, False),
                    "k25 T=1": lambda: _native.eval_match_polygons(*tabs, score, w, h, nc, [0.5], 100),
                    "k25 T=10": lambda: _native.eval_match_polygons(*tabs, score, w, h, nc, thr10, 100)}
            res = {}
            for rnd in range(2):                  # interleaved rounds (guide rule 24)
                for key, fn in legs.items():
                    res.setdefault(key, []).append(kernel_ms(fn))
            med = {k: float(np.median([r[0] for r in v])) for k, v in res.items()}
            mn = {k: min(r[1] for r in v) for k, v in res.items()}
            out = legs["k25 T=10"]()
            n_pairs = int(out[1][-1])
            table_bytes = 16 * (npts + npb) + 4 * (nb + nbb + 2) + 4 * (nb + nbb) + 8 * (nr + 1) + 16 * nr + 8 * nbb
            for key, T_ in (("k25 T=1", 1), ("k25 T=10", 10)):
                report(f"k25_eval_match_polygons_{name} T={T_}", table_bytes + 4 * n_pairs + 21 * nb + 37 * nbb + 9 * nr, med[key], mn[key],
                       rows=nr, gt_polygons=nb, detections=nbb, width=W, height=H, pixels=nr * W * H, pairs=n_pairs,
                       evaluated=int((out[6] == 0).sum()), tp_at_first=int((out[7] & 1).sum()),
                       k22_host_entry_ms=round(med["k22"], 4), k22_host_entry_min_ms=round(mn["k22"], 4),
                       k25_over_k22=round(med[key] / med["k22"], 3))

        for shape in raster_shapes():
            k25_leg(*shape)
    if "k23" in only:
        import ctypes as C
        # K23 (COCO run-length masks) on the k21 leg's two tables: measure-only (status, action, area, bbox, run_off) and full
        # (runs and strings too), with the runs and the bytes that come out, interleaved with K21 over the same table as a
        # yardstick: K21's cost follows the image, K23's the polygons' boxes.  The entry takes no stream: it runs on the library's
        # own stream and is blocking, so it is timed by the host's clock round the call, K21 beside it in the same way.
        import time
        n_runs, n_text, total = C.c_int64(), C.c_int64(), C.c_int64()

        def wall(fn, iters=10, warm=2):
            for _ in range(warm):
                fn()
            ts = []
            for _ in range(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts)), float(min(ts))

        def k23_leg(name, xy_, pt_, roff, nr, nb, npts, W, H):
            w = torch.full((nr,), float(W), dtype=torch.float64, device=dev); h = torch.full((nr,), float(H), dtype=torch.float64, device=dev)
            sel = (torch.arange(nb, device=dev, dtype=torch.int32) % 20).contiguous()
            e = lambda n_, dt: torch.empty(max(n_, 1), dtype=dt, device=dev)                   # noqa: E731
            status, act, area, bbox = e(nr, torch.uint8), e(nb, torch.uint8), e(nb, torch.int64), e(4 * nb, torch.int32)
            roff_, toff_ = e(nb + 1, torch.int64), e(nb + 1, torch.int64)
            a23 = (xy_.data_ptr(), pt_.data_ptr(), roff.data_ptr(), sel.data_ptr(), w.data_ptr(), h.data_ptr(), nr, nb, npts, 1 << 26,
                   status.data_ptr(), act.data_ptr(), area.data_ptr(), bbox.data_ptr(), roff_.data_ptr())
            torch.cuda.synchronize()
            ck(L.dyd_polygon_rle_dev(*a23, None, 0, None, None, 0, C.byref(n_runs), C.byref(n_text)), "k23 measure")
            R = n_runs.value
            runs = e(R, torch.int32)
            ck(L.dyd_polygon_rle_dev(*a23, runs.data_ptr(), R, toff_.data_ptr(), None, 0, C.byref(n_runs), C.byref(n_text)), "k23 runs")
            T = n_text.value
            text = e(T, torch.uint8)
            val = sel + 1
            P21 = nr * W * H
            pix = e(P21, torch.uint8)
            s21, p21, a21_, c21, o21 = e(nr, torch.uint8), e(nr + 1, torch.int64), e(nb, torch.uint8), e(nb, torch.int64), e(nb, torch.int64)
            args21 = (xy_.data_ptr(), pt_.data_ptr(), roff.data_ptr(), val.data_ptr(), w.data_ptr(), h.data_ptr(), nr, nb, npts, 0, 1 << 26,
                      s21.data_ptr(), p21.data_ptr(), a21_.data_ptr(), c21.data_ptr(), o21.data_ptr(), pix.data_ptr(), P21,
                      C.byref(total), sp)
            legs = {"k21": lambda: ck(L.dyd_rasterize_polygons_dev(*args21), "k21"),
                    "k23m": lambda: ck(L.dyd_polygon_rle_dev(*a23, None, 0, None, None, 0, C.byref(n_runs), C.byref(n_text)), "k23 measure"),
                    "k23": lambda: ck(L.dyd_polygon_rle_dev(*a23, runs.data_ptr(), R, toff_.data_ptr(), text.data_ptr(), T,
                                                            C.byref(n_runs), C.byref(n_text)), "k23")}
            res = {}
            for rnd in range(2):                  # interleaved rounds (guide rule 24)
                for key, fn in legs.items():
                    res.setdefault(key, []).append(wall(fn))
            med = {k: float(np.median([r[0] for r in v])) for k, v in res.items()}
            mn = {k: min(r[1] for r in v) for k, v in res.items()}
            assert int(area.sum().item()) == int(c21.sum().item()), "K23's areas are not K21's covered counts"
            table_bytes = 16 * npts + 4 * (nb + 1) + 4 * nb + 4 * (nr + 1) + 16 * nr
            small_out = nr + nb + 8 * nb + 16 * nb + 8 * (nb + 1)
            span = bbox.view(-1, 4)
            report(f"k23_polygon_rle_{name}_measure_only", table_bytes + small_out, med["k23m"], mn["k23m"], rows=nr, polygons=nb, runs=R,
                   host_clock=True)
            report(f"k23_polygon_rle_{name}", table_bytes + small_out + 8 * (nb + 1) + 4 * R + T, med["k23"], mn["k23"], rows=nr, polygons=nb,
                   points=npts, width=W, height=H, runs=R, text_bytes=T, bytes_out=small_out + 8 * (nb + 1) + 4 * R + T,
                   covered_pixels=int(area.sum().item()), box_columns=int(span[:, 2].sum().item()), image_pixels=P21,
                   mask_bytes_k21=P21, k21_ms=round(med["k21"], 4), k21_min_ms=round(mn["k21"], 4),
                   k23_over_k21=round(med["k23"] / med["k21"], 3), host_clock=True)

        for shape in raster_shapes():
            k23_leg(*shape)
    if "k14" in only:
        import ctypes as C
        # K14 (polygon audit) on K13's two shapes, and long polygons (convex rings of 256 vertices: no crossing, so the wave
        # tier tests every edge pair).  Bytes: in 16*P + 4*(B+1) + 4*B + 4*(N+1) + 17*N, out 10*B + the class counters.
        nc = 20
        cat = torch.empty(B, dtype=torch.uint8, device=dev); dfc = torch.empty(B, dtype=torch.uint8, device=dev)
        area = torch.empty(B, dtype=torch.float64, device=dev)
        cc = torch.empty((nc, 14), dtype=torch.int64, device=dev); hist = torch.empty((nc, 11), dtype=torch.int64, device=dev)

        def k14_leg(name, xy_, pt_, roff, nr, nb, npts):
            w = torch.full((nr,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((nr,), 1080.0, dtype=torch.float64, device=dev)
            st = torch.zeros(nr, dtype=torch.uint8, device=dev)
            cls = (torch.arange(nb, device=dev, dtype=torch.int32) % nc).contiguous()
            a14 = (xy_.data_ptr(), pt_.data_ptr(), roff.data_ptr(), cls.data_ptr(), w.data_ptr(), h.data_ptr(), st.data_ptr(), nr, nb,
                   npts, nc, 1.0, cat.data_ptr(), dfc.data_ptr(), area.data_ptr(), cc.data_ptr(), hist.data_ptr(), sp)
            med, mn = timeit(lambda: ck(L.dyd_audit_polygons_dev(*a14), "k14"))
            c = cc.sum(0).tolist()
            report(f"k14_audit_polygons_{name}", 16 * npts + 4 * (nb + 1) + 4 * nb + 4 * (nr + 1) + 17 * nr + 10 * nb, med, mn,
                   rows=nr, polygons=nb, points=npts, polygons_per_s=round(nb / med * 1e3),
                   categories=dict(zip(("written", "clipped", "bad_coords", "too_few_points", "empty", "no_size"), c[2:8])),
                   defects=dict(zip(("duplicate_vertices", "self_intersecting", "tiny_area"), c[8:11])))

        k14_leg("records", xy, pt_off, torch.arange(B + 1, dtype=torch.int32, device=dev), B, B, P)
        k14_leg("rows", xy, pt_off, box_off, N, B, P)
        nl, m = 1_000_000, 256
        th = torch.arange(m, dtype=torch.float64, device=dev) * (2 * np.pi / m)
        ring = torch.stack([500.0 + 400.0 * torch.cos(th), 500.0 + 400.0 * torch.sin(th)], 1)
        xl = ring.repeat(nl, 1).contiguous()
        ptl = torch.arange(nl + 1, dtype=torch.int32, device=dev) * m
        k14_leg("long_256", xl, ptl, torch.arange(nl + 1, dtype=torch.int32, device=dev), nl, nl, nl * m)
        del xl, cat, dfc, area
    if "k16" in only:
        import ctypes as C
        # K16 (COCO annotation objects) beside K13 on K13's two shapes, rounds interleaved.  K16 bytes: in 16*P + 4*(B+1) + 4*B +
        # 4*(N+1) + 17*N, out 9*B + 4*N + T; K13 bytes as in its leg.
        total = C.c_int64()
        act = torch.empty(B, dtype=torch.uint8, device=dev)
        area = torch.empty(B, dtype=torch.float64, device=dev)
        cat = (torch.arange(B, device=dev, dtype=torch.int32) % 20 + 1).contiguous()
        for shape, roff, nr in (("records", torch.arange(B + 1, dtype=torch.int32, device=dev), B), ("rows", box_off, N)):
            w = torch.full((nr,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((nr,), 1080.0, dtype=torch.float64, device=dev)
            st = torch.zeros(nr, dtype=torch.uint8, device=dev)
            cid = (torch.arange(nr, device=dev, dtype=torch.int32) % 20).contiguous()
            toff = torch.empty(nr + 1, dtype=torch.int64, device=dev); flag = torch.empty(nr, dtype=torch.uint8, device=dev)
            kept = torch.empty(nr, dtype=torch.int32, device=dev)
            seg_args = (xy.data_ptr(), pt_off.data_ptr(), roff.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), nr, B, P,
                        toff.data_ptr(), flag.data_ptr(), act.data_ptr())
            ck(L.dyd_yolo_seg_lines_dev(*seg_args, None, 0, C.byref(total), sp), "k13 measure")
            T13 = total.value
            text13 = torch.empty(T13, dtype=torch.uint8, device=dev)
            for flags, name in ((1, "segment"), (0, "detect")):
                coco_args = (xy.data_ptr(), pt_off.data_ptr(), roff.data_ptr(), cat.data_ptr(), w.data_ptr(), h.data_ptr(), st.data_ptr(),
                             nr, B, P, 1, 1, flags, act.data_ptr(), area.data_ptr(), kept.data_ptr())
                ck(L.dyd_coco_annotations_dev(*coco_args, None, 0, C.byref(total), sp), "k16 measure")
                T16 = total.value
                counts = torch.bincount(act.to(torch.int64), minlength=256)[:7].tolist()
                text16 = torch.empty(T16, dtype=torch.uint8, device=dev)
                res = {}
                for rnd in range(2):                  # interleaved rounds
                    res.setdefault("k13", []).append(timeit(lambda: ck(L.dyd_yolo_seg_lines_dev(*seg_args, text13.data_ptr(), T13,
                                                                                                C.byref(total), sp), "k13")))
                    res.setdefault("k16", []).append(timeit(lambda: ck(L.dyd_coco_annotations_dev(*coco_args, text16.data_ptr(), T16,
                                                                                                  C.byref(total), sp), "k16")))
                k13_bytes = 16 * P + 4 * (B + 1) + B + 4 * (nr + 1) + 20 * nr + 8 * (nr + 1) + nr + B + T13
                k16_bytes = 16 * P + 4 * (B + 1) + 4 * B + 4 * (nr + 1) + 17 * nr + 9 * B + 4 * nr + T16
                med13, mn13 = min(res["k13"])
                med16, mn16 = min(res["k16"])
                report(f"k13_yolo_seg_lines_{shape}", k13_bytes, med13, mn13, rows=nr, polygons=B, points=P, text_bytes=T13)
                report(f"k16_coco_{name}_{shape}", k16_bytes, med16, mn16, rows=nr, polygons=B, points=P, text_bytes=T16,
                       actions=dict(zip(("written", "clipped", "bad_coords", "too_few_points", "empty", "no_size", "too_large"), counts)),
                       bytes_per_s_vs_k13=round((k16_bytes / med16) / (k13_bytes / med13), 3))
                del text16
            del text13
        del act, area, cat
    if "k17" in only:
        import ctypes as C
        # K17 (oriented-box lines) beside K13 on K13's two shapes, rounds interleaved, then long polygons (K14's long_256 rings,
        # a tenth as many: every vertex is a hull vertex, so a lane makes 258 passes over its 256 points).  K17 bytes: in as K13,
        # out 8*(N+1) + N + 2*B + T (the 64*B of corners stay inside the library when the caller asks for none).
        total = C.c_int64()
        names17 = ("written", "clipped", "bad_coords", "too_few_points", "empty", "no_size", "flat")

        def k17_leg(shape, xy_, pt_, roff, nr, nb, npts, with_k13=True, iters=args.iters):
            w = torch.full((nr,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((nr,), 1080.0, dtype=torch.float64, device=dev)
            cid = (torch.arange(nr, device=dev, dtype=torch.int32) % 20).contiguous()
            toff = torch.empty(nr + 1, dtype=torch.int64, device=dev); flag = torch.empty(nr, dtype=torch.uint8, device=dev)
            act = torch.empty(nb, dtype=torch.uint8, device=dev); cl = torch.empty(nb, dtype=torch.uint8, device=dev)
            seg_args = (xy_.data_ptr(), pt_.data_ptr(), roff.data_ptr(), None, w.data_ptr(), h.data_ptr(), cid.data_ptr(), nr, nb, npts,
                        toff.data_ptr(), flag.data_ptr(), act.data_ptr())
            obb_args = seg_args + (cl.data_ptr(), None)
            ck(L.dyd_yolo_obb_lines_dev(*obb_args, None, 0, C.byref(total), sp), "k17 measure")
            T17 = total.value
            counts = torch.bincount(act.to(torch.int64), minlength=256)[:7].tolist()
            text17 = torch.empty(T17, dtype=torch.uint8, device=dev)
            ck(L.dyd_yolo_seg_lines_dev(*seg_args, None, 0, C.byref(total), sp), "k13 measure")
            T13 = total.value
            text13 = torch.empty(T13, dtype=torch.uint8, device=dev)
            res = {}
            for rnd in range(2):                      # interleaved rounds
                if with_k13:
                    res.setdefault("k13", []).append(timeit(lambda: ck(L.dyd_yolo_seg_lines_dev(*seg_args, text13.data_ptr(), T13,
                                                                                                C.byref(total), sp), "k13"), iters=iters))
                res.setdefault("k17", []).append(timeit(lambda: ck(L.dyd_yolo_obb_lines_dev(*obb_args, text17.data_ptr(), T17,
                                                                                            C.byref(total), sp), "k17"), iters=iters))
            base = 16 * npts + 4 * (nb + 1) + nb + 4 * (nr + 1) + 20 * nr + 8 * (nr + 1) + nr
            k17_bytes = base + 2 * nb + T17
            med17, mn17 = min(res["k17"])
            extra = {}
            if with_k13:
                k13_bytes = base + nb + T13
                med13, mn13 = min(res["k13"])
                report(f"k13_yolo_seg_lines_{shape}", k13_bytes, med13, mn13, rows=nr, polygons=nb, points=npts, text_bytes=T13)
                extra = {"bytes_per_s_vs_k13": round((k17_bytes / med17) / (k13_bytes / med13), 3), "ms_vs_k13": round(med17 / med13, 3)}
            report(f"k17_yolo_obb_lines_{shape}", k17_bytes, med17, mn17, rows=nr, polygons=nb, points=npts, text_bytes=T17,
                   polygons_per_s=round(nb / med17 * 1e3), clamped=int(cl.sum().item()), actions=dict(zip(names17, counts)), **extra)

        k17_leg("records", xy, pt_off, torch.arange(B + 1, dtype=torch.int32, device=dev), B, B, P)
        k17_leg("rows", xy, pt_off, box_off, N, B, P)
        nl, m = 100_000, 256
        th = torch.arange(m, dtype=torch.float64, device=dev) * (2 * np.pi / m)
        ring = torch.stack([500.0 + 400.0 * torch.cos(th), 500.0 + 400.0 * torch.sin(th)], 1)
        xl = ring.repeat(nl, 1).contiguous()
        k17_leg("long_256", xl, torch.arange(nl + 1, dtype=torch.int32, device=dev) * m, torch.arange(nl + 1, dtype=torch.int32, device=dev),
                nl, nl, nl * m, iters=3)
        del xl
    if "k14tier" in only:
        import ctypes as C
        # K14's tier threshold: 1 M convex rings of m vertices (no crossing: every edge pair tested) with the in-lane limit
        # ("k14_lane_edges") below and above m, so each m runs once in its lane and once on the wave tier
        nl, nc = 1_000_000, 20
        cat = torch.empty(nl, dtype=torch.uint8, device=dev); dfc = torch.empty(nl, dtype=torch.uint8, device=dev)
        area = torch.empty(nl, dtype=torch.float64, device=dev)
        cc = torch.empty((nc, 14), dtype=torch.int64, device=dev); hist = torch.empty((nc, 11), dtype=torch.int64, device=dev)
        one = torch.arange(nl + 1, dtype=torch.int32, device=dev)
        w = torch.full((nl,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((nl,), 1080.0, dtype=torch.float64, device=dev)
        st = torch.zeros(nl, dtype=torch.uint8, device=dev)
        cls = (torch.arange(nl, device=dev, dtype=torch.int32) % nc).contiguous()
        for m in (8, 16, 24, 32, 48, 64, 96):
            th = torch.arange(m, dtype=torch.float64, device=dev) * (2 * np.pi / m)
            xl = torch.stack([500.0 + 400.0 * torch.cos(th), 500.0 + 400.0 * torch.sin(th)], 1).repeat(nl, 1).contiguous()
            ptl = one * m
            a14 = (xl.data_ptr(), ptl.data_ptr(), one.data_ptr(), cls.data_ptr(), w.data_ptr(), h.data_ptr(), st.data_ptr(), nl, nl,
                   nl * m, nc, 1.0, cat.data_ptr(), dfc.data_ptr(), area.data_ptr(), cc.data_ptr(), hist.data_ptr(), sp)
            for lim in (m - 1, m):
                ck(L.dyd_set_option(b"k14_lane_edges", lim), "opt")
                med, mn = timeit(lambda: ck(L.dyd_audit_polygons_dev(*a14), "k14"), iters=5)
                report(f"k14_tier_ring{m}_{'wave' if lim < m else 'lane'}", 16 * nl * m, med, mn, polygons=nl, vertices=m,
                       selfx=int(cc[:, 9].sum()))
            del xl
        ck(L.dyd_set_option(b"k14_lane_edges", 0), "opt")
    if "simplify" in only:
        # K19 beside K14 (which reads the same bytes) on rings of m jittered vertices, 2^24 points per table, tolerance 1
        nc, total_pts = 20, 1 << 24
        g = torch.Generator(device=dev).manual_seed(19)
        for m in (8, 64, 1024):
            nl = total_pts // m
            th = torch.arange(m, dtype=torch.float64, device=dev) * (2 * np.pi / m)
            rad = 400.0 + 1.4 * (torch.rand((nl, m), generator=g, device=dev, dtype=torch.float64) - 0.5)
            xl = torch.stack([500.0 + rad * torch.cos(th), 500.0 + rad * torch.sin(th)], 2).reshape(-1, 2).contiguous()
            del rad
            one = torch.arange(nl + 1, dtype=torch.int32, device=dev)
            ptl = (one * m).contiguous()
            keep = torch.empty(nl * m, dtype=torch.uint8, device=dev); act = torch.empty(nl, dtype=torch.uint8, device=dev)
            kept = torch.empty(nl, dtype=torch.int32, device=dev); dev2 = torch.empty(nl, dtype=torch.float64, device=dev)
            cat = torch.empty(nl, dtype=torch.uint8, device=dev); dfc = torch.empty(nl, dtype=torch.uint8, device=dev)
            area = torch.empty(nl, dtype=torch.float64, device=dev)
            cc = torch.empty((nc, 14), dtype=torch.int64, device=dev); hist = torch.empty((nc, 11), dtype=torch.int64, device=dev)
            w = torch.full((nl,), 1920.0, dtype=torch.float64, device=dev); h = torch.full((nl,), 1080.0, dtype=torch.float64, device=dev)
            st = torch.zeros(nl, dtype=torch.uint8, device=dev)
            cls = (torch.arange(nl, device=dev, dtype=torch.int32) % nc).contiguous()
            a19 = (xl.data_ptr(), ptl.data_ptr(), nl, nl * m, 1.0, keep.data_ptr(), act.data_ptr(), kept.data_ptr(), dev2.data_ptr(), sp)
            a14 = (xl.data_ptr(), ptl.data_ptr(), one.data_ptr(), cls.data_ptr(), w.data_ptr(), h.data_ptr(), st.data_ptr(), nl, nl,
                   nl * m, nc, 1.0, cat.data_ptr(), dfc.data_ptr(), area.data_ptr(), cc.data_ptr(), hist.data_ptr(), sp)
            res = {}
            for rnd in range(2):                      # interleaved rounds
                res.setdefault("k19", []).append(timeit(lambda: ck(L.dyd_simplify_polygons_dev(*a19), "k19"), iters=5))
                res.setdefault("k14", []).append(timeit(lambda: ck(L.dyd_audit_polygons_dev(*a14), "k14"), iters=5))
            nbytes = 16 * nl * m + 4 * (nl + 1) + nl * m + 13 * nl
            med19, mn19 = min(res["k19"])
            med14, mn14 = min(res["k14"])
            report(f"k14_audit_polygons_ring{m}", nbytes, med14, mn14, polygons=nl, vertices=m)
            if m == 64:                               # the same table with the lane tier raised to take it (default: LDS tier)
                ck(L.dyd_set_option(b"k19_lane_points", 64), "opt")
                medl, mnl = timeit(lambda: ck(L.dyd_simplify_polygons_dev(*a19), "k19"), iters=5)
                ck(L.dyd_set_option(b"k19_lane_points", 0), "opt")
                report("k19_simplify_polygons_ring64_in_lane", nbytes, medl, mnl, polygons=nl, vertices=m)
            report(f"k19_simplify_polygons_ring{m}", nbytes, med19, mn19, polygons=nl, vertices=m, tolerance=1.0,
                   kept_points=int(kept.sum().item()), simplified=int((act == 1).sum().item()), ms_vs_k14=round(med19 / med14, 3))
            del xl, keep
    if "k7mix" in only:
        # where the box-tiled kernel overtakes the row kernels: rows of one box with a share of two-box rows mixed in
        import ctypes as C
        ck(L.dyd_bbox_minmax_dev(xy.data_ptr(), pt_off.data_ptr(), B, P, out_box.data_ptr(), out_arg.data_ptr(), sp), "k1")
        g = torch.Generator(device=dev).manual_seed(9)
        total = C.c_int64()
        for share in (0.0, 0.05, 0.1, 0.25, 0.5, 1.0):
            nr = int(B / (1 + share))
            counts = (torch.rand(nr, generator=g, device=dev) < share).to(torch.int32) + 1
            ro = torch.zeros(nr + 1, dtype=torch.int32, device=dev)
            ro[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
            nbx = int(ro[-1].item())
            w2 = torch.full((nr,), 1920.0, dtype=torch.float64, device=dev); h2 = torch.full((nr,), 1080.0, dtype=torch.float64, device=dev)
            c2 = (torch.arange(nr, device=dev, dtype=torch.int32) % 20).contiguous()
            to2 = torch.empty(nr + 1, dtype=torch.int64, device=dev); fl2 = torch.empty(nr, dtype=torch.uint8, device=dev)
            ck(L.dyd_set_option(b"k7_variant", 22), "opt")
            ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), ro.data_ptr(), None, w2.data_ptr(), h2.data_ptr(), c2.data_ptr(), nr, nbx,
                                    to2.data_ptr(), fl2.data_ptr(), None, 0, C.byref(total), sp), "k7 measure")
            tx = torch.empty(total.value, dtype=torch.uint8, device=dev)
            res = {}
            for variant in (22, 30, 22, 30):
                ck(L.dyd_set_option(b"k7_variant", variant), "opt")
                med, mn = timeit(lambda: ck(L.dyd_yolo_lines_dev(out_box.data_ptr(), ro.data_ptr(), None, w2.data_ptr(), h2.data_ptr(), c2.data_ptr(),
                                                                  nr, nbx, to2.data_ptr(), fl2.data_ptr(), tx.data_ptr(), total.value, C.byref(total), sp), "k7"),
                                 iters=10, warm=2)
                res.setdefault(variant, []).append(med)
            print(json.dumps({"k7_boxes_per_row": round(nbx / nr, 3), "rows": nr, "lines": nbx, "pair_rows_ms": round(min(res[22]), 4),
                              "box_tiles_ms": round(min(res[30]), 4)}), flush=True)
            del ro, w2, h2, c2, to2, fl2, tx, counts
        ck(L.dyd_set_option(b"k7_variant", -1), "opt")

if __name__ == "__main__":
    main()
