#!/usr/bin/env python3
"""Host-inclusive split of the box repair step (repair_boxes_frame) on one MI355X: native scan / K11 (host arrays in and out,
copies included) / native emit / the rest (sizes, splicing, the changes and per_class frames).  Prints one JSON line.

    python tools/repair_phases.py [--rows 1000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    from test_gpu_box_audit import _synthetic_frame

    from deal_yolo_daya_amd import _native
    from deal_yolo_daya_amd import native_json as nj
    from deal_yolo_daya_amd.core import processor as P

    df = _synthetic_frame(args.rows, np.random.default_rng(args.rows))
    acc = {"scan": 0.0, "k11": 0.0, "emit": 0.0}

    def timed(key, fn):
        def wrap(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                acc[key] += time.perf_counter() - t0
        return wrap

    nj.scan_named_boxes = timed("scan", nj.scan_named_boxes)
    _native.repair_boxes = timed("k11", _native.repair_boxes)
    nj.NamedBoxScan.emit_repaired = timed("emit", nj.NamedBoxScan.emit_repaired)
    P.repair_boxes_frame(df)                                        # warm-up: code objects, page faults
    res = []
    for _ in range(args.reps):
        for k in acc:
            acc[k] = 0.0
        stats = {}
        t0 = time.perf_counter()
        P.repair_boxes_frame(df, stats=stats)
        total = time.perf_counter() - t0
        res.append({"total": total, **acc, "rest": total - sum(acc.values())})
    med = {k: round(float(np.median([r[k] for r in res])) * 1e3, 2) for k in res[0]}
    print(json.dumps({"tool": "repair_phases", "rows": args.rows, "boxes": stats["boxes"], "clipped": stats["boxes_clipped"],
                      "removed": stats["boxes_removed"], "rows_changed": stats["rows_changed"], "ms_median": med,
                      "device": _native.device_name()}), flush=True)


if __name__ == "__main__":
    main()
