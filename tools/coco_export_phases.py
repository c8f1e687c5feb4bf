#!/usr/bin/env python3
"""Host-inclusive split of the COCO export (export_coco_frame) on one MI355X: native named-polygon scan / K16 (host arrays in
and out, copies included) / the rest (sizes, splicing, category ids, image entries, writing the file).  Prints one JSON line.

    python tools/coco_export_phases.py [--rows 1000000] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    from deal_yolo_daya_amd import _native, synth
    from deal_yolo_daya_amd import native_json as nj
    from deal_yolo_daya_amd.core import processor as P

    df = synth.to_frame(synth.generate(args.rows, seed=7))           # synthetic polygons (3..12 points), 20 class names
    rng = np.random.default_rng(args.rows)
    df["width"] = rng.choice([640, 1280, 1920], args.rows)
    df["height"] = rng.choice([480, 720, 1080], args.rows)
    acc = {"scan": 0.0, "k16": 0.0}

    def timed(key, fn):
        def wrap(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                acc[key] += time.perf_counter() - t0
        return wrap

    nj.scan_named_polygons = timed("scan", nj.scan_named_polygons)
    _native.coco_annotations = timed("k16", _native.coco_annotations)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "instances.json")
        P.export_coco_frame(df, out, json_col=synth.ANN_COL)         # warm-up: code objects, page faults
        res = []
        for _ in range(args.reps):
            for k in acc:
                acc[k] = 0.0
            t0 = time.perf_counter()
            stats = P.export_coco_frame(df, out, json_col=synth.ANN_COL)
            total = time.perf_counter() - t0
            res.append({"total": total, **acc, "rest": total - sum(acc.values())})
        size = os.path.getsize(out)
    med = {k: round(float(np.median([r[k] for r in res])) * 1e3, 2) for k in res[0]}
    print(json.dumps({"tool": "coco_export_phases", "rows": args.rows, "polygons": stats["polygons"],
                      "annotations": stats["annotations"], "images": stats["images"], "file_bytes": size,
                      "ms_median": med, "device": _native.device_name()}), flush=True)


if __name__ == "__main__":
    main()
