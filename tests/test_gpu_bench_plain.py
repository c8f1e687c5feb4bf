"""bench.py's plain run and --dump-outputs: the line's contract without --full, EXACTLY --steps timed steps, identical dumps from two
runs with the same arguments, and the dumped sample of the fused launch's outputs equal to the CPU oracle on the same table
(bench.draw_table redrawn in this process with the seed the run used)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, STEPS = 20_000, 3
NAMES = ("high_sample", "high_sample_rows", "box_sample", "arg_sample", "box_sample_ids", "high_count_per_block", "arg_sum_per_block")


def _plain_run(dump_dir):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--rows", str(ROWS),
           "--ramp-ms", "10", "--dump-outputs", str(dump_dir)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(dump_dir, n + ".npy")) for n in NAMES}


def test_plain_run_and_its_dump(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    import torch
    from deal_yolo_daya_amd import synth
    from oracle import lib as olib

    line, got = _plain_run(tmp_path / "a")
    assert line["full"] is False and line["steps"] == STEPS and line["n_gpus"] == 1 and line["config"]["rows_per_gpu"] == ROWS
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(ROWS * 1e3 / line["ms_per_step"], rel=1e-9) and line["roofline"]["frac"] > 0
    for k in ("cpu_baseline", "host_inclusive", "full_pipeline", "dense", "sharded_exchange", "sharded_exchange_strong", "fused_strong"):
        assert line[k] is None, k                                                  # those legs run with --full only
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    _, again = _plain_run(tmp_path / "b")                                         # same arguments -> same inputs -> same files
    for n in NAMES:
        assert np.array_equal(got[n], again[n], equal_nan=True), n

    # the table the run drew (rank 0: seed synth.SEED), through the CPU oracle
    t = bench.draw_table(ROWS, None, synth.SEED, torch.device("cuda", 0))
    xy, pt_off, box_off = (t[k].cpu().numpy() for k in ("xy", "pt_off", "box_off"))
    box, arg, high = olib.bbox_iou_chain(xy, pt_off, box_off, bench.MIN_BOXES, bench.THR)
    N, B = len(box_off) - 1, len(pt_off) - 1
    assert line["config"]["boxes_per_gpu"] == B and line["config"]["high_rows_rank0"] == int(high.sum())
    rows = got["high_sample_rows"].astype(np.int64)
    boxes = got["box_sample_ids"].astype(np.int64)
    assert np.array_equal(rows, np.arange(N)) and len(boxes) == min(B, bench.DUMP_BOXES) and np.all(np.diff(boxes) > 0)
    assert np.array_equal(got["high_sample"], high[rows].astype(np.float32))
    assert np.array_equal(got["box_sample"].view(np.uint64), box[boxes].view(np.uint64))
    assert np.array_equal(got["arg_sample"], arg[boxes].astype(np.float64))

    def block_sums(v):
        return np.add.reduceat(v.astype(np.int64), np.arange(0, len(v), bench.DUMP_BLOCK)).astype(np.float64)

    assert np.array_equal(got["high_count_per_block"], block_sums(high))
    assert np.array_equal(got["arg_sum_per_block"], block_sums(arg.astype(np.int64).sum(1)))
