"""What tests/test_gpu_streams.py relies on, checked without a GPU: every entry of include/dyd.h that takes a stream is
registered there, every decoy is a valid table of the real table's shape whose reference outputs differ from the real table's
in every array, and the slice of the long sparse table keeps more than one part in every scan and its row of 700 polygons."""
import os
import re

import numpy as np
import pytest

import long_tables as LT
import test_gpu_streams as S
from stream_contract import differs, merge_off, moved, rev_off, rot_cls, valid_offsets

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dyd.h")
SCAN_TILE, POLY_BLOCK = 2048, 256          # K13_SCAN_TILE, polygons per workgroup (tests/test_long_tables_cpu.py)


def stream_entries():
    """the functions declared in include/dyd.h whose last parameter is `void *stream`"""
    with open(HEADER, encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    found = set()
    for m in re.finditer(r"\b(dyd_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if " ".join(m.group(2).split()).endswith("void *stream"):
            found.add(m.group(1))
    return found


def test_every_entry_that_takes_a_stream_is_registered():
    declared = stream_entries()
    assert len(declared) >= 27 and "dyd_compare_polygons_dev" in declared and "dyd_sync" in declared
    assert declared == set(S.ENTRIES), (sorted(declared - set(S.ENTRIES)), sorted(set(S.ENTRIES) - declared))
    for entry, test in S.ENTRIES.items():
        assert callable(getattr(S, test)), entry
    no_device_input = {"dyd_sync", "dyd_device_status", "dyd_mt19937_permutation_dev", "dyd_membench_dev"}
    assert {k.split(":")[0] for k in S.CASES} == declared - no_device_input      # membench copies bytes: any bytes are a valid decoy
    assert set(S.BLOCKING) <= declared


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_the_decoy_is_a_valid_table_and_changes_every_output(name):
    c = S.case(name)
    assert len(c.real) == len(c.decoy)
    changed = 0
    for k, (r, d) in enumerate(zip(c.real, c.decoy)):
        r, d = np.asarray(r), np.asarray(d)
        assert r.dtype == d.dtype and r.shape == d.shape, k
        changed += differs(r, d)
    assert changed
    for k in c.offsets:
        assert valid_offsets(c.real[k], c.decoy[k]), k
    for k, n_classes in c.classes.items():
        allowed = set(np.unique(c.real[k]).tolist()) | set(range(n_classes))
        assert set(np.unique(c.decoy[k]).tolist()) <= allowed, k
    want, other = c.want(), c.ref(c.decoy)
    assert len(want) == len(other)
    same = [k for k, (a, b) in enumerate(zip(want, other)) if not differs(a, b)]
    assert same == sorted(c.may_equal) and len(same) <= 1, same


def test_the_decoy_builders():
    off = np.asarray([0, 3, 3, 10, 11], np.int32)
    assert rev_off(off).tolist() == [0, 1, 8, 8, 11] and merge_off(off).tolist() == [0, 3, 3, 11, 11]
    assert merge_off(np.asarray([0, 2, 5, 9], np.int64)).tolist() == [0, 5, 5, 9]
    assert valid_offsets(off, rev_off(off)) and valid_offsets(off, merge_off(off)) and not valid_offsets(off, off[::-1])
    assert rot_cls(np.asarray([-1, 0, 2, 7], np.int32), 3).tolist() == [-1, 1, 0, 7]
    xy = np.asarray([0.0, 1.0, np.nan, 5.0])
    assert moved(xy).tolist()[2:] == [3.25, -0.75] and np.isnan(moved(xy)[0]) and moved(xy)[1] == 3.25


def test_the_slice_of_the_long_table_keeps_its_shape():
    xy, pt_off, row_off, W, H = LT.long_sparse(0, S.N_LONG)
    n, nb = len(W), len(pt_off) - 1
    count = np.diff(row_off)
    assert len(row_off) == n + 1 and row_off[-1] == nb and len(xy) == 2 * pt_off[-1]
    assert n > SCAN_TILE and nb > SCAN_TILE                      # more than one part in the scans over rows and over polygons
    big = int(np.argmax(count))
    assert count[big] == 700 > 2 * POLY_BLOCK and big == 2500
    blocks = np.arange(0, nb, POLY_BLOCK)                         # a block of polygons wholly inside that row
    assert ((blocks >= row_off[big]) & (blocks + POLY_BLOCK <= row_off[big + 1])).any()
    assert count[0] == 0 and count[-1] == 1 and set(LT.size_status(W, H).tolist()) == {0, 1, 2}
    with pytest.raises(IndexError):                               # the generator puts the row of 700 polygons at index 2500
        LT.long_sparse(0, 1500)
    want = S.case("dyd_yolo_seg_lines_dev").want()
    assert len(want[3]) > 32 * 1024 and len(set(want[2].tolist())) >= 3            # more than one print window of K13
    k20 = S.case("dyd_yolo_tile_lines_dev").want()
    assert len(k20[2]) > SCAN_TILE                               # the scan over tiles has more than one part, too
    assert len(S.case("dyd_rasterize_polygons_dev").want()[-1]) > 10000
