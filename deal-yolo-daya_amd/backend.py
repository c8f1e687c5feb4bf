"""Device-stage backend used by the step functions.

The product backend is ``_native`` (ctypes -> libdyd_gfx950.so -> HIP kernels on gfx950) and
nothing else: ``default_backend()`` raises when the library or the device is missing.  The
step functions take an optional ``backend=`` argument only so that host-side logic
(flatten / emit / sharding) can be exercised without a GPU by the CPU test-suite, which
injects its own checker there; no such object exists inside this package.
"""
from __future__ import annotations

# The later steps ask for their own entry on top of these (core/processor.py: _step_backend), e.g. compare_boxes (K18),
# rasterize_polygons (K21), polygon_rle (K23), compare_polygons (K22), eval_match_boxes and eval_accumulate (K24), eval_match_polygons (K25): a backend without it raises TypeError there, never a CPU fallback.
REQUIRED = ("bbox_minmax", "iou_any_ge", "bbox_iou_fused", "hash128", "dedup", "isin", "mt19937_permutation", "split_ids", "yolo_lines")


def default_backend():
    from . import _native

    _native.lib()          # raises NativeUnavailable: no CPU fallback
    return _native


def resolve(backend):
    if backend is None:
        return default_backend()
    missing = [n for n in REQUIRED if not hasattr(backend, n)]
    if missing:
        raise TypeError(f"backend lacks {missing}")
    return backend
