"""ctypes binding of libdyd_gfx950.so (C ABI: include/dyd.h).

This is the thin layer between the Python host code and the HIP kernels.  It has NO CPU
fallback: a missing library or a missing gfx950 device raises ``NativeUnavailable`` the
first time a device stage is requested.

Numpy-facing helpers (``bbox_minmax`` ...) use the host-pointer entry points (the library
stages H2D/D2H); ``lib()`` exposes the raw ``_dev`` entry points for callers that keep data
resident in HBM (bench.py, the distributed path).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DYD_LIB_PATH") or os.path.join(_PKG, "libdyd_gfx950.so")   # env: A/B builds of the library

KEEP_FIRST, KEEP_LAST, KEEP_NONE = 0, 1, 2
_KEEP = {"first": KEEP_FIRST, "last": KEEP_LAST, False: KEEP_NONE}

_lock = threading.Lock()
_lib = None
_ready = False


class NativeUnavailable(RuntimeError):
    """libdyd_gfx950.so could not be loaded or no gfx950 device is usable."""


class NativeError(RuntimeError):
    """An entry point of libdyd_gfx950.so returned an error code."""


_c = C
_dp, _i32p, _i64p, _u8p, _u64p = (C.POINTER(t) for t in (C.c_double, C.c_int32, C.c_int64, C.c_uint8, C.c_uint64))

# name -> (restype, argtypes); mirrors include/dyd.h line by line
SIGNATURES = {
    "dyd_init": (C.c_int, [C.c_int]),
    "dyd_shutdown": (None, []),
    "dyd_last_error": (C.c_char_p, []),
    "dyd_device_count": (C.c_int, []),
    "dyd_version": (C.c_char_p, []),
    "dyd_device_name": (C.c_char_p, []),
    "dyd_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "dyd_free": (C.c_int, [C.c_void_p]),
    "dyd_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "dyd_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "dyd_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "dyd_sync": (C.c_int, [C.c_void_p]),
    "dyd_device_status": (C.c_int, [C.c_void_p]),
    "dyd_last_kernel_ms": (C.c_double, []),
    "dyd_bbox_minmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dyd_bbox_minmax_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_iou_any_ge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "dyd_suppress_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "dyd_suppress_boxes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "dyd_json_scan_box_objects": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_json_scan_box_objects_v": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_scan_box_object": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_box_name": (C.c_void_p, [C.c_void_p]),
    "dyd_json_emit_dropping": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p)]),
    "dyd_box_audit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_box_audit_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "dyd_repair_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_repair_boxes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "dyd_compare_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                    C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "dyd_compare_boxes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_eval_match_boxes": (C.c_int, [C.c_void_p] * 7 + [C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7),
    "dyd_eval_accumulate": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
                            + [C.c_void_p] * 8),
    "dyd_eval_match_polygons": (C.c_int, [C.c_void_p] * 11 + [C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                                              C.c_int64] + [C.c_void_p] * 13),
    "dyd_json_emit_repaired": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p)]),
    "dyd_json_emit_simplified": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p)]),
    "dyd_json_scan_named_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_json_scan_named_boxes_v": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_scan_names": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_iou_any_ge_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "dyd_bbox_iou_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "dyd_host_pool_trim": (None, []),
    "dyd_stage_acquire": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "dyd_stage_release": (None, [C.c_void_p]),
    "dyd_bbox_iou_fused_staged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_bbox_iou_fused_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                         C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_hash128": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "dyd_hash128_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dyd_dedup": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "dyd_dedup_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "dyd_isin": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "dyd_dedup_partner": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "dyd_isin_partner": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "dyd_host_cells_differ": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "dyd_isin_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "dyd_dedup_global_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "dyd_mt19937_permutation": (C.c_int, [C.c_uint32, C.c_int64, C.c_void_p]),
    "dyd_split_ids": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p]),
    "dyd_split_ids_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_split_ids_sharded_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_mt19937_permutation_dev": (C.c_int, [C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_split_ids_seeded": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p]),
    "dyd_split_ids_seeded_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_yolo_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "dyd_yolo_lines_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "dyd_yolo_seg_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "dyd_yolo_seg_lines_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.POINTER(C.c_int64), C.c_void_p]),
    "dyd_yolo_obb_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_int64)]),
    "dyd_yolo_obb_lines_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "dyd_audit_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_audit_polygons_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_simplify_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_simplify_polygons_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_yolo_tile_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                      C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "dyd_yolo_tile_lines_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int32,
                                          C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int64,
                                          C.POINTER(C.c_int64), C.c_void_p]),
    "dyd_rasterize_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64)]),
    "dyd_rasterize_polygons_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "dyd_compare_polygons": (C.c_int, [C.c_void_p] * 10 + [C.c_int64, C.c_int32, C.c_double, C.c_int, C.c_int64, C.c_int64]
                             + [C.c_void_p] * 15),
    "dyd_compare_polygons_dev": (C.c_int, [C.c_void_p] * 10 + [C.c_int64] * 5 + [C.c_int32, C.c_double, C.c_int, C.c_int64, C.c_int64]
                                 + [C.c_void_p] * 16 + [C.c_int64, C.c_void_p]),
    "dyd_polygon_rle": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int64] + [C.c_void_p] * 6
                        + [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "dyd_polygon_rle_dev": (C.c_int, [C.c_void_p] * 6 + [C.c_int64] * 4 + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                                                               C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dyd_coco_annotations": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_int64, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int64)]),
    "dyd_coco_annotations_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "dyd_json_scan_named_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_json_scan_named_polygons_v": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_json_scan_labelled_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                                  C.POINTER(C.c_void_p)]),
    "dyd_json_scan_labelled_polygons_v": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.POINTER(C.c_void_p)]),
    "dyd_json_scan_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_json_emit_polygons": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_json_scan_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_scan_n_boxes": (C.c_int64, [C.c_void_p]),
    "dyd_scan_n_points": (C.c_int64, [C.c_void_p]),
    "dyd_scan_xy": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_pt_off": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_cell_box_off": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_status": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_wh_kind": (C.c_void_p, [C.c_void_p, C.c_int]),
    "dyd_scan_wh_value": (C.c_void_p, [C.c_void_p, C.c_int]),
    "dyd_scan_iou_host": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_fast_cells": (C.c_int64, [C.c_void_p]),
    "dyd_json_scan_polygons_v": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_json_replace_iou": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double,
                                       C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_scan_high": (C.c_void_p, [C.c_void_p]),
    "dyd_scan_parts": (C.c_int32, [C.c_void_p]),
    "dyd_scan_part": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                C.POINTER(C.c_void_p)]),
    "dyd_scan_text": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_scan_totals": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "dyd_scan_free": (None, [C.c_void_p]),
    "dyd_synth_json": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                 C.POINTER(C.c_void_p), C.c_void_p]),
    "dyd_json_scan_labelled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_void_p)]),
    "dyd_scan_sel": (C.c_void_p, [C.c_void_p]),
    "dyd_json_split_expand": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
                                        C.POINTER(C.c_void_p)]),
    "dyd_split_status": (C.c_void_p, [C.c_void_p]),
    "dyd_split_n_expanded": (C.c_void_p, [C.c_void_p]),
    "dyd_split_rows": (C.c_int64, [C.c_void_p]),
    "dyd_split_row_cell": (C.c_void_p, [C.c_void_p]),
    "dyd_split_row_label": (C.c_void_p, [C.c_void_p]),
    "dyd_split_events": (C.c_int64, [C.c_void_p]),
    "dyd_split_event_cell": (C.c_void_p, [C.c_void_p]),
    "dyd_split_event_kind": (C.c_void_p, [C.c_void_p]),
    "dyd_split_strings": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_split_free": (None, [C.c_void_p]),
    "dyd_json_split_expand_v": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
                                          C.POINTER(C.c_void_p)]),
    "dyd_split_rec_views": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_split_event_code": (C.c_void_p, [C.c_void_p]),
    "dyd_split_undefined": (C.c_int64, [C.c_void_p]),
    "dyd_split_label_first": (C.c_void_p, [C.c_void_p]),
    "dyd_split_label_count": (C.c_void_p, [C.c_void_p]),
    "dyd_split_fast_cells": (C.c_int64, [C.c_void_p]),
    "dyd_split_all_ascii": (C.c_int, [C.c_void_p]),
    "dyd_split_reason_code": (C.c_void_p, [C.c_void_p]),
    "dyd_split_reason_distinct": (C.c_int64, [C.c_void_p]),
    "dyd_split_reason_first": (C.c_void_p, [C.c_void_p]),
    "dyd_split_seconds": (None, [C.c_void_p, C.c_void_p]),
    "dyd_json_relabel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_int, C.POINTER(C.c_void_p)]),
    "dyd_relabel_status": (C.c_void_p, [C.c_void_p]),
    "dyd_relabel_has_diff": (C.c_void_p, [C.c_void_p]),
    "dyd_relabel_counts": (C.c_void_p, [C.c_void_p]),
    "dyd_relabel_tokens": (C.c_int64, [C.c_void_p]),
    "dyd_relabel_token_cell": (C.c_void_p, [C.c_void_p]),
    "dyd_relabel_strings": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_relabel_free": (None, [C.c_void_p]),
    "dyd_csv_index": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "dyd_csv_rows": (C.c_int64, [C.c_void_p]),
    "dyd_csv_cols": (C.c_int32, [C.c_void_p]),
    "dyd_csv_header": (C.c_int64, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "dyd_csv_extract": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "dyd_csv_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "dyd_csv_col_bytes": (C.c_int64, [C.c_void_p, C.c_int32]),
    "dyd_csv_row_end": (C.c_int64, [C.c_void_p, C.c_int64]),
    "dyd_csv_has_cr": (C.c_int, [C.c_void_p]),
    "dyd_csv_free": (None, [C.c_void_p]),
    "dyd_csv_write": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "dyd_host_free": (None, [C.c_void_p]),
    "dyd_set_option": (C.c_int, [C.c_char_p, C.c_int64]),
    "dyd_membench_dev": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
}


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libdyd_gfx950.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j8"]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if out.returncode != 0:
        raise RuntimeError("building libdyd_gfx950.so failed:\n" + out.stdout)
    if verbose:
        print(out.stdout)
    return LIB_PATH


def _one_hip_runtime_per_process():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  If this library pulled in
    /opt/rocm's copy first and torch initialised its bundled copy afterwards, the process would hold
    two HIP runtimes and the second one finds no GPU.  Importing torch first (when it is installed)
    makes libdyd_gfx950.so bind to the runtime torch uses, so device pointers and streams are shared."""
    import sys

    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:  # torch is optional plumbing; without it /opt/rocm's runtime is used
            pass


def load_library():
    """dlopen the library and declare every prototype.  Does not touch the GPU."""
    global _lib
    with _lock:
        if _lib is None:
            _one_hip_runtime_per_process()
            if not os.path.exists(LIB_PATH):
                raise NativeUnavailable(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or `make -C deal-yolo-daya_amd/csrc`).  There is no CPU fallback.")
            try:
                lib_ = C.CDLL(LIB_PATH)
            except OSError as e:
                raise NativeUnavailable(f"cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib_, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib_
    return _lib


def lib():
    """The loaded library with an initialised device context (raises if there is no gfx950)."""
    global _ready
    l = load_library()
    if not _ready:
        with _lock:
            if not _ready:
                dev = int(os.environ.get("DYD_DEVICE", "-1"))
                rc = l.dyd_init(dev)
                if rc != 0:
                    raise NativeUnavailable(
                        "dyd_init failed: " + l.dyd_last_error().decode("utf-8", "replace")
                        + " — the HIP device stage is required; there is no CPU fallback.")
                _ready = True
    return l


def available() -> bool:
    try:
        lib()
        return True
    except NativeUnavailable:
        return False


def check(rc: int, what: str):
    if rc != 0:
        raise NativeError(f"{what} failed ({rc}): " + load_library().dyd_last_error().decode("utf-8", "replace"))


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def device_name() -> str:
    return lib().dyd_device_name().decode()


def last_kernel_ms() -> float:
    return float(load_library().dyd_last_kernel_ms())


# ------------------------------------------------------------------ numpy-facing helpers
def bbox_minmax(xy: np.ndarray, pt_off: np.ndarray):
    """K1 over host arrays: returns (box4 [B,4] f64, arg4 [B,4] i32)."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int32)
    nb = len(pt_off) - 1
    if nb < 0 or (nb >= 0 and (pt_off[0] != 0 or 2 * int(pt_off[-1]) != xy.size)):
        raise ValueError("pt_off must start at 0 and end at the number of points")
    box = np.empty((nb, 4), np.float64)
    arg = np.empty((nb, 4), np.int32)
    check(lib().dyd_bbox_minmax(_ptr(xy), _ptr(pt_off), nb, _ptr(box), _ptr(arg)), "dyd_bbox_minmax")
    return box, arg


def iou_any_ge(box4: np.ndarray, row_off: np.ndarray, min_boxes: int, thr: float, want_max: bool = False):
    """K2 over host arrays: HIGH flag per row (and the max pair IoU when ``want_max``)."""
    box4 = np.ascontiguousarray(box4, dtype=np.float64).reshape(-1)
    row_off = np.ascontiguousarray(row_off, dtype=np.int32)
    n = len(row_off) - 1
    if n < 0 or row_off[0] != 0 or 4 * int(row_off[-1]) != box4.size:
        raise ValueError("row_off must start at 0 and end at the number of boxes")
    high = np.empty(n, np.uint8)
    mx = np.empty(n, np.float64) if want_max else None
    check(lib().dyd_iou_any_ge(_ptr(box4), _ptr(row_off), n, int(min_boxes), float(thr), _ptr(high),
                               _ptr(mx) if want_max else None), "dyd_iou_any_ge")
    return (high, mx) if want_max else high


def suppress_boxes(box4: np.ndarray, row_off: np.ndarray, thr: float, name=None):
    """K9 over host arrays: (keep [B] u8, partner [B] i32).  A box is dropped when an earlier kept box of its row (of equal
    name id when ``name`` is given) reaches IoU >= thr with it; partner = in-row index of the first such box, else -1."""
    box4 = np.ascontiguousarray(box4, dtype=np.float64).reshape(-1)
    row_off = np.ascontiguousarray(row_off, dtype=np.int32)
    n = len(row_off) - 1
    if n < 0 or row_off[0] != 0 or 4 * int(row_off[-1]) != box4.size:
        raise ValueError("row_off must start at 0 and end at the number of boxes")
    nb = int(row_off[-1])
    if name is not None:
        name = np.ascontiguousarray(name, dtype=np.int32)
        if name.size != nb:
            raise ValueError("name must hold one id per box")
    keep = np.ones(nb, np.uint8)
    partner = np.full(nb, -1, np.int32)
    check(lib().dyd_suppress_boxes(_ptr(box4), _ptr(row_off), n, _ptr(name) if name is not None else None, float(thr),
                                   _ptr(keep), _ptr(partner)), "dyd_suppress_boxes")
    return keep, partner


AUDIT_BPI = 257      # boxes_per_image bins: 0..255 boxes, then >= 256


def _box_table(box4, row_off, cls, width, height, size_status) -> tuple:
    """the box table of K10 / K11 as contiguous arrays of the kernels' dtypes, its sizes checked -> (box4, row_off, cls, width,
    height, size_status, n_rows, n_boxes)"""
    box4 = np.ascontiguousarray(box4, dtype=np.float64).reshape(-1)
    row_off = np.ascontiguousarray(row_off, dtype=np.int32)
    n = len(row_off) - 1
    if n < 0 or row_off[0] != 0 or 4 * int(row_off[-1]) != box4.size:
        raise ValueError("row_off must start at 0 and end at the number of boxes")
    nb = int(row_off[-1])
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    width = np.ascontiguousarray(width, dtype=np.float64)
    height = np.ascontiguousarray(height, dtype=np.float64)
    size_status = np.ascontiguousarray(size_status, dtype=np.uint8)
    if cls.size != nb or width.size != n or height.size != n or size_status.size != n:
        raise ValueError("cls must hold one id per box; width, height and size_status one value per row")
    return box4, row_off, cls, width, height, size_status, n, nb


def _poly_table(xy, pt_off, row_off, width, height, row_col: tuple, poly_col: tuple = None) -> tuple:
    """the polygon table of K13 / K14 / K16 as contiguous arrays of the kernels' dtypes, its sizes checked -> (xy, pt_off, row_off,
    width, height, the step's per-row column, its per-polygon column or None, n_rows, n_polys).  row_col / poly_col = (name, values,
    dtype) of the step's own columns."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int32)
    row_off = np.ascontiguousarray(row_off, dtype=np.int32)
    width = np.ascontiguousarray(width, dtype=np.float64)
    height = np.ascontiguousarray(height, dtype=np.float64)
    per_row = np.ascontiguousarray(row_col[1], dtype=row_col[2])
    per_poly = np.ascontiguousarray(poly_col[1], dtype=poly_col[2]) if poly_col else None
    n = len(row_off) - 1
    if n < 0 or len(width) != n or len(height) != n or len(per_row) != n:
        raise ValueError(f"row_off / width / height / {row_col[0]} sizes disagree")
    nb = int(row_off[-1]) if n else 0
    if (poly_col and len(per_poly) != nb) or len(pt_off) != nb + 1 or (nb and 2 * int(pt_off[-1]) != len(xy)):
        raise ValueError(f"{poly_col[0]} and pt_off must hold one entry per polygon (pt_off one more), ending at the number of points"
                         if poly_col else "pt_off must hold one entry per polygon plus one and end at the number of points")
    return xy, pt_off, row_off, width, height, per_row, per_poly, n, nb


def _take_text(text, total) -> bytes:
    """the malloc'ed text an entry handed back, as bytes; the buffer is released"""
    try:
        return C.string_at(text.value, total.value) if total.value else b""
    finally:
        load_library().dyd_host_free(text)


def box_audit(box4: np.ndarray, row_off: np.ndarray, cls: np.ndarray, width: np.ndarray, height: np.ndarray,
              size_status: np.ndarray, n_classes: int, nbins: int):
    """K10 over host arrays -> (flag [B] u8, row_counts [N,6] i32, class_counts [C,9] i64, hist_wh [C,nb,nb] i64,
    hist_xy [C,nb,nb] i64, boxes_per_image [257] i64).  See include/dyd.h for the columns and the flag bits."""
    box4, row_off, cls, width, height, size_status, n, nb = _box_table(box4, row_off, cls, width, height, size_status)
    nbins, n_classes = int(nbins), int(n_classes)
    if not 1 <= nbins <= 64:
        raise ValueError(f"nbins must lie in 1..64, got {nbins}")
    flag = np.zeros(nb, np.uint8)
    rows = np.zeros((n, 6), np.int32)
    cc = np.zeros((n_classes, 9), np.int64)
    wh = np.zeros((n_classes, nbins, nbins), np.int64)
    xy = np.zeros((n_classes, nbins, nbins), np.int64)
    bpi = np.zeros(AUDIT_BPI, np.int64)
    check(lib().dyd_box_audit(_ptr(box4), _ptr(row_off), n, _ptr(cls), _ptr(width), _ptr(height), _ptr(size_status), n_classes,
                              nbins, _ptr(flag), _ptr(rows), _ptr(cc), _ptr(wh), _ptr(xy), _ptr(bpi)), "dyd_box_audit")
    return flag, rows, cc, wh, xy, bpi


POLY_CLASS_COLS = 14   # K14 per-class counters: polygons, images, 6 categories, 3 defects, 3 area buckets
POLY_HIST_BINS = 11    # K14 vertex-count bins: <= 2, 3, 4, 8, 16, 32, 64, 128, 256, 1024, the rest


def audit_polygons(xy, pt_off, row_off, cls, width, height, size_status, n_classes: int, min_area: float = 1.0):
    """K14 over host arrays -> (category u8 [B], defects u8 [B], area f64 [B], class_counts i64 [C, 14], hist_vertices
    i64 [C, 11]).  Codes, bits and columns: include/dyd.h."""
    xy, pt_off, row_off, width, height, size_status, cls, n, nb = _poly_table(
        xy, pt_off, row_off, width, height, ("size_status", size_status, np.uint8), ("cls", cls, np.int32))
    n_classes, min_area = int(n_classes), float(min_area)
    cat, dfc, area = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), np.zeros(nb, np.float64)
    cc, hist = np.zeros((n_classes, POLY_CLASS_COLS), np.int64), np.zeros((n_classes, POLY_HIST_BINS), np.int64)
    check(lib().dyd_audit_polygons(_ptr(xy) if xy.size else None, _ptr(pt_off), _ptr(row_off), _ptr(cls), _ptr(width),
                                   _ptr(height), _ptr(size_status), n, n_classes, min_area, _ptr(cat), _ptr(dfc), _ptr(area),
                                   _ptr(cc), _ptr(hist)), "dyd_audit_polygons")
    return cat, dfc, area, cc, hist


def simplify_polygons(xy, pt_off, tolerance: float = 1.0):
    """K19 over host arrays -> (keep u8 [P], action u8 [B], kept i32 [B], dev2 f64 [B]).  Rule and codes: include/dyd.h."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int32)
    nb = len(pt_off) - 1
    if nb < 0 or (nb and 2 * int(pt_off[-1]) != len(xy)):
        raise ValueError("pt_off must hold one entry per polygon plus one and end at the number of points")
    keep, action = np.zeros(len(xy) // 2, np.uint8), np.zeros(nb, np.uint8)
    kept, dev2 = np.zeros(nb, np.int32), np.zeros(nb, np.float64)
    check(lib().dyd_simplify_polygons(_ptr(xy) if xy.size else None, _ptr(pt_off), nb, float(tolerance),
                                      _ptr(keep) if keep.size else None, _ptr(action), _ptr(kept), _ptr(dev2)),
          "dyd_simplify_polygons")
    return keep, action, kept, dev2


COCO_SEGMENTATION = 1   # K16 flags bit 0: print the polygon into "segmentation" (clear: the detect flavour, an empty list)


def coco_annotations(xy, pt_off, row_off, cat_id, width, height, size_status, image_id_base: int = 1, ann_id_base: int = 1,
                     flags: int = COCO_SEGMENTATION):
    """K16 over host arrays -> (action u8 [B], area f64 [B] (NaN unless printed), row_kept i32 [n], text bytes): one COCO
    annotation object per polygon with cat_id >= 1 that K13 would write, joined with ",".  Definition: include/dyd.h."""
    xy, pt_off, row_off, width, height, size_status, cat_id, n, nb = _poly_table(
        xy, pt_off, row_off, width, height, ("size_status", size_status, np.uint8), ("cat_id", cat_id, np.int32))
    action, area, kept = np.zeros(nb, np.uint8), np.zeros(nb, np.float64), np.zeros(n, np.int32)
    text, total = C.c_void_p(), C.c_int64()
    check(lib().dyd_coco_annotations(_ptr(xy) if xy.size else None, _ptr(pt_off), _ptr(row_off), _ptr(cat_id) if nb else None,
                                     _ptr(width), _ptr(height), _ptr(size_status), n, int(image_id_base), int(ann_id_base),
                                     int(flags), _ptr(action) if nb else None, _ptr(area) if nb else None, _ptr(kept), C.byref(text),
                                     C.byref(total)), "dyd_coco_annotations")
    return action, area, kept, _take_text(text, total)


def yolo_tile_lines(xy, pt_off, row_off, cls, width, height, tile_w: int, tile_h: int, step_x: int, step_y: int,
                    min_visibility: float = 0.1, mode: int = 0, max_tiles_per_row: int = 4096):
    """K20 over host arrays -> (row_status u8 [n], tile_off i64 [n+1], tile_line_count i32 [T], text_off i64 [T+1], action u8 [B],
    tiles_written / tiles_cut / tiles_dropped i32 [B], text bytes).  mode 0 segment, 1 detect.  Rule and codes: include/dyd.h."""
    from .flatten import tile_grid

    xy, pt_off, row_off, width, height, _, cls, n, nb = _poly_table(xy, pt_off, row_off, width, height,   # no row column of its own
                                                                    ("width", width, np.float64), ("cls", cls, np.int32))
    args = tuple(int(v) for v in (tile_w, tile_h, step_x, step_y))
    T = 0
    if n and all(1 <= v <= 1 << 20 for v in args) and 1 <= int(max_tiles_per_row) <= 1 << 20:   # else the entry rejects the call
        _, nx, ny = tile_grid(width, height, *args, int(max_tiles_per_row))
        T = int((nx * ny).sum())
    status, tile_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    lines, text_off = np.zeros(T, np.int32), np.zeros(T + 1, np.int64)
    action = np.zeros(nb, np.uint8)
    written, cut, dropped = np.zeros(nb, np.int32), np.zeros(nb, np.int32), np.zeros(nb, np.int32)
    text, total, n_tiles = C.c_void_p(), C.c_int64(), C.c_int64()
    opt = lambda a: _ptr(a) if a.size else None          # noqa: E731
    check(lib().dyd_yolo_tile_lines(opt(xy), _ptr(pt_off), _ptr(row_off), opt(cls), _ptr(width), _ptr(height), n, *args,
                                    float(min_visibility), int(mode), int(max_tiles_per_row), T, _ptr(status), _ptr(tile_off),
                                    opt(lines), _ptr(text_off), opt(action), opt(written), opt(cut), opt(dropped),
                                    C.byref(n_tiles), C.byref(text), C.byref(total)), "dyd_yolo_tile_lines")
    return status, tile_off, lines, text_off, action, written, cut, dropped, _take_text(text, total)


def rasterize_polygons(xy, pt_off, row_off, val, width, height, background: int = 0, max_pixels_per_row: int = 1 << 26):
    """K21 over host arrays -> (row_status u8 [n], pix_off i64 [n+1], action u8 [B], covered i64 [B], owned i64 [B], pixels u8
    [pix_off[n]]): the mask of row i is pixels[pix_off[i]:pix_off[i+1]] as H lines of W bytes.  Rule and codes: include/dyd.h."""
    xy, pt_off, row_off, width, height, _, val, n, nb = _poly_table(xy, pt_off, row_off, width, height,   # no row column of its own
                                                                    ("width", width, np.float64), ("val", val, np.int32))
    status, pix_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    action, covered, owned = np.zeros(nb, np.uint8), np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    pixels, total = C.c_void_p(), C.c_int64()
    opt = lambda a: _ptr(a) if a.size else None          # noqa: E731
    check(lib().dyd_rasterize_polygons(opt(xy), _ptr(pt_off), _ptr(row_off), opt(val), _ptr(width), _ptr(height), n, int(background),
                                       int(max_pixels_per_row), _ptr(status), _ptr(pix_off), opt(action), opt(covered), opt(owned),
                                       C.byref(pixels), C.byref(total)), "dyd_rasterize_polygons")
    return status, pix_off, action, covered, owned, np.frombuffer(_take_text(pixels, total), np.uint8)


def polygon_rle(xy, pt_off, row_off, sel, width, height, max_pixels_per_row: int = 1 << 26):
    """K23 over host arrays -> (row_status u8 [n], action u8 [B], area i64 [B], bbox i32 [B, 4], run_off i64 [B+1], runs u32
    [run_off[B]], text_off i64 [B+1], text bytes): the column-major run lengths of polygon p's own mask are
    runs[run_off[p]:run_off[p+1]], their COCO "counts" string text[text_off[p]:text_off[p+1]].  Rule and codes: include/dyd.h."""
    xy, pt_off, row_off, width, height, _, sel, n, nb = _poly_table(xy, pt_off, row_off, width, height,   # no row column of its own
                                                                    ("width", width, np.float64), ("sel", sel, np.int32))
    status, action = np.zeros(n, np.uint8), np.zeros(nb, np.uint8)
    area, bbox = np.zeros(nb, np.int64), np.zeros((nb, 4), np.int32)
    run_off, text_off = np.zeros(nb + 1, np.int64), np.zeros(nb + 1, np.int64)
    runs, n_runs, text, total = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
    opt = lambda a: _ptr(a) if a.size else None          # noqa: E731
    check(lib().dyd_polygon_rle(opt(xy), _ptr(pt_off), _ptr(row_off), opt(sel), _ptr(width), _ptr(height), n, int(max_pixels_per_row),
                                _ptr(status), opt(action), opt(area), opt(bbox), _ptr(run_off), _ptr(text_off), C.byref(runs),
                                C.byref(n_runs), C.byref(text), C.byref(total)), "dyd_polygon_rle")
    n_bytes = C.c_int64(4 * n_runs.value)
    return (status, action, area, bbox, run_off, np.frombuffer(_take_text(runs, n_bytes), np.uint32), text_off,
            _take_text(text, total))


def compare_polygons(a_xy, a_pt_off, a_row_off, a_cls, b_xy, b_pt_off, b_row_off, b_cls, width, height, n_classes: int,
                     thr: float = 0.5, by_label: bool = False, max_pixels_per_row: int = 1 << 26, max_pairs_per_row: int = 1 << 20):
    """K22 over host arrays: two polygon tables of the same rows -> (row_status u8 [n], pair_off i64 [n+1], a_action u8 [A],
    b_action u8 [B], a_pixels i64 [A], b_pixels i64 [B], a_match i32 [A], b_match i32 [B], b_iou f64 [B], a_best f64 [A], b_best
    f64 [B], row_counts i32 [n, 4], confusion u64 [C+1, C+1], pixel_confusion u64 [C+1, C+1], row_pixels i64 [n, 2]).  Rule and
    codes: include/dyd.h."""
    a_xy, a_pt_off, a_row_off, width, height, _, a_cls, n, na = _poly_table(a_xy, a_pt_off, a_row_off, width, height,
                                                                            ("width", width, np.float64), ("a_cls", a_cls, np.int32))
    b_xy, b_pt_off, b_row_off, _, _, _, b_cls, _, nb = _poly_table(b_xy, b_pt_off, b_row_off, width, height,
                                                                   ("width", width, np.float64), ("b_cls", b_cls, np.int32))
    C_ = int(n_classes)
    cells = max(C_, 0) + 1
    status, pair_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    a_act, b_act = np.zeros(na, np.uint8), np.zeros(nb, np.uint8)
    a_pix, b_pix = np.zeros(na, np.int64), np.zeros(nb, np.int64)
    a_match, b_match = np.full(na, -1, np.int32), np.full(nb, -1, np.int32)
    b_iou, a_best, b_best = np.zeros(nb, np.float64), np.zeros(na, np.float64), np.zeros(nb, np.float64)
    rows, row_pixels = np.zeros((n, 4), np.int32), np.zeros((n, 2), np.int64)
    conf, pconf = np.zeros((cells, cells), np.uint64), np.zeros((cells, cells), np.uint64)
    opt = lambda a: _ptr(a) if a.size else None          # noqa: E731
    check(lib().dyd_compare_polygons(opt(a_xy), _ptr(a_pt_off), _ptr(a_row_off), opt(a_cls), opt(b_xy), _ptr(b_pt_off),
                                     _ptr(b_row_off), opt(b_cls), _ptr(width), _ptr(height), n, C_, float(thr), int(bool(by_label)),
                                     int(max_pixels_per_row), int(max_pairs_per_row), _ptr(status), _ptr(pair_off), opt(a_act),
                                     opt(b_act), opt(a_pix), opt(b_pix), opt(a_match), opt(b_match), opt(b_iou), opt(a_best),
                                     opt(b_best), _ptr(rows), _ptr(conf), _ptr(pconf), _ptr(row_pixels)), "dyd_compare_polygons")
    return status, pair_off, a_act, b_act, a_pix, b_pix, a_match, b_match, b_iou, a_best, b_best, rows, conf, pconf, row_pixels


REPAIR_ACTIONS = 8   # action codes of K11: keep, clip, no_size, bad_coords, degenerate, outside, low_visibility, small


def repair_boxes(box4: np.ndarray, row_off: np.ndarray, cls: np.ndarray, width: np.ndarray, height: np.ndarray,
                 size_status: np.ndarray, n_classes: int, min_visibility: float = 0.0, min_size: float = 0.0):
    """K11 over host arrays -> (action [B] u8, box4 [B,4] f64, row_counts [N,8] i32, class_counts [C,8] i64).  See
    include/dyd.h for the action codes and the rules."""
    box4, row_off, cls, width, height, size_status, n, nb = _box_table(box4, row_off, cls, width, height, size_status)
    min_visibility, min_size, n_classes = float(min_visibility), float(min_size), int(n_classes)
    if not 0.0 <= min_visibility <= 1.0:
        raise ValueError(f"min_visibility must lie in [0, 1], got {min_visibility}")
    if not (np.isfinite(min_size) and min_size >= 0.0):
        raise ValueError(f"min_size must be finite and >= 0, got {min_size}")
    action = np.zeros(nb, np.uint8)
    out_box = np.zeros((nb, 4), np.float64)
    rows = np.zeros((n, REPAIR_ACTIONS), np.int32)
    cc = np.zeros((n_classes, REPAIR_ACTIONS), np.int64)
    check(lib().dyd_repair_boxes(_ptr(box4), _ptr(row_off), n, _ptr(cls), _ptr(width), _ptr(height), _ptr(size_status),
                                 n_classes, min_visibility, min_size, _ptr(action), _ptr(out_box), _ptr(rows), _ptr(cc)),
          "dyd_repair_boxes")
    return action, out_box, rows, cc


def _compare_side(box4, row_off, cls, what: str) -> tuple:
    """one table of K18 as contiguous arrays of the kernel's dtypes, its sizes checked -> (box4, row_off, cls, n_boxes)"""
    box4 = np.ascontiguousarray(box4, dtype=np.float64).reshape(-1)
    row_off = np.ascontiguousarray(row_off, dtype=np.int32)
    if len(row_off) < 1 or row_off[0] != 0 or 4 * int(row_off[-1]) != box4.size:
        raise ValueError(f"{what}: row_off must start at 0 and end at the number of boxes")
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    if cls.size != int(row_off[-1]):
        raise ValueError(f"{what}: cls must hold one id per box")
    return box4, row_off, cls, int(row_off[-1])


def compare_boxes(a_box4, a_row_off, a_cls, b_box4, b_row_off, b_cls, n_classes: int, thr: float, by_label: bool = False):
    """K18 over host arrays: two box tables of the same rows -> (a_match [A] i32, b_match [B] i32, b_iou [B] f64, a_best [A] f64,
    b_best [B] f64, row_counts [N,4] i32, confusion [C+1,C+1] u64).  See include/dyd.h for the matching rule."""
    a_box4, a_row_off, a_cls, na = _compare_side(a_box4, a_row_off, a_cls, "A")
    b_box4, b_row_off, b_cls, nb = _compare_side(b_box4, b_row_off, b_cls, "B")
    n, n_classes = len(a_row_off) - 1, int(n_classes)
    if len(b_row_off) - 1 != n:
        raise ValueError("the two tables must cover the same rows")
    a_match, a_best = np.full(na, -1, np.int32), np.zeros(na, np.float64)
    b_match, b_iou, b_best = np.full(nb, -1, np.int32), np.zeros(nb, np.float64), np.zeros(nb, np.float64)
    rows = np.zeros((n, 4), np.int32)
    conf = np.zeros((n_classes + 1, n_classes + 1), np.uint64)
    check(lib().dyd_compare_boxes(_ptr(a_box4), _ptr(a_row_off), _ptr(a_cls), _ptr(b_box4), _ptr(b_row_off), _ptr(b_cls), n,
                                  n_classes, float(thr), int(bool(by_label)), _ptr(a_match), _ptr(b_match), _ptr(b_iou),
                                  _ptr(a_best), _ptr(b_best), _ptr(rows), _ptr(conf)), "dyd_compare_boxes")
    return a_match, b_match, b_iou, a_best, b_best, rows, conf


def _eval_match_arrays(dt_score, iou_thr, ng: int, nd: int):
    """what both matchers take and give back: the scores and thresholds as flat f64, and the seven result arrays
    (dt_state, dt_tp, dt_gt, dt_iou, dt_best per detection; gt_hit, gt_best per ground-truth object)"""
    dt_score = np.ascontiguousarray(dt_score, dtype=np.float64).reshape(-1)
    if dt_score.size != nd:
        raise ValueError("dt_score must hold one score per detection")
    iou_thr = np.ascontiguousarray(iou_thr, dtype=np.float64).reshape(-1)
    out = (np.zeros(nd, np.int32), np.zeros(nd, np.uint32), np.full(nd, -1, np.int32), np.zeros(nd, np.float64),
           np.zeros(nd, np.float64), np.zeros(ng, np.uint32), np.zeros(ng, np.float64))
    return dt_score, iou_thr, out


def eval_match_boxes(gt_box4, gt_row_off, gt_cls, dt_box4, dt_row_off, dt_cls, dt_score, n_classes: int, iou_thr,
                     max_dets: int = 100):
    """K24's matching over host arrays: a ground-truth table and a detection table with scores over the same rows ->
    (dt_state [D] i32, dt_tp [D] u32, dt_gt [D] i32, dt_iou [D] f64, dt_best [D] f64, gt_hit [G] u32, gt_best [G] f64).  See
    include/dyd.h for the rule."""
    gt_box4, gt_row_off, gt_cls, ng = _compare_side(gt_box4, gt_row_off, gt_cls, "GT")
    dt_box4, dt_row_off, dt_cls, nd = _compare_side(dt_box4, dt_row_off, dt_cls, "detections")
    n = len(gt_row_off) - 1
    if len(dt_row_off) - 1 != n:
        raise ValueError("the two tables must cover the same rows")
    dt_score, iou_thr, out = _eval_match_arrays(dt_score, iou_thr, ng, nd)
    check(lib().dyd_eval_match_boxes(_ptr(gt_box4), _ptr(gt_row_off), _ptr(gt_cls), _ptr(dt_box4), _ptr(dt_row_off), _ptr(dt_cls),
                                     _ptr(dt_score), n, int(n_classes), _ptr(iou_thr), int(iou_thr.size), int(max_dets),
                                     *map(_ptr, out)), "dyd_eval_match_boxes")
    return out


def eval_accumulate(cls, score, tp, n_classes: int, n_thresholds: int, npig, rec):
    """K24's accumulation over host arrays: the evaluated detections of a whole table in table order (class, score, matched-at
    mask), npig [C] GT boxes per class, rec [R] recall points -> (precision [C,T,R], score_at [C,T,R], recall [C,T], ap [C,T],
    best_f1 [C,T], best_score [C,T] f64, best_tp [C,T], best_dets [C,T] i64).  See include/dyd.h for the rule."""
    cls = np.ascontiguousarray(cls, dtype=np.int32).reshape(-1)
    score = np.ascontiguousarray(score, dtype=np.float64).reshape(-1)
    tp = np.ascontiguousarray(tp, dtype=np.uint32).reshape(-1)
    if not cls.size == score.size == tp.size:
        raise ValueError("cls, score and tp must hold one entry per detection")
    C_, T = int(n_classes), int(n_thresholds)
    npig = np.ascontiguousarray(npig, dtype=np.int64).reshape(-1)
    if npig.size != C_:
        raise ValueError("npig must hold one count per class")
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1)
    R = rec.size
    shape = (C_, max(T, 0))
    precision, score_at = np.zeros((*shape, R), np.float64), np.zeros((*shape, R), np.float64)
    recall, ap, f1, bs = (np.zeros(shape, np.float64) for _ in range(4))
    btp, bd = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    check(lib().dyd_eval_accumulate(_ptr(cls), _ptr(score), _ptr(tp), cls.size, C_, T, _ptr(npig), _ptr(rec), R, _ptr(precision),
                                    _ptr(score_at), _ptr(recall), _ptr(ap), _ptr(f1), _ptr(bs), _ptr(btp), _ptr(bd)),
          "dyd_eval_accumulate")
    return precision, score_at, recall, ap, f1, bs, btp, bd


def eval_match_polygons(gt_xy, gt_pt_off, gt_row_off, gt_cls, dt_xy, dt_pt_off, dt_row_off, dt_cls, dt_score, width, height,
                        n_classes: int, iou_thr, max_dets: int = 100, max_pixels_per_row: int = 1 << 26,
                        max_pairs_per_row: int = 1 << 20):
    """K25's matching over host arrays: a ground-truth polygon table and a detection table with scores over the same rows ->
    (row_status u8 [n], pair_off i64 [n+1], gt_action u8 [G], dt_action u8 [D], gt_pixels i64 [G], dt_pixels i64 [D], dt_state
    i32 [D], dt_tp u32 [D], dt_gt i32 [D], dt_iou f64 [D], dt_best f64 [D], gt_hit u32 [G], gt_best f64 [G]).  Rule and codes:
    include/dyd.h."""
    gt_xy, gt_pt_off, gt_row_off, width, height, _, gt_cls, n, ng = _poly_table(gt_xy, gt_pt_off, gt_row_off, width, height,
                                                                                ("width", width, np.float64), ("gt_cls", gt_cls, np.int32))
    dt_xy, dt_pt_off, dt_row_off, _, _, _, dt_cls, _, nd = _poly_table(dt_xy, dt_pt_off, dt_row_off, width, height,
                                                                       ("width", width, np.float64), ("dt_cls", dt_cls, np.int32))
    dt_score, iou_thr, out = _eval_match_arrays(dt_score, iou_thr, ng, nd)
    status, pair_off = np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
    g_act, d_act = np.zeros(ng, np.uint8), np.zeros(nd, np.uint8)
    g_pix, d_pix = np.zeros(ng, np.int64), np.zeros(nd, np.int64)
    opt = lambda a: _ptr(a) if a.size else None          # noqa: E731
    check(lib().dyd_eval_match_polygons(opt(gt_xy), _ptr(gt_pt_off), _ptr(gt_row_off), opt(gt_cls), opt(dt_xy), _ptr(dt_pt_off),
                                        _ptr(dt_row_off), opt(dt_cls), opt(dt_score), _ptr(width), _ptr(height), n, int(n_classes),
                                        _ptr(iou_thr), int(iou_thr.size), int(max_dets), int(max_pixels_per_row),
                                        int(max_pairs_per_row), _ptr(status), _ptr(pair_off), opt(g_act), opt(d_act), opt(g_pix),
                                        opt(d_pix), *map(opt, out)), "dyd_eval_match_polygons")
    return (status, pair_off, g_act, d_act, g_pix, d_pix, *out)


def bbox_iou_fused(xy: np.ndarray, pt_off: np.ndarray, box_off: np.ndarray, min_boxes: int, thr: float,
                   want_box: bool = False):
    """Fused K1+K2 over host arrays (one launch): (arg4 [B,4] i32, high [N] u8[, box4 [B,4] f64]).  The flag follows the
    reference's replace -> IoU chain: a row's box list ends at its first polygon without a valid point."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int32)
    box_off = np.ascontiguousarray(box_off, dtype=np.int32)
    n, nb = len(box_off) - 1, len(pt_off) - 1
    if n < 0 or nb < 0 or box_off[0] != 0 or pt_off[0] != 0 or int(box_off[-1]) != nb or 2 * int(pt_off[-1]) != xy.size:
        raise ValueError("box_off / pt_off / xy sizes disagree")
    arg = np.empty((nb, 4), np.int32)
    high = np.zeros(n, np.uint8)
    box = np.empty((nb, 4), np.float64) if want_box else None
    check(lib().dyd_bbox_iou_fused(_ptr(xy), _ptr(pt_off), _ptr(box_off), n, int(min_boxes), float(thr),
                                   _ptr(box) if want_box else None, _ptr(arg), _ptr(high)), "dyd_bbox_iou_fused")
    return (arg, high, box) if want_box else (arg, high)


def hash128(data: np.ndarray, off: np.ndarray) -> np.ndarray:
    """K3 over host arrays: [n,2] u64."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(off) - 1
    if n < 0 or off[0] != 0 or int(off[-1]) != data.size:
        raise ValueError("off must start at 0 and end at len(bytes)")
    out = np.empty((n, 2), np.uint64)
    check(lib().dyd_hash128(_ptr(data) if data.size else None, _ptr(off), n, _ptr(out)), "dyd_hash128")
    return out


def dedup(h: np.ndarray, keep) -> np.ndarray:
    """K4 over host arrays: keep-mask (uint8) for keep in {"first", "last", False}."""
    if keep not in _KEEP:
        raise ValueError('keep must be either "first", "last" or False')
    h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 2)
    out = np.empty(len(h), np.uint8)
    check(lib().dyd_dedup(_ptr(h), len(h), _KEEP[keep], _ptr(out)), "dyd_dedup")
    return out


def isin(h: np.ndarray, ref_h: np.ndarray) -> np.ndarray:
    """K5 over host arrays."""
    h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 2)
    ref_h = np.ascontiguousarray(ref_h, dtype=np.uint64).reshape(-1, 2)
    out = np.empty(len(h), np.uint8)
    check(lib().dyd_isin(_ptr(h), len(h), _ptr(ref_h) if len(ref_h) else None, len(ref_h), _ptr(out)), "dyd_isin")
    return out


def dedup_partner(h: np.ndarray) -> np.ndarray:
    """per row the first row whose hash equals its own (int64; the row itself for a first occurrence)"""
    h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 2)
    out = np.empty(len(h), np.int64)
    check(lib().dyd_dedup_partner(_ptr(h), len(h), _ptr(out)), "dyd_dedup_partner")
    return out


def isin_partner(h: np.ndarray, ref_h: np.ndarray) -> np.ndarray:
    """per main row the reference row whose hash it equals (int64, -1: none)"""
    h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 2)
    ref_h = np.ascontiguousarray(ref_h, dtype=np.uint64).reshape(-1, 2)
    out = np.empty(len(h), np.int64)
    check(lib().dyd_isin_partner(_ptr(h), len(h), _ptr(ref_h) if len(ref_h) else None, len(ref_h), _ptr(out)), "dyd_isin_partner")
    return out


def cells_differ(text_a, off_a, idx_a, text_b, off_b, idx_b, n: int) -> np.ndarray:
    """uint8 per pair: do the cells a[idx_a[i]] and b[idx_b[i]] (flat utf-8 + int64 offsets) differ?  Pairs with a negative index
    count as equal.  Host code inside the library, multithreaded; needs no GPU."""
    text_a = np.ascontiguousarray(text_a, dtype=np.uint8); text_b = np.ascontiguousarray(text_b, dtype=np.uint8)
    off_a = np.ascontiguousarray(off_a, dtype=np.int64); off_b = np.ascontiguousarray(off_b, dtype=np.int64)
    idx_a = None if idx_a is None else np.ascontiguousarray(idx_a, dtype=np.int64)
    idx_b = None if idx_b is None else np.ascontiguousarray(idx_b, dtype=np.int64)
    out = np.zeros(int(n), np.uint8)
    if n:
        load_library().dyd_host_cells_differ(_ptr(text_a) if text_a.size else None, _ptr(off_a), None if idx_a is None else _ptr(idx_a),
                                             _ptr(text_b) if text_b.size else None, _ptr(off_b), None if idx_b is None else _ptr(idx_b),
                                             int(n), 0, _ptr(out))
    return out


def mt19937_permutation(seed: int, n: int) -> np.ndarray:
    """Host code inside the library: numpy legacy RandomState(seed).permutation(n)."""
    if not (0 <= int(seed) <= 2 ** 32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")   # numpy's message (mtrand legacy seeding)
    out = np.empty(int(n), np.int64)
    check(load_library().dyd_mt19937_permutation(int(seed), int(n), _ptr(out)), "dyd_mt19937_permutation")
    return out


def mt19937_permutation_device(seed: int, n: int, want_inverse: bool = False):
    """K8: the same permutation computed in parallel on the GPU (n <= 2^30) -> perm [, inverse] as int64 host arrays"""
    if not (0 <= int(seed) <= 2 ** 32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    L = lib()
    n = int(n)
    nbytes = 8 * max(n, 1)
    d_perm, d_inv = C.c_void_p(), C.c_void_p()
    check(L.dyd_malloc(C.byref(d_perm), nbytes), "dyd_malloc")
    check(L.dyd_malloc(C.byref(d_inv), nbytes), "dyd_malloc")
    try:
        check(L.dyd_mt19937_permutation_dev(int(seed), n, d_perm, d_inv, None), "dyd_mt19937_permutation_dev")
        perm, inv = np.empty(n, np.int64), np.empty(n, np.int64)
        if n:
            check(L.dyd_d2h(_ptr(perm), d_perm, 8 * n), "dyd_d2h")
            check(L.dyd_d2h(_ptr(inv), d_inv, 8 * n), "dyd_d2h")
    finally:
        L.dyd_free(d_perm)
        L.dyd_free(d_inv)
    return (perm, inv) if want_inverse else perm


def split_ids_seeded(cat, seed: int, sizes, n_train, n_val):
    """K8 + K6 over host arrays: (split u8, pos i64); the categories' permutations are made on the device from `seed`"""
    if not (0 <= int(seed) <= 2 ** 32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    cat = np.ascontiguousarray(cat, dtype=np.int32)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    n_train = np.ascontiguousarray(n_train, dtype=np.int64)
    n_val = np.ascontiguousarray(n_val, dtype=np.int64)
    if not (len(sizes) == len(n_train) == len(n_val)):
        raise ValueError("sizes / n_train / n_val sizes disagree")
    split = np.empty(len(cat), np.uint8)
    pos = np.empty(len(cat), np.int64)
    check(lib().dyd_split_ids_seeded(_ptr(cat), len(cat), int(seed), _ptr(sizes), _ptr(n_train), _ptr(n_val), len(sizes),
                                     _ptr(split), _ptr(pos)), "dyd_split_ids_seeded")
    return split, pos


def split_ids(cat, perm_concat, cat_off, n_train, n_val):
    """K6 over host arrays: (split u8, pos i64)."""
    cat = np.ascontiguousarray(cat, dtype=np.int32)
    perm_concat = np.ascontiguousarray(perm_concat, dtype=np.int64)
    cat_off = np.ascontiguousarray(cat_off, dtype=np.int64)
    n_train = np.ascontiguousarray(n_train, dtype=np.int64)
    n_val = np.ascontiguousarray(n_val, dtype=np.int64)
    n_cat = len(n_train)
    if len(cat_off) != n_cat + 1 or len(n_val) != n_cat or int(cat_off[-1]) != len(perm_concat):
        raise ValueError("cat_off / n_train / n_val / perm sizes disagree")
    split = np.empty(len(cat), np.uint8)
    pos = np.empty(len(cat), np.int64)
    check(lib().dyd_split_ids(_ptr(cat), len(cat), _ptr(perm_concat), _ptr(cat_off), _ptr(n_train), _ptr(n_val),
                              n_cat, _ptr(split), _ptr(pos)), "dyd_split_ids")
    return split, pos


def yolo_lines(box4, row_off, sel, width, height, class_id):
    """K7 over host arrays -> (text_off int64 [n+1], flag u8 [n], text bytes).  flag 2 rows carry no text:
    the caller prints them (zero image size, values of 2^43 and more)."""
    box4 = np.ascontiguousarray(box4, dtype=np.float64).reshape(-1)
    row_off = np.ascontiguousarray(row_off, dtype=np.int32)
    n = len(row_off) - 1
    width = np.ascontiguousarray(width, dtype=np.float64)
    height = np.ascontiguousarray(height, dtype=np.float64)
    class_id = np.ascontiguousarray(class_id, dtype=np.int32)
    if n < 0 or len(width) != n or len(height) != n or len(class_id) != n:
        raise ValueError("row_off / width / height / class_id sizes disagree")
    if n and (int(row_off[-1]) * 4 != len(box4)):
        raise ValueError("row_off[-1] != number of boxes")
    sel_p = None
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.uint8)
        if len(sel) * 4 != len(box4):
            raise ValueError("sel size != number of boxes")
        sel_p = _ptr(sel)
    off = np.zeros(n + 1, np.int64)
    flag = np.zeros(n, np.uint8)
    text, total = C.c_void_p(), C.c_int64()
    check(lib().dyd_yolo_lines(_ptr(box4), _ptr(row_off), sel_p, _ptr(width), _ptr(height), _ptr(class_id), n, _ptr(off),
                               _ptr(flag), C.byref(text), C.byref(total)), "dyd_yolo_lines")
    return off, flag, _take_text(text, total)


def yolo_seg_lines(xy, pt_off, row_off, sel, width, height, class_id):
    """K13 over host arrays -> (text_off int64 [n+1], flag u8 [n], action u8 [n_polys], text bytes).  flag 2 rows carry no
    text: the caller decides them (zero image size, negative class id).  Action codes: include/dyd.h."""
    xy, pt_off, row_off, width, height, class_id, _, n, nb = _poly_table(xy, pt_off, row_off, width, height,
                                                                         ("class_id", class_id, np.int32))
    sel_p = None
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.uint8)
        if len(sel) != nb:
            raise ValueError("sel size != number of polygons")
        sel_p = _ptr(sel) if nb else None
    off = np.zeros(n + 1, np.int64)
    flag = np.zeros(n, np.uint8)
    action = np.zeros(nb, np.uint8)
    text, total = C.c_void_p(), C.c_int64()
    check(lib().dyd_yolo_seg_lines(_ptr(xy) if xy.size else None, _ptr(pt_off), _ptr(row_off), sel_p, _ptr(width), _ptr(height),
                                   _ptr(class_id), n, _ptr(off), _ptr(flag), _ptr(action) if nb else None, C.byref(text),
                                   C.byref(total)), "dyd_yolo_seg_lines")
    return off, flag, action, _take_text(text, total)


def yolo_obb_lines(xy, pt_off, row_off, sel, width, height, class_id, corners=False):
    """K17 over host arrays -> (text_off int64 [n+1], flag u8 [n], action u8 [n_polys], text bytes, clamped u8 [n_polys]), and
    with corners=True the pixel corners f64 [n_polys, 8] (x1 y1 .. x4 y4 before clamping, NaN for a polygon without a line) as a
    sixth item.  Flags as yolo_seg_lines.  Action codes: include/dyd.h (K13's and 6 flat)."""
    xy, pt_off, row_off, width, height, class_id, _, n, nb = _poly_table(xy, pt_off, row_off, width, height,
                                                                         ("class_id", class_id, np.int32))
    sel_p = None
    if sel is not None:
        sel = np.ascontiguousarray(sel, dtype=np.uint8)
        if len(sel) != nb:
            raise ValueError("sel size != number of polygons")
        sel_p = _ptr(sel) if nb else None
    off = np.zeros(n + 1, np.int64)
    flag = np.zeros(n, np.uint8)
    action = np.zeros(nb, np.uint8)
    clamped = np.zeros(nb, np.uint8)
    cor = np.full((nb, 8), np.nan) if corners else None
    text, total = C.c_void_p(), C.c_int64()
    check(lib().dyd_yolo_obb_lines(_ptr(xy) if xy.size else None, _ptr(pt_off), _ptr(row_off), sel_p, _ptr(width), _ptr(height),
                                   _ptr(class_id), n, _ptr(off), _ptr(flag), _ptr(action) if nb else None,
                                   _ptr(clamped) if nb else None, _ptr(cor) if corners and nb else None, C.byref(text),
                                   C.byref(total)), "dyd_yolo_obb_lines")
    res = (off, flag, action, _take_text(text, total), clamped)
    return res + (cor,) if corners else res
