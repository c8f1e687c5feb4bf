// k18_pick.h — the pieces of the greedy matcher that K18 (k18_compare.hip: k18_big_rows_kernel, boxes) and K22
// (k22_poly_compare.hip: k22_match_kernel, polygons by mask IoU) share: an IoU as a sort key and a count in the confusion
// matrix in device memory.  The wave's arg-max over the candidates of one B object (largest key, then the lowest index among
// its holders, the largest best key carried along) stays written out in both kernels: as a function, in four spellings, it
// moved the register count of k18_big_rows_kernel.  K24 (k24_eval.hip, scored evaluation) takes from here the box
// load, the pair IoU (K2's arithmetic, the first box's area handed in), the keys, and the host side's check and upload of a table;
// K25 (k25_poly_eval.hip, scored polygon evaluation) the keys alone, both through eval_match.h, which holds what those two share.
#pragma once

#include "k2_wave.h"

namespace dyd {

// sort keys of an IoU (IoU >= 0 orders like its u64 bits): `best` key (0 for NaN and 0.0) and candidate key (bits + 1; 0 = no
// candidate)
__device__ __forceinline__ unsigned long long k18_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double k18_value(unsigned long long k) { return __longlong_as_double((long long)k); }
__device__ __forceinline__ unsigned long long k18_best_key(double iou) { return (iou > 0.0) ? k18_bits(iou) : 0ull; }
__device__ __forceinline__ unsigned long long k18_cand_key(double iou) { return k18_bits(iou) + 1ull; }

__device__ __forceinline__ Corners k18_load(const double *box4, int64_t b) {
    const double2 *g = reinterpret_cast<const double2 *>(box4 + 4 * b);
    return normalise(g[0], g[1]);
}

// calculate_iou(a, b) :328-339, a_ar = area of a.  NO_NAN as in pair_hits (k2_wave.h): the same value from v_max_f64 / v_min_f64.
template <bool NO_NAN>
__device__ __forceinline__ double k18_iou(const Corners &a, const Corners &b, double a_ar) {
    double ix1, iy1, ix2, iy2, w, h;
    if (NO_NAN) {
        ix1 = vmax(a.x1, b.x1);
        iy1 = vmax(a.y1, b.y1);
        ix2 = vmin(a.x2, b.x2);
        iy2 = vmin(a.y2, b.y2);
        w = vmax0(ix2 - ix1);
        h = vmax0(iy2 - iy1);
    } else {
        ix1 = (b.x1 > a.x1) ? b.x1 : a.x1;
        iy1 = (b.y1 > a.y1) ? b.y1 : a.y1;
        ix2 = (b.x2 < a.x2) ? b.x2 : a.x2;
        iy2 = (b.y2 < a.y2) ? b.y2 : a.y2;
        w = ix2 - ix1;
        h = iy2 - iy1;
        w = (w > 0.0) ? w : 0.0;
        h = (h > 0.0) ? h : 0.0;
    }
    const double inter = w * h;
    if (inter == 0.0) return 0.0;
    const double uni = a_ar + area_of(b) - inter;
    return (uni != 0.0) ? inter / uni : 0.0;
}

// one count in confusion[a][b]; a, b in 0..C (C = none), anything else (a class id outside the list) is not counted
__device__ __forceinline__ void k18_count(unsigned long long *conf, int32_t C, int32_t a, int32_t b) {
    if ((uint32_t)a > (uint32_t)C || (uint32_t)b > (uint32_t)C) return;
    atomicAdd(conf + (int64_t)a * (C + 1) + b, 1ull);
}

// one side of a comparison in host memory: offsets monotone from 0, class ids inside the list -> *n_boxes
inline int k18_check_side(const double *box4, const int32_t *row_off, const int32_t *cls, int64_t n_rows, int32_t n_classes,
                          int64_t *n_boxes) {
    DYD_REQUIRE(row_off, "null pointer");
    DYD_REQUIRE(row_off[0] == 0, "row_off[0] != 0");
    for (int64_t i = 0; i < n_rows; ++i) DYD_REQUIRE(row_off[i + 1] >= row_off[i], "row_off not monotone");
    const int64_t nb = row_off[n_rows];
    if (nb > 0) {
        DYD_REQUIRE(box4 && cls, "null pointer");
        for (int64_t b = 0; b < nb; ++b) DYD_REQUIRE(cls[b] >= 0 && cls[b] < n_classes, "class id outside 0..n_classes-1");
    }
    *n_boxes = nb;
    return DYD_OK;
}

struct K18Side {
    DevBuf box, off, cls;
    int upload(const double *box4, const int32_t *row_off, const int32_t *cls_, int64_t n_rows, int64_t nb) {
        int rc;
        if ((rc = box.alloc(32 * (size_t)nb)) || (rc = off.alloc(4 * (size_t)(n_rows + 1))) || (rc = cls.alloc(4 * (size_t)nb)))
            return rc;
        hipStream_t s = ctx().stream;
        if (nb) {
            DYD_HIP(hipMemcpyAsync(box.p, box4, 32 * (size_t)nb, hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(cls.p, cls_, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
        }
        DYD_HIP(hipMemcpyAsync(off.p, row_off, 4 * (size_t)(n_rows + 1), hipMemcpyHostToDevice, s));
        return DYD_OK;
    }
};

}  // namespace dyd
