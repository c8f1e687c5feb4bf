// k22_pairs.h — the pair step of K22 (k22_poly_compare.hip: rows, polygons, paint into the pair table, pixel counts) as K25
// (k25_poly_eval.hip, scored polygon evaluation) calls it: the tables and outputs as the step takes them, and the step itself.
// Host code only; the kernels stay in k22_poly_compare.hip.
#pragma once

#include "sized_out.h"

namespace dyd {

constexpr uint8_t CMP_ROW_PAIRS = 4;         // row status: more pairs than max_pairs_per_row

// one table of a comparison in device memory with its outputs; match and best belong to K22's matcher alone
struct K22Table {
    const double *xy;
    const int32_t *pt_off, *row_off, *cls;
    int64_t n_polys, n_points;
    uint8_t *action;
    int64_t *pixels;
    int32_t *match;
    double *best;
};

// b_iou, row_counts and confusion belong to K22's matcher; pixel_confusion and row_pixels to the comparison flavour of the paint
struct K22Out {
    uint8_t *row_status;
    int64_t *pair_off;
    double *b_iou;
    int32_t *row_counts;
    uint64_t *confusion, *pixel_confusion;
    int64_t *row_pixels;
};

int compare_params(int32_t n_classes, int64_t max_pixels, int64_t max_pairs);

// Steps 1 to 3 of K22 on device pointers: row_status, pair_off, both sides' action and pixels, and the pair table, which
// `pairs_out` is asked for once its size is known (it fails before anything but row_status and pair_off is written).
// for_eval: the evaluation flavour of the paint kernel, which touches neither matrix nor row_pixels and leaves the cells of
// pairs of different classes at 0; otherwise the comparison flavour, with the three counters of `o` cleared first.
int compare_pairs_launch(const K22Table &a, const K22Table &b, const double *width, const double *height, int64_t n_rows, int32_t C,
                         int64_t max_pixels, int64_t max_pairs, const K22Out &o, bool for_eval, SizedOut &pairs_out, hipStream_t st);

}  // namespace dyd
