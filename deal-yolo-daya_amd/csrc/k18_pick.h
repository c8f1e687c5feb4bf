// k18_pick.h — the pieces of the greedy matcher that K18 (k18_compare.hip: k18_big_rows_kernel, boxes) and K22
// (k22_poly_compare.hip: k22_match_kernel, polygons by mask IoU) share: an IoU as a sort key and a count in the confusion
// matrix in device memory.  The wave's arg-max over the candidates of one B object (largest key, then the lowest index among
// its holders, the largest best key carried along) stays written out in both kernels: as a function, in four spellings, it
// moved the register count of k18_big_rows_kernel.
#pragma once

#include "dyd_common.h"

namespace dyd {

// sort keys of an IoU (IoU >= 0 orders like its u64 bits): `best` key (0 for NaN and 0.0) and candidate key (bits + 1; 0 = no
// candidate)
__device__ __forceinline__ unsigned long long k18_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double k18_value(unsigned long long k) { return __longlong_as_double((long long)k); }
__device__ __forceinline__ unsigned long long k18_best_key(double iou) { return (iou > 0.0) ? k18_bits(iou) : 0ull; }
__device__ __forceinline__ unsigned long long k18_cand_key(double iou) { return k18_bits(iou) + 1ull; }

// one count in confusion[a][b]; a, b in 0..C (C = none), anything else (a class id outside the list) is not counted
__device__ __forceinline__ void k18_count(unsigned long long *conf, int32_t C, int32_t a, int32_t b) {
    if ((uint32_t)a > (uint32_t)C || (uint32_t)b > (uint32_t)C) return;
    atomicAdd(conf + (int64_t)a * (C + 1) + b, 1ull);
}

}  // namespace dyd
