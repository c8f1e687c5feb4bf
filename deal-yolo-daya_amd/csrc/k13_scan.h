// k13_scan.h — the int64 inclusive scan of k13_seg.hip (reduce, scan of the block sums, apply), for the kernels that turn
// byte counts into text offsets: K13 and K17 over rows, K16 over polygons.  The kernels live in k13_seg.hip.
#pragma once

#include "dyd_common.h"

namespace dyd {

int64_t k13_scan_parts(int64_t n);   // int64 entries of scratch the scan of n values needs
// v[0..n) -> its inclusive prefix sums, in place, on st
void k13_scan_inclusive(int64_t *v, int64_t n, int64_t *part, hipStream_t st);

}  // namespace dyd
