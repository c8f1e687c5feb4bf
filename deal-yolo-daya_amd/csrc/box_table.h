// box_table.h — what the box steps K10 (k10_audit.hip) and K11 (k11_repair.hip) share: the wave sync of their row-tile walks,
// and the checks and staging of the box table for their host-pointer entries.  The row-tile walk itself stays written out in
// each kernel: moved into one shared function (driven by lambdas, or only its lane -> row search) it left the resource usage
// unchanged but not the code, and K10 ran 1.8 % slower on MI355X (10 M rows, 20 classes, nb = 16).
//
// A box table in HBM: box4 = B x (x1, y1, x2, y2) f64 (16-B aligned), row_off = N+1 int32, cls = B int32, width / height =
// N f64, size_status = N u8 (0 ok, 1 missing, 2 invalid).
#pragma once

#include "dyd_common.h"

namespace dyd {

__device__ __forceinline__ void box_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Host-pointer entries: checks a box table in host memory and sets *n_boxes = row_off[n_rows].  row_outs / box_outs say whether
// the entry's per-row / per-box output pointers are all set.
inline int box_table_check(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls, const double *width,
                           const double *height, const uint8_t *size_status, int32_t n_classes, bool row_outs, bool box_outs,
                           int64_t *n_boxes) {
    int64_t nb = 0;
    if (n_rows > 0) {
        DYD_REQUIRE(row_off && width && height && size_status && row_outs, "null pointer");
        DYD_REQUIRE(row_off[0] == 0, "row_off[0] != 0");
        for (int64_t i = 0; i < n_rows; ++i) DYD_REQUIRE(row_off[i + 1] >= row_off[i], "row_off not monotone");
        nb = row_off[n_rows];
    }
    if (nb > 0) {
        DYD_REQUIRE(box4 && cls && box_outs, "null pointer");
        for (int64_t b = 0; b < nb; ++b) DYD_REQUIRE(cls[b] >= -1 && cls[b] < n_classes, "class id outside -1..n_classes-1");
    }
    *n_boxes = nb;
    return DYD_OK;
}

// A checked box table of nb boxes copied to device memory on the library's stream.
struct BoxTableDev {
    DevBuf box, off, cls, w, h, st;

    int upload(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls_, const double *width,
               const double *height, const uint8_t *size_status, int64_t nb) {
        int rc;
        if ((rc = box.alloc(32 * (size_t)nb)) || (rc = off.alloc(4 * (size_t)(n_rows + 1))) || (rc = cls.alloc(4 * (size_t)nb)) ||
            (rc = w.alloc(8 * (size_t)n_rows)) || (rc = h.alloc(8 * (size_t)n_rows)) || (rc = st.alloc((size_t)n_rows)))
            return rc;
        hipStream_t s = ctx().stream;
        if (nb) {
            DYD_HIP(hipMemcpyAsync(box.p, box4, 32 * (size_t)nb, hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(cls.p, cls_, 4 * (size_t)nb, hipMemcpyHostToDevice, s));
        }
        if (n_rows) {
            DYD_HIP(hipMemcpyAsync(off.p, row_off, 4 * (size_t)(n_rows + 1), hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(w.p, width, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(h.p, height, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(st.p, size_status, (size_t)n_rows, hipMemcpyHostToDevice, s));
        }
        return DYD_OK;
    }
};

}  // namespace dyd
