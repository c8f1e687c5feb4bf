// poly_table.h — what the host-pointer entries of the polygon steps K13 (k13_seg.hip), K14 (k14_poly_audit.hip), K16
// (k16_coco.hip), K17 (k17_obb.hip), K20 (k20_tile.hip), K21 (k21_raster.hip), K22 (k22_poly_compare.hip, two tables) and K23 (k23_rle.hip) share: the checks of a polygon table in host memory and its staging in device memory.  The polygon twin of
// box_table.h; the device code the three kernels share is in k13_poly.h (polygon, clip, walk, row search) and k13_scan.h (scan,
// print window).
//
// A polygon table: xy = P x (x, y) f64, pt_off = B+1 int32, row_off = N+1 int32, width / height = N f64, and per step one or
// two columns of its own (K13 and K17: sel = B u8, class_id = N int32; K14: cls = B int32, size_status = N u8; K16: cat_id = B int32,
// size_status = N u8; K20 (k20_tile.hip): cls = B int32; K21 (k21_raster.hip): val = B int32; K23 (k23_rle.hip): sel = B int32), which each entry checks for NULL and uploads itself.
// K19 (k19_simplify.hip) has no rows: it passes one row that holds every polygon through the same checks and stages xy and
// pt_off with poly_column.
#pragma once

#include "dyd_common.h"

namespace dyd {

// Checks a polygon table in host memory and sets *n_polys = row_off[n_rows], *n_points = pt_off[n_polys].  row_cols / poly_cols
// say whether the entry's own per-row / per-polygon pointers (columns and outputs) are all set.  cls (optional): class ids that
// must lie in -1..n_classes-1 (K14).
inline int poly_table_check(const double *xy, const int32_t *pt_off, const int32_t *row_off, int64_t n_rows, const double *width,
                            const double *height, bool row_cols, bool poly_cols, const int32_t *cls, int32_t n_classes,
                            int64_t *n_polys, int64_t *n_points) {
    int64_t nb = 0, np = 0;
    if (n_rows > 0) {
        DYD_REQUIRE(row_off && width && height && row_cols, "null pointer");
        DYD_REQUIRE(row_off[0] == 0, "row_off[0] != 0");
        for (int64_t i = 0; i < n_rows; ++i) DYD_REQUIRE(row_off[i + 1] >= row_off[i], "row_off not monotone");
        nb = row_off[n_rows];
    }
    if (nb > 0) {
        DYD_REQUIRE(pt_off && poly_cols, "null pointer");
        DYD_REQUIRE(pt_off[0] == 0, "pt_off[0] != 0");
        for (int64_t p = 0; p < nb; ++p) {
            DYD_REQUIRE(pt_off[p + 1] >= pt_off[p], "pt_off not monotone");
            if (cls) DYD_REQUIRE(cls[p] >= -1 && cls[p] < n_classes, "class id outside -1..n_classes-1");
        }
        np = pt_off[nb];
        DYD_REQUIRE(np == 0 || xy, "null pointer");
    }
    *n_polys = nb;
    *n_points = np;
    return DYD_OK;
}

// A checked polygon table of nb polygons and np points copied to device memory on the library's stream.
struct PolyTableDev {
    DevBuf xy, pt, row, w, h;

    int upload(const double *xy_, const int32_t *pt_off, const int32_t *row_off, const double *width, const double *height,
               int64_t n_rows, int64_t nb, int64_t np) {
        int rc;
        if ((rc = xy.alloc(16 * (size_t)np)) || (rc = pt.alloc(4 * (size_t)(nb + 1))) || (rc = row.alloc(4 * (size_t)(n_rows + 1))) ||
            (rc = w.alloc(8 * (size_t)n_rows)) || (rc = h.alloc(8 * (size_t)n_rows)))
            return rc;
        hipStream_t s = ctx().stream;
        if (np) DYD_HIP(hipMemcpyAsync(xy.p, xy_, 16 * (size_t)np, hipMemcpyHostToDevice, s));
        if (nb) DYD_HIP(hipMemcpyAsync(pt.p, pt_off, 4 * (size_t)(nb + 1), hipMemcpyHostToDevice, s));
        if (n_rows) {
            DYD_HIP(hipMemcpyAsync(row.p, row_off, 4 * (size_t)(n_rows + 1), hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(w.p, width, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            DYD_HIP(hipMemcpyAsync(h.p, height, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
        }
        return DYD_OK;
    }
};

// one more column of the table (or an output buffer, src = NULL) in device memory
inline int poly_column(DevBuf &d, const void *src, size_t bytes) {
    int rc = d.alloc(bytes);
    if (rc) return rc;
    if (src && bytes) DYD_HIP(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, ctx().stream));
    return DYD_OK;
}

}  // namespace dyd
