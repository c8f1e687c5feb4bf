// k21_cover.h — the pixel rule of include/dyd.h (centre sampling, canonical edge direction, even-odd), once, for the two steps
// that scan-convert polygons: K21 (k21_raster.hip, label masks) and K22 (k22_poly_compare.hip, mask IoU).  Here: the row rule,
// the action codes, the polygons of a row, the strip of an item (the struct), the box cull and the edge -> crossing list -> parity step.
// What a step does with the parity (K21: a byte per pixel in LDS, K22: a bit per pixel in a register) stays in its own file.
// DESIGN §5s has the mapping and its cost.
#pragma once

#include "k13_poly.h"

namespace dyd {

enum : uint8_t { COVER_DONE = 0, COVER_NO_ROW = 5 };   // a polygon's action; the other actions are K13's codes

inline int k21_capped(int v, int most) { return v > 0 ? (v < most ? v : most) : most; }   // an option: <= 0 is the default

// row status (0 rasterised, 1 no_size, 2 fractional_size, 3 too_large); for status 0 the image's width and height
__device__ __forceinline__ uint8_t k21_row_size(double W, double H, int64_t max_pixels, int64_t *w, int64_t *h) {
    *w = *h = 0;
    if (!k13_size_ok(W) || !k13_size_ok(H)) return 1;
    if (W != floor(W) || H != floor(H)) return 2;
    const int64_t iw = (int64_t)W, ih = (int64_t)H;
    if (iw > max_pixels || ih > max_pixels || iw * ih > max_pixels) return 3;   // the product stays at or below 2^60
    *w = iw;
    *h = ih;
    return 0;
}

// the polygons [first, last) of row r, clamped as K13 clamps them
__device__ __forceinline__ void k21_row_polys(const int32_t *__restrict__ row_off, int64_t r, int64_t n_polys, int64_t *first,
                                              int64_t *last) {
    const int64_t a = max((int64_t)row_off[r], (int64_t)0), b = min((int64_t)row_off[r + 1], n_polys);
    *first = a;
    *last = max(b, a);
}

// A lane per polygon: action (COVER_DONE, COVER_NO_ROW for a row of status != 0, SEG_UNSELECTED for val < 0, else K13's code)
// and info[4p .. 4p+3] = x1, y1, x2, y2 of the points, which is the box of V.  The kernel lives in k21_raster.hip.
void k21_polys(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const uint8_t *row_status,
               int64_t n_rows, int64_t n_polys, int64_t n_points, uint8_t *action, double *info, hipStream_t st);

// The strip of an item = (row, scanline, strip of `strip` columns): the centres of its scanline and of its first and last pixel,
// its first column, its pixels and the 64-pixel words that hold them.  Each paint kernel decodes its item into one itself: as
// a shared function the decode moved the scalar registers of both kernels.
struct K21Strip {
    double yc, xc_first, xc_last;
    int64_t x0;
    int npx, n_words;
};

// The cull: false when polygon p cannot cover a pixel centre of the strip.  No edge crosses the scanline unless by1 <= yc < by2.
// A crossing lies within an ulp of [bx1, bx2]: to the right of the box (with a pixel to spare) no crossing has xs > xc; to the
// left every one has, and a closed outline crosses a scanline an even number of times, so the parity stays 0.
__device__ __forceinline__ bool k21_reaches(const uint8_t *__restrict__ action, const double *__restrict__ info, int64_t p,
                                            const K21Strip &s) {
    if (action[p] != COVER_DONE) return false;
    const double *q = info + 4 * p;
    const double bx1 = q[0], by1 = q[1], bx2 = q[2], by2 = q[3];
    return by1 <= s.yc && s.yc < by2 && !(s.xc_first >= bx2 + 1.0) && !(s.xc_last <= bx1 - 1.0);
}

// The edge step of one polygon on the scanline yc, by a wave: pts[0 .. n) are its points, box = x1, y1, x2, y2 its box (a
// two-point polygon stands for the four corners).  Lanes take edges in chunks of 64 and compute xs for the crossing ones (one
// division per edge and scanline); a ballot and a popcount compact them into `list` (LDS, capacity cap); apply(n_listed) XORs
// xs > xc for the listed crossings into the caller's parity.  A full list is applied and emptied: parity is linear in the
// crossings, so any edge count is exact.  Ends with the last apply.
template <class Apply>
__device__ __forceinline__ void k21_edges(const double2 *__restrict__ pts, int n, const double *__restrict__ box, double yc,
                                          int cap, double *list, Apply apply) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const double bx1 = box[0], by1 = box[1], bx2 = box[2], by2 = box[3];
    const bool two = n == 2;
    const int m = two ? 4 : n;
    int n_listed = 0;
    for (int k0 = 0; k0 < m; k0 += kWave) {
        const int k = k0 + lane;
        bool cross = false;
        double xs = 0.0;
        if (k < m) {
            const int kn = k + 1 == m ? 0 : k + 1;
            double ax, ay, bx, by;
            if (two) {   // the corners (x1, y1), (x2, y1), (x2, y2), (x1, y2) of the box
                ax = k == 0 || k == 3 ? bx1 : bx2;
                ay = k < 2 ? by1 : by2;
                bx = kn == 0 || kn == 3 ? bx1 : bx2;
                by = kn < 2 ? by1 : by2;
            } else {
                const double2 A = pts[k], B = pts[kn];
                ax = A.x; ay = A.y; bx = B.x; by = B.y;
            }
            const bool swap = ay > by || (ay == by && ax > bx);   // the canonical direction
            const double Px = swap ? bx : ax, Py = swap ? by : ay, Qx = swap ? ax : bx, Qy = swap ? ay : by;
            if (Py != Qy && Py <= yc && yc < Qy) {
                cross = true;
                const double t = yc - Py, d = Qx - Px;
                const double num = t * d;
                xs = Px + num / (Qy - Py);
            }
        }
        const unsigned long long mask = __ballot(cross);
        const int rank = __popcll(mask & below), count = __popcll(mask);
        for (int done = 0; done < count;) {
            const int take = min(cap - n_listed, count - done);
            if (cross && rank >= done && rank < done + take) list[n_listed + rank - done] = xs;
            n_listed += take;
            done += take;
            if (n_listed == cap) {
                apply(n_listed);
                n_listed = 0;
            }
        }
    }
    apply(n_listed);
}

}  // namespace dyd
