// k13_poly.h — the polygon handling K13 (k13_seg.hip), K14 (k14_poly_audit.hip) and K16 (k16_coco.hip) share: a polygon's
// checks before clipping, its vertex list V, the Sutherland-Hodgman pipeline that clips it to the image (include/dyd.h, DESIGN
// §5l) and the walk over the clipped vertices that decides `empty` and gives the area; the search of an offsets array and a
// polygon tile's row range.  K14 and K16 give every polygon the action K13 would give it by calling this same code; K20
// (k20_tile.hip) runs the same clip and walk once per tile on the polygon moved to the tile's origin.
//
// Two pieces stay written out in their kernels, because sharing them changed a kernel's registers (the rule of box_table.h:
// a helper has to cost nothing).  K14 keeps its own copy of ClipWalk's walk: through the struct k14_poly_kernel takes 105 VGPRs
// instead of 103.  K13 and K16 keep their print windows (LDS image, base / wlo / whi, put, the 16-byte stream-out): one struct
// for both, with the image as a member, an argument or an array reference, took k13_print_kernel from 78 VGPRs and no scratch
// to 106 VGPRs and 16 bytes of scratch per lane.
#pragma once

#include "dyd_common.h"

namespace dyd {

constexpr double K13_LIMIT = 8796093022208.0;   // 2^43: |coordinate|, W and H stay below it

enum : uint8_t { SEG_WRITTEN = 0, SEG_CLIPPED = 1, SEG_BAD_COORDS = 2, SEG_TOO_FEW = 3, SEG_EMPTY = 4, SEG_NO_SIZE = 5,
                 SEG_UNSELECTED = 255 };

__device__ __forceinline__ bool k13_size_ok(double v) { return v > 0.0 && v < K13_LIMIT; }   // false for NaN

// The polygon's vertex list V: the points as given, or for exactly two points the four corners of their box.
struct Poly {
    const double *p;   // 2*n values
    int n;
    double x1, y1, x2, y2;   // bounding box of the points
    // V[k] to f(x, y) for k = 0 .. count-1 while f returns true (two points: the corners, unrolled, so that the box stays in registers)
    template <class F>
    __device__ __forceinline__ void each(F &f) const {
        if (n == 2) {
            if (f(x1, y1) && f(x2, y1) && f(x2, y2)) f(x1, y2);
            return;
        }
        for (int k = 0; k < n; ++k) {
            const double2 v = *reinterpret_cast<const double2 *>(p + 2 * k);
            if (!f(v.x, v.y)) return;
        }
    }
};

// One clip pass: its first input vertex, the previous one and whether that was inside.
struct ClipPass {
    double fx, fy, px, py;
    bool pin, any;
};

// The four clip passes as a pipeline.  K: 0 x >= 0, 1 x <= W, 2 y >= 0, 3 y <= H.  One named member per pass (not an array
// indexed by K) keeps the state in registers.
struct Clip {
    double W, H;
    ClipPass s0, s1, s2, s3;

    __device__ __forceinline__ Clip(double w, double h) : W(w), H(h) { s0.any = s1.any = s2.any = s3.any = false; }
    template <int K>
    __device__ __forceinline__ ClipPass &pass() {
        if constexpr (K == 0) return s0;
        else if constexpr (K == 1) return s1;
        else if constexpr (K == 2) return s2;
        else return s3;
    }
    template <int K>
    __device__ __forceinline__ bool inside(double x, double y) const {
        if constexpr (K == 0) return x >= 0.0;
        else if constexpr (K == 1) return x <= W;
        else if constexpr (K == 2) return y >= 0.0;
        else return y <= H;
    }
    template <int K, class Out>
    __device__ __forceinline__ void edge(double ax, double ay, bool ain, double bx, double by, bool bin, Out &out) {
        if (ain) push<K + 1>(ax, ay, out);
        if (ain != bin) {
            if constexpr (K < 2) {
                const double c = (K == 0) ? 0.0 : W;
                const double t = (c - ax) / (bx - ax);
                push<K + 1>(c, ay + t * (by - ay), out);
            } else {
                const double c = (K == 2) ? 0.0 : H;
                const double t = (c - ay) / (by - ay);
                push<K + 1>(ax + t * (bx - ax), c, out);
            }
        }
    }
    template <int K, class Out>
    __device__ __forceinline__ void push(double x, double y, Out &out) {
        if constexpr (K == 4) {
            out(x, y);
        } else {
            ClipPass &st = pass<K>();
            const bool in = inside<K>(x, y);
            if (!st.any) {
                st.any = true;
                st.fx = x;
                st.fy = y;
            } else {
                edge<K>(st.px, st.py, st.pin, x, y, in, out);
            }
            st.px = x;
            st.py = y;
            st.pin = in;
        }
    }
    template <int K, class Out>
    __device__ __forceinline__ void close(Out &out) {
        if constexpr (K < 4) {
            ClipPass &st = pass<K>();
            if (st.any) edge<K>(st.px, st.py, st.pin, st.fx, st.fy, inside<K>(st.fx, st.fy), out);
            close<K + 1>(out);
        }
    }
};

// the polygon's vertices after clipping, in order, to out(x, y); out returns false to stop early.  P: Poly, or K20's polygon
// seen from a tile (its each() hands out the translated vertices)
template <class P, class Out>
__device__ __forceinline__ void k13_vertices(const P &pg, bool needs_clip, double W, double H, Out &out) {
    if (!needs_clip) {
        pg.each(out);
        return;
    }
    Clip c(W, H);
    bool go = true;
    auto sink = [&](double x, double y) { if (go) go = out(x, y); };
    auto feed = [&](double x, double y) {
        c.push<0>(x, y, sink);
        return go;
    };
    pg.each(feed);
    if (go) c.close<0>(sink);
}

// V's checks before clipping: -> action (SEG_BAD_COORDS, SEG_TOO_FEW) or 0xff to go on; bounding box in the Poly's box fields
__device__ __forceinline__ uint8_t k13_prepare(const double *xy, int32_t a, int32_t b, Poly &pg) {
    pg.p = xy + 2 * (int64_t)a;
    pg.n = b - a;
    double lx = 0.0, ly = 0.0, hx = 0.0, hy = 0.0;
    bool bad = false;
    for (int k = 0; k < pg.n; ++k) {
        const double2 v = *reinterpret_cast<const double2 *>(pg.p + 2 * k);
        bad |= !(fabs(v.x) < K13_LIMIT) || !(fabs(v.y) < K13_LIMIT);   // NaN and inf fail too
        if (k == 0) { lx = hx = v.x; ly = hy = v.y; }
        lx = fmin(lx, v.x); hx = fmax(hx, v.x);
        ly = fmin(ly, v.y); hy = fmax(hy, v.y);
    }
    pg.x1 = lx; pg.y1 = ly; pg.x2 = hx; pg.y2 = hy;
    if (bad) return SEG_BAD_COORDS;
    if (pg.n < 2) return SEG_TOO_FEW;
    return 0xff;
}

template <class P>
__device__ __forceinline__ bool k13_outside(const P &pg, double W, double H) {
    return pg.x1 < 0.0 || pg.x2 > W || pg.y1 < 0.0 || pg.y2 > H;
}

// What the steps take from one pass over the clipped vertices C: their count, extent and shoelace sum.
struct ClipWalk {
    int m = 0;
    double lx = 0.0, ly = 0.0, hx = 0.0, hy = 0.0, fx = 0.0, fy = 0.0, px = 0.0, py = 0.0, s = 0.0;

    __device__ __forceinline__ void add(double x, double y) {
        if (m == 0) { lx = hx = fx = x; ly = hy = fy = y; }
        else s += px * y - x * py;
        lx = fmin(lx, x); hx = fmax(hx, x);
        ly = fmin(ly, y); hy = fmax(hy, y);
        px = x; py = y;
        ++m;
    }
    __device__ __forceinline__ bool empty() const { return m < 3 || !(hx - lx > 0.0) || !(hy - ly > 0.0); }
    // |shoelace sum| * 0.5, the closing edge included
    __device__ __forceinline__ double area() const { return fabs(s + (px * fy - fx * py)) * 0.5; }
};

// last i in [lo, hi] with off[i] <= x (off non-decreasing, off[lo] <= x)
template <class T>
__device__ __forceinline__ int64_t last_le(const T *off, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {   // invariant: off[lo] <= x; answer in [lo, hi]
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A lane per polygon over the tile [p0, p1): two lanes find the rows of its first and last polygon (rows[0], rows[1], in LDS),
// every lane then searches its own row only between them.  Ends with a barrier.
__device__ __forceinline__ void poly_tile_rows(const int32_t *__restrict__ row_off, int64_t n_rows, int64_t p0, int64_t p1, int32_t *rows) {
    if (threadIdx.x < 2) rows[threadIdx.x] = (int32_t)last_le(row_off, 0, n_rows - 1, threadIdx.x == 0 ? p0 : p1 - 1);
    __syncthreads();
}

}  // namespace dyd
