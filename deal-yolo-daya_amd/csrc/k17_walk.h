// k17_walk.h — the geometry of K17 (k17_obb.hip): the minimum-area enclosing rectangle of a polygon's clipped vertices, by the
// rules of include/dyd.h (K17 block) and DESIGN §5o.  Every min and max is a strict comparison (the first value wins a tie),
// never fmin / fmax; IEEE f64 without contraction.
#pragma once

#include "k13_poly.h"

namespace dyd {

constexpr uint8_t OBB_FLAT = 6;

// The rectangle of one hull edge from (ex, ey) along (dx, dy): u in [a, b] along it, v in [e, f] across it.  An axis-aligned
// edge stands for C's own extent and keeps no numbers.
struct ObbRect {
    double ex, ey, dx, dy, a, b, e, f;
    bool axis;
};

// A prepared polygon (k13_prepare gave 0xff) -> its action: SEG_EMPTY, OBB_FLAT, or SEG_WRITTEN / SEG_CLIPPED with the corners
// x1 y1 .. x4 y4 in c (indexed by constants only) and `clamped`.  One pass over the clipped vertices C for K13's count and
// `empty`, C's extent and the start, then one pass per hull edge that takes the extents along the edge found last and selects
// the next edge at once; every pass runs the clip again, so the state is O(1).  An unclipped two-point polygon is its box.
__device__ __forceinline__ uint8_t k17_rectangle(const Poly &pg, bool clip, double W, double H, double (&c)[8], uint8_t &clamped) {
    double lx, ly, hx, hy, area;         // C's extent; the kept rectangle's area
    ObbRect kept;
    kept.axis = true;
    bool empty, any = false;
    if (pg.n == 2 && !clip) {            // the box itself: its first edge is axis-aligned and no later one is smaller
        lx = pg.x1; ly = pg.y1; hx = pg.x2; hy = pg.y2;
        empty = !(hx - lx > 0.0) || !(hy - ly > 0.0);
        area = (hx - lx) * (hy - ly);
        any = true;
    } else {
        ClipWalk w;                      // K13's count and its `empty`
        double sx = 0.0, sy = 0.0;       // the start: the first lowest vertex, the leftmost of those
        lx = ly = hx = hy = 0.0;
        auto scan = [&](double x, double y) {
            const bool f0 = w.m == 0;    // selects, not branches: conditional stores to captured values cost scratch
            const bool low = f0 || y < sy || (y == sy && x < sx);
            sx = low ? x : sx;
            sy = low ? y : sy;
            lx = (f0 || x < lx) ? x : lx;
            hx = (f0 || x > hx) ? x : hx;
            ly = (f0 || y < ly) ? y : ly;
            hy = (f0 || y > hy) ? y : hy;
            w.add(x, y);
            return true;
        };
        k13_vertices(pg, clip, W, H, scan);
        empty = w.empty();
        area = 0.0;
        if (!empty) {
            const int m = w.m;
            double cx = sx, cy = sy;                     // cur
            double ex = 0.0, ey = 0.0, dx = 0.0, dy = 0.0;   // the edge found last: its extents are taken in this pass
            bool have = false, last = false;
            for (int steps = 0;;) {
                double bx = 0.0, by = 0.0, bd = 0.0;     // best and its squared distance from cur
                double ua = 0.0, ub = 0.0, ve = 0.0, vf = 0.0;
                bool hb = false, first = true;
                auto pass = [&](double x, double y) {
                    const double u = (x - ex) * dx + (y - ey) * dy;   // all zero before the first edge
                    const double v = (y - ey) * dx - (x - ex) * dy;
                    ua = (first || u < ua) ? u : ua;
                    ub = (first || u > ub) ? u : ub;
                    ve = (first || v < ve) ? v : ve;
                    vf = (first || v > vf) ? v : vf;
                    first = false;
                    const double kx = x - cx, ky = y - cy;
                    const double d = kx * kx + ky * ky;
                    const double cr = (bx - cx) * ky - (by - cy) * kx;
                    const bool take = !last && (x != cx || y != cy) && (!hb || cr < 0.0 || (cr == 0.0 && d > bd));
                    bx = take ? x : bx;
                    by = take ? y : by;
                    bd = take ? d : bd;
                    hb |= take;
                    return true;
                };
                k13_vertices(pg, clip, W, H, pass);
                if (have) {
                    const bool axis = dx == 0.0 || dy == 0.0;
                    const double ar = axis ? (hx - lx) * (hy - ly) : ((ub - ua) * (vf - ve)) / (dx * dx + dy * dy);
                    if (!any || ar < area) {             // a strictly smaller area replaces the kept rectangle
                        any = true;
                        area = ar;
                        kept = ObbRect{ex, ey, dx, dy, ua, ub, ve, vf, axis};
                    }
                }
                if (last || !hb) break;
                ex = cx; ey = cy;
                dx = bx - cx; dy = by - cy;
                have = true;
                cx = bx; cy = by;
                ++steps;
                last = (cx == sx && cy == sy) || steps == m;   // one more pass, for this edge's extents only
            }
        }
    }
    if (empty) return SEG_EMPTY;
    if (!any || !(area > 0.0)) return OBB_FLAT;
    if (kept.axis) {
        c[0] = lx; c[1] = ly; c[2] = hx; c[3] = ly; c[4] = hx; c[5] = hy; c[6] = lx; c[7] = hy;
    } else {
        const double L = kept.dx * kept.dx + kept.dy * kept.dy;
        auto corner = [&](double u, double v, double &x, double &y) {
            x = kept.ex + (u * kept.dx - v * kept.dy) / L;
            y = kept.ey + (u * kept.dy + v * kept.dx) / L;
        };
        corner(kept.a, kept.e, c[0], c[1]);
        corner(kept.b, kept.e, c[2], c[3]);
        corner(kept.b, kept.f, c[4], c[5]);
        corner(kept.a, kept.f, c[6], c[7]);
    }
    bool out = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) out |= c[2 * k] < 0.0 || c[2 * k] > W || c[2 * k + 1] < 0.0 || c[2 * k + 1] > H;
    clamped = out ? 1 : 0;
    return clip ? SEG_CLIPPED : SEG_WRITTEN;
}

}  // namespace dyd
