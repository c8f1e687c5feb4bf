// k14_poly_audit.hip — K14: per-class polygon statistics and defects of an annotation table (the polygon audit step).
//
// For every polygon with a class: the category K13 would give it (k13_poly.h's checks and clip, the same code), and for the
// written and clipped ones three defect bits and the clipped area (include/dyd.h and DESIGN §5m have the definition):
//   duplicate_vertices  len(V) >= 3 and some V[k] == V[k-1], cyclically;
//   self_intersecting   len(V) >= 3; U = V without cyclically consecutive duplicates, m = len(U) >= 3, and an adjacent edge pair
//                       doubles back (o(a,b,c) == 0 and (b-a).(c-b) < 0) or two non-adjacent edges of U share a point;
//   tiny_area           |shoelace sum over the clipped vertices| * 0.5 < min_area.
// Every test is IEEE f64 without contraction, in the order the definition writes it.  The edges of U are the edges
// e_k = (V[k-1], V[k]) (k - 1 cyclic) whose ends differ, in V's order: two of them are adjacent when no such edge lies between
// them, or when they are the first and the last.  So the tests walk V itself and need no copy of U.
//
// Layout in HBM: xy = P x (x, y) f64 (16-B aligned), pt_off = B+1 int32, row_off = N+1 int32, cls = B int32 (-1: the name is no
// str, the polygon is only counted by the host), width / height = N f64, size_status = N u8 (0 ok, 1 missing, 2 invalid).
// Out: category = B u8 (255 for cls -1), defects = B u8, area = B f64 (NaN unless written or clipped), class_counts = C x 14 u64,
// hist = C x 11 u64 (vertex counts).
//
// Mapping.
//   1. k14_poly_kernel, a lane per polygon over 256-polygon tiles of a persistent grid: two lanes find the tile's first and last
//      row by a binary search over row_off, every lane then searches only between them.  One streaming pass over V gives the
//      checks (k13_prepare), then one over the clipped vertices (k13_vertices) the category and the shoelace sum with O(1)
//      state, then one over V the duplicate test, the fold-back test and the first and last edge of U.  A polygon with at most
//      K14_LANE_EDGES edges of U runs the O(m^2) edge-pair test in its lane (vertices from L1 / L2), stopping at the first hit;
//      a larger one goes to a work list (the threshold: DESIGN §5m; dyd_set_option "k14_lane_edges" moves it for A/B runs).
//      Class counters and the vertex histogram: LDS copies of the block, one u64 global atomic per non-zero counter at the end
//      (K10's scheme), global atomics when C > K14_LDS_CLASSES.
//   2. k14_wave_kernel, a wave per listed polygon: lane L takes the edges e_k with k = L (mod 64) against every later edge, and
//      the wave stops by ballot after each round of 64 edges once a lane has a hit.  The cost is O(m^2 / 64) per polygon: no
//      sweep (O(m log m)) here, see DESIGN §5m.
// No kernel indexes a per-lane array at run time: no scratch.
#include "k13_poly.h"
#include "poly_table.h"

namespace dyd {

constexpr int K14_BLOCK = 256;
constexpr int K14_LANE_EDGES = 64;          // edges of U up to which a lane runs the pair test itself (default)
constexpr int K14_CLSC = 14;                // polygons, images, 6 categories (K13's codes), 3 defects, 3 area buckets
constexpr int K14_HIST = 11;                // vertex counts <= 2, 3, 4, 8, 16, 32, 64, 128, 256, 1024, the rest
constexpr int K14_LDS_CLASSES = 128;
constexpr int K14_CAT_COL = 2, K14_DEF_COL = 8, K14_AREA_COL = 11;

enum : uint8_t { K14_DUP = 1, K14_SELFX = 2, K14_TINY = 4, K14_UNMATCHABLE = 255 };

struct K14Shared {
    uint32_t cnt[K14_LDS_CLASSES * (K14_CLSC + K14_HIST)];
    int32_t rows[2];
};

__device__ __forceinline__ double k14_o(double px, double py, double qx, double qy, double rx, double ry) {
    return (qx - px) * (ry - py) - (qy - py) * (rx - px);
}

__device__ __forceinline__ bool k14_on(double px, double py, double qx, double qy, double rx, double ry) {
    return fmin(px, qx) <= rx && rx <= fmax(px, qx) && fmin(py, qy) <= ry && ry <= fmax(py, qy);
}

// segments (a, b) and (c, d) share a point: a proper crossing by strict signs, or a collinear end inside the other's box
__device__ __forceinline__ bool k14_meet(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
    const double d1 = k14_o(cx, cy, dx, dy, ax, ay), d2 = k14_o(cx, cy, dx, dy, bx, by);
    const double d3 = k14_o(ax, ay, bx, by, cx, cy), d4 = k14_o(ax, ay, bx, by, dx, dy);
    if (((d1 > 0.0 && d2 < 0.0) || (d1 < 0.0 && d2 > 0.0)) && ((d3 > 0.0 && d4 < 0.0) || (d3 < 0.0 && d4 > 0.0))) return true;
    return (d1 == 0.0 && k14_on(cx, cy, dx, dy, ax, ay)) || (d2 == 0.0 && k14_on(cx, cy, dx, dy, bx, by)) ||
           (d3 == 0.0 && k14_on(ax, ay, bx, by, cx, cy)) || (d4 == 0.0 && k14_on(ax, ay, bx, by, dx, dy));
}

// the edges (a, b), (b, c) double back on each other
__device__ __forceinline__ bool k14_fold(double ax, double ay, double bx, double by, double cx, double cy) {
    return k14_o(ax, ay, bx, by, cx, cy) == 0.0 && (bx - ax) * (cx - bx) + (by - ay) * (cy - by) < 0.0;
}

__device__ __forceinline__ double2 k14_v(const double *p, int k) { return *reinterpret_cast<const double2 *>(p + 2 * k); }

// edge e_k = (a, b) of U against every later edge of U but its neighbours; first / last: the first and last k of an edge of U
__device__ __forceinline__ bool k14_edge_hits(const double *p, int n, int k, double ax, double ay, double bx, double by, int first,
                                              int last) {
    bool adjacent = true;                      // the next edge of U is e_k's neighbour
    double cx = bx, cy = by;
    for (int j = k + 1; j < n; ++j) {
        const double2 d = k14_v(p, j);
        if (d.x != cx || d.y != cy) {
            if (adjacent) adjacent = false;
            else if (!(k == first && j == last) && k14_meet(ax, ay, bx, by, cx, cy, d.x, d.y)) return true;
        }
        cx = d.x;
        cy = d.y;
    }
    return false;
}

__device__ __forceinline__ int k14_hist_bin(int n) {
    if (n <= 4) return n <= 2 ? 0 : n - 2;
    int b = 3;
    for (int e = 8; e <= 256 && n > e; e <<= 1) ++b;   // 8 -> 3 ... 256 -> 8
    if (n <= 256) return b;
    return n <= 1024 ? 9 : 10;
}

__device__ __forceinline__ void k14_add(uint32_t *lds, uint64_t *glob, bool use_lds, int64_t at) {
    if (use_lds) atomicAdd(lds + at, 1u);
    else atomicAdd(reinterpret_cast<unsigned long long *>(glob + at), 1ull);
}

__global__ __launch_bounds__(K14_BLOCK) void k14_poly_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                             const int32_t *__restrict__ row_off, const int32_t *__restrict__ cls,
                                                             const double *__restrict__ width, const double *__restrict__ height,
                                                             const uint8_t *__restrict__ size_status, int64_t n_rows,
                                                             int64_t n_polys, int64_t n_points, int32_t n_classes, double min_area,
                                                             int32_t lane_edges,
                                                             uint8_t *__restrict__ out_cat, uint8_t *__restrict__ out_def,
                                                             double *__restrict__ out_area, uint64_t *__restrict__ out_cls,
                                                             uint64_t *__restrict__ out_hist, int32_t *__restrict__ work,
                                                             uint32_t *__restrict__ n_work) {
    __shared__ K14Shared S;
    const bool lds = n_classes <= K14_LDS_CLASSES;
    const int ncnt = K14_CLSC + K14_HIST;
    if (lds)
        for (int k = threadIdx.x; k < n_classes * ncnt; k += K14_BLOCK) S.cnt[k] = 0u;
    const int64_t n_tiles = (n_polys + K14_BLOCK - 1) / K14_BLOCK;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t p0 = t * K14_BLOCK;
        __syncthreads();                       // the previous tile's lanes are done with S.rows (and the zeroing is visible)
        poly_tile_rows(row_off, n_rows, p0, min(p0 + K14_BLOCK, n_polys), S.rows);
        const int64_t p = p0 + threadIdx.x;
        if (p >= n_polys) continue;
        const int32_t c = cls[p];
        if (c < 0 || c >= n_classes) {
            out_cat[p] = K14_UNMATCHABLE;
            out_def[p] = 0;
            out_area[p] = __builtin_nan("");
            continue;
        }
        const int64_t r = last_le(row_off, S.rows[0], S.rows[1], p);
        const double W = width[r], H = height[r];
        const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);   // as K13
        uint8_t cat, def = 0;
        double area = __builtin_nan("");
        Poly pg;
        pg.p = xy + 2 * (int64_t)a;
        pg.n = b - a;
        if (size_status[r] != 0 || !k13_size_ok(W) || !k13_size_ok(H)) {
            cat = SEG_NO_SIZE;
        } else {
            cat = k13_prepare(xy, a, b, pg);
            if (cat == 0xff) {
                const bool clip = k13_outside(pg, W, H);
                // k13_poly.h's ClipWalk, written out: through the struct this kernel takes 105 VGPRs, not 103
                int m = 0;
                double lx = 0.0, ly = 0.0, hx = 0.0, hy = 0.0, fx = 0.0, fy = 0.0, px = 0.0, py = 0.0, s = 0.0;
                auto walk = [&](double x, double y) {
                    if (m == 0) { lx = hx = fx = x; ly = hy = fy = y; }
                    else s += px * y - x * py;
                    lx = fmin(lx, x); hx = fmax(hx, x);
                    ly = fmin(ly, y); hy = fmax(hy, y);
                    px = x; py = y;
                    ++m;
                    return true;
                };
                k13_vertices(pg, clip, W, H, walk);
                if (m < 3 || !(hx - lx > 0.0) || !(hy - ly > 0.0)) {
                    cat = SEG_EMPTY;
                } else {
                    cat = clip ? SEG_CLIPPED : SEG_WRITTEN;
                    s += px * fy - fx * py;
                    area = fabs(s) * 0.5;
                    if (area < min_area) def |= K14_TINY;
                }
            }
        }
        const int n = pg.n;
        if (cat <= SEG_CLIPPED && n >= 3) {
            // duplicates, fold-backs and the first / last edge of U in one pass over V
            const double2 vl = k14_v(pg.p, n - 1);
            double qx = vl.x, qy = vl.y;        // V[k - 1]
            double u0x = 0, u0y = 0, u1x = 0, u1y = 0, ax = 0, ay = 0, bx = 0, by = 0;
            int m = 0, first = -1, last = -1;
            bool fold = false;
            for (int k = 0; k < n; ++k) {
                const double2 v = k14_v(pg.p, k);
                if (v.x != qx || v.y != qy) {
                    if (m == 0) { u0x = v.x; u0y = v.y; first = k; }
                    else if (m == 1) { u1x = v.x; u1y = v.y; }
                    if (m >= 2) fold |= k14_fold(ax, ay, bx, by, v.x, v.y);
                    ax = bx; ay = by; bx = v.x; by = v.y;
                    last = k;
                    ++m;
                }
                qx = v.x;
                qy = v.y;
            }
            if (m < n) def |= K14_DUP;
            if (m >= 3) {
                fold = fold || k14_fold(ax, ay, bx, by, u0x, u0y) || k14_fold(bx, by, u0x, u0y, u1x, u1y);
                if (fold) {
                    def |= K14_SELFX;
                } else if (m <= lane_edges) {
                    double cx = vl.x, cy = vl.y;
                    for (int k = 0; k < n; ++k) {
                        const double2 v = k14_v(pg.p, k);
                        if ((v.x != cx || v.y != cy) && k14_edge_hits(pg.p, n, k, cx, cy, v.x, v.y, first, last)) {
                            def |= K14_SELFX;
                            break;
                        }
                        cx = v.x;
                        cy = v.y;
                    }
                } else {
                    work[atomicAdd(n_work, 1u)] = (int32_t)p;
                }
            }
        }
        out_cat[p] = cat;
        out_def[p] = def;
        out_area[p] = area;
        // class counters: "images" when no earlier polygon of the row has the class
        bool first_in_row = true;
        for (int64_t q = p - 1; q >= max(row_off[r], 0); --q)
            if (cls[q] == c) { first_in_row = false; break; }
        uint32_t *lc = S.cnt + (int64_t)c * ncnt;
        uint64_t *gc = out_cls + (int64_t)c * K14_CLSC, *gh = out_hist + (int64_t)c * K14_HIST;
        k14_add(lc, gc, lds, 0);
        if (first_in_row) k14_add(lc, gc, lds, 1);
        k14_add(lc, gc, lds, K14_CAT_COL + cat);
        if (def & K14_DUP) k14_add(lc, gc, lds, K14_DEF_COL + 0);
        if (def & K14_SELFX) k14_add(lc, gc, lds, K14_DEF_COL + 1);
        if (def & K14_TINY) k14_add(lc, gc, lds, K14_DEF_COL + 2);
        if (cat <= SEG_CLIPPED) k14_add(lc, gc, lds, K14_AREA_COL + (area < 1024.0 ? 0 : (area < 9216.0 ? 1 : 2)));
        if (lds) atomicAdd(lc + K14_CLSC + k14_hist_bin(n), 1u);
        else atomicAdd(reinterpret_cast<unsigned long long *>(gh + k14_hist_bin(n)), 1ull);
    }
    if (!lds) return;
    __syncthreads();
    for (int k = threadIdx.x; k < n_classes * ncnt; k += K14_BLOCK) {
        const uint32_t v = S.cnt[k];
        if (!v) continue;
        const int cc = k / ncnt, j = k - cc * ncnt;
        uint64_t *dst = j < K14_CLSC ? out_cls + (int64_t)cc * K14_CLSC + j : out_hist + (int64_t)cc * K14_HIST + (j - K14_CLSC);
        atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
    }
}

// ---- 2. the wave tier: a wave per listed polygon ------------------------------------------------------------------
__global__ __launch_bounds__(K14_BLOCK) void k14_wave_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                             const int32_t *__restrict__ cls, int64_t n_points,
                                                             const int32_t *__restrict__ work, const uint32_t *__restrict__ n_work,
                                                             uint8_t *__restrict__ out_def,
                                                             uint64_t *__restrict__ out_cls) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * (K14_BLOCK / kWave);
    const int64_t total = *n_work;
    for (int64_t w = (int64_t)blockIdx.x * (K14_BLOCK / kWave) + threadIdx.x / kWave; w < total; w += waves) {
        const int32_t p = work[w];
        const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
        const double *v = xy + 2 * (int64_t)a;
        const int n = b - a;
        int first = -1, last = -1;
        for (int base = 0; base < n; base += kWave) {
            const int k = base + lane;
            bool kept = false;
            if (k < n) {
                const double2 q = k14_v(v, k == 0 ? n - 1 : k - 1), c = k14_v(v, k);
                kept = q.x != c.x || q.y != c.y;
            }
            const uint64_t mask = __ballot(kept);
            if (mask) {
                if (first < 0) first = base + __ffsll((long long)mask) - 1;
                last = base + 63 - __clzll((long long)mask);
            }
        }
        bool hit = false;
        for (int base = 0; base < n; base += kWave) {
            const int k = base + lane;
            if (k < n) {
                const double2 q = k14_v(v, k == 0 ? n - 1 : k - 1), c = k14_v(v, k);
                if ((q.x != c.x || q.y != c.y) && k14_edge_hits(v, n, k, q.x, q.y, c.x, c.y, first, last)) hit = true;
            }
            if (__ballot(hit)) {
                hit = true;
                break;
            }
        }
        if (hit && lane == 0) {
            out_def[p] |= K14_SELFX;
            atomicAdd(reinterpret_cast<unsigned long long *>(out_cls + (int64_t)cls[p] * K14_CLSC + K14_DEF_COL + 1), 1ull);
        }
    }
}

// dyd_set_option("k14_lane_edges", m): the largest U a lane tests itself; <= 0 restores K14_LANE_EDGES
static int g_k14_lane_edges = K14_LANE_EDGES;

void set_k14_lane_edges(int v) { g_k14_lane_edges = v > 0 ? v : K14_LANE_EDGES; }

static int k14_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                      const double *height, const uint8_t *size_status, int64_t n_rows, int64_t n_polys, int32_t n_classes,
                      int64_t n_points, double min_area, uint8_t *out_cat, uint8_t *out_def, double *out_area, int64_t *out_cls,
                      int64_t *out_hist, hipStream_t st) {
    if (n_classes > 0) {
        DYD_HIP(hipMemsetAsync(out_cls, 0, 8 * (size_t)n_classes * K14_CLSC, st));
        DYD_HIP(hipMemsetAsync(out_hist, 0, 8 * (size_t)n_classes * K14_HIST, st));
    }
    if (n_rows == 0 || n_polys == 0) return DYD_OK;
    DevBuf d_work;
    int rc;
    if ((rc = d_work.alloc(4 * (size_t)n_polys + 16, st))) return rc;
    uint32_t *n_work = reinterpret_cast<uint32_t *>(d_work.as<int32_t>() + n_polys);
    DYD_HIP(hipMemsetAsync(n_work, 0, 4, st));
    const int64_t tiles = ceil_div(n_polys, (int64_t)K14_BLOCK);
    const int64_t want = (int64_t)ctx().num_cu * 8;
    const unsigned blocks = (unsigned)(tiles < want ? tiles : want);
    hipLaunchKernelGGL(k14_poly_kernel, dim3(blocks), dim3(K14_BLOCK), 0, st, xy, pt_off, row_off, cls, width, height, size_status,
                       n_rows, n_polys, n_points, n_classes, min_area, g_k14_lane_edges, out_cat, out_def, out_area,
                       reinterpret_cast<uint64_t *>(out_cls), reinterpret_cast<uint64_t *>(out_hist), d_work.as<int32_t>(), n_work);
    hipLaunchKernelGGL(k14_wave_kernel, dim3((unsigned)ctx().num_cu * 2), dim3(K14_BLOCK), 0, st, xy, pt_off, cls, n_points,
                       d_work.as<int32_t>(), n_work, out_def, reinterpret_cast<uint64_t *>(out_cls));
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_audit_polygons_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                           const double *height, const uint8_t *size_status, int64_t n_rows, int64_t n_polys, int64_t n_points,
                           int32_t n_classes, double min_area, uint8_t *out_category, uint8_t *out_defects, double *out_area,
                           int64_t *out_class_counts, int64_t *out_hist_vertices, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && n_classes >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31), "n_polys or n_points exceeds int32 offsets");
    DYD_REQUIRE(std::isfinite(min_area) && min_area >= 0.0, "min_area must be finite and >= 0");
    DYD_REQUIRE(n_classes == 0 || (out_class_counts && out_hist_vertices), "null pointer");
    DYD_REQUIRE(n_rows == 0 || (row_off && width && height && size_status), "null pointer");
    DYD_REQUIRE(n_polys == 0 || (pt_off && cls && out_category && out_defects && out_area), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(xy) & 15) == 0, "xy must be 16-byte aligned");
    return k14_launch(xy, pt_off, row_off, cls, width, height, size_status, n_rows, n_polys, n_classes, n_points, min_area, out_category,
                      out_defects, out_area, out_class_counts, out_hist_vertices, pick_stream(stream));
}

int dyd_audit_polygons(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                       const double *height, const uint8_t *size_status, int64_t n_rows, int32_t n_classes, double min_area,
                       uint8_t *out_category, uint8_t *out_defects, double *out_area, int64_t *out_class_counts,
                       int64_t *out_hist_vertices) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_classes >= 0, "negative size");
    DYD_REQUIRE(std::isfinite(min_area) && min_area >= 0.0, "min_area must be finite and >= 0");
    DYD_REQUIRE(n_classes == 0 || (out_class_counts && out_hist_vertices), "null pointer");
    int64_t nb = 0, np = 0;
    int rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, size_status,
                              cls && out_category && out_defects && out_area, cls, n_classes, &nb, &np);
    if (rc) return rc;
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_cls, d_st, d_cat, d_def, d_area, d_cc, d_hist;
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, nb, np)) || (rc = poly_column(d_cls, cls, 4 * (size_t)nb)) ||
        (rc = poly_column(d_st, size_status, (size_t)n_rows)) || (rc = d_cat.alloc((size_t)nb)) || (rc = d_def.alloc((size_t)nb)) ||
        (rc = d_area.alloc(8 * (size_t)nb)) || (rc = d_cc.alloc(8 * K14_CLSC * (size_t)n_classes)) ||
        (rc = d_hist.alloc(8 * K14_HIST * (size_t)n_classes)))
        return rc;
    KernelTimer timer(st);
    rc = k14_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), d_cls.as<int32_t>(), t.w.as<double>(), t.h.as<double>(),
                    d_st.as<uint8_t>(), n_rows, nb, n_classes, np, min_area, d_cat.as<uint8_t>(), d_def.as<uint8_t>(),
                    d_area.as<double>(), d_cc.as<int64_t>(), d_hist.as<int64_t>(), st);
    if (rc) return rc;
    timer.finish();
    if (nb) {
        DYD_HIP(hipMemcpyAsync(out_category, d_cat.p, (size_t)nb, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_defects, d_def.p, (size_t)nb, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_area, d_area.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    if (n_classes) {
        DYD_HIP(hipMemcpyAsync(out_class_counts, d_cc.p, 8 * K14_CLSC * (size_t)n_classes, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_hist_vertices, d_hist.p, 8 * K14_HIST * (size_t)n_classes, hipMemcpyDeviceToHost, st));
    }
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
