// k20_tile.hip — K20: tiled YOLO label lines.
//
// Every image row is cut into a grid of overlapping tiles and every tile gets the label lines of the polygons that reach into
// it, as K13 would print them for the polygon moved to the tile's origin in an image of the tile's size (include/dyd.h has the
// rule; DESIGN §5r the mapping and its cost).  The polygon code is K13's: Poly / k13_prepare for the image-level action, Clip
// and ClipWalk per tile, k13_num8 for the numbers, k13_scan_inclusive for both offset arrays.
//
// Layout in HBM: xy = P x (x, y) f64, pt_off = B+1 int32, row_off = N+1 int32, cls = B int32, width / height = N f64.
// Outputs: row_status = N u8, tile_off = N+1 int64, tile_line_count = T int32, text_off = T+1 int64, action = B u8,
// tiles_written / tiles_cut / tiles_dropped = B int32, text.  Scratch: 40 bytes per polygon (bounding box, image-clipped area).
//
// Steps (no hand-off between workgroups inside a launch):
//   1. grid, a lane per row: status and tile count; a scan gives tile_off; the host reads T;
//   2. polygons, a lane per polygon: K13's action on the row's W and H, the bounding box and A_img;
//   3. measure, a lane per tile: the row's polygons in order, culled by the box, then translated, clipped and walked; the
//      tile's bytes and lines; the per-polygon counters by integer atomics;
//   4. a scan gives text_off; the host reads the text's size;
//   5. print, a workgroup per K20_WINDOW bytes of output aligned to 16 bytes of the text's address: a lane per tile that meets
//      the window walks the tile as step 3 does and prints the part inside the window into LDS, which streams out in 16-byte
//      stores.
// Steps 3 and 5 share one walk (k20_walk_tile), so a line's length and its bytes come from the same code.
#include "k13_poly.h"
#include "k13_scan.h"
#include "poly_table.h"
#include "round6.h"
#include "sized_out.h"
#include "text_window.h"

namespace dyd {

constexpr int K20_BLOCK = 256;
constexpr int K20_PRINT_BLOCK = 64;          // a wave per print window: the lanes are the window's tiles
constexpr int K20_WINDOW = 8 * 1024;         // bytes of text per print workgroup (multiple of 16)
constexpr int64_t K20_MAX_TILE = 1 << 20;    // tile size, step and max_tiles_per_row stay at or below it

struct TileParams {
    int64_t tile_w, tile_h, step_x, step_y, max_tiles;
    double min_vis;
    int mode;   // 0 segment, 1 detect
};

// one axis of the grid: the number of tiles
__device__ __forceinline__ int64_t k20_axis_count(int64_t L, int64_t T, int64_t S) { return L <= T ? 1 : (L - T + S - 1) / S + 1; }

// tile j of the axis -> origin; *extent = its length
__device__ __forceinline__ int64_t k20_axis_tile(int64_t L, int64_t T, int64_t S, int64_t j, int64_t *extent) {
    if (L <= T) {
        *extent = L;
        return 0;
    }
    *extent = T;
    return min(j * S, L - T);
}

// row status (0 tiled, 1 no_size, 2 fractional_size, 3 too_many_tiles) and, for status 0, the grid's columns and rows
__device__ __forceinline__ uint8_t k20_row_grid(double W, double H, const TileParams &tp, int64_t *nx, int64_t *ny) {
    *nx = *ny = 0;
    if (!k13_size_ok(W) || !k13_size_ok(H)) return 1;
    if (W != floor(W) || H != floor(H)) return 2;
    const int64_t cx = k20_axis_count((int64_t)W, tp.tile_w, tp.step_x), cy = k20_axis_count((int64_t)H, tp.tile_h, tp.step_y);
    if (cx > tp.max_tiles || cy > tp.max_tiles || cx * cy > tp.max_tiles) return 3;   // the product stays below 2^40
    *nx = cx;
    *ny = cy;
    return 0;
}

// ---- 1. grid: a lane per row -----------------------------------------------------------------------------------
__global__ __launch_bounds__(K20_BLOCK) void k20_grid_kernel(const double *__restrict__ width, const double *__restrict__ height,
                                                             int64_t n_rows, TileParams tp, uint8_t *__restrict__ row_status,
                                                             int64_t *__restrict__ tile_off) {
    const int64_t i = (int64_t)blockIdx.x * K20_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    int64_t nx, ny;
    row_status[i] = k20_row_grid(width[i], height[i], tp, &nx, &ny);
    tile_off[i + 1] = nx * ny;
    if (i == 0) tile_off[0] = 0;
}

// ---- 2. polygons: a lane per polygon ---------------------------------------------------------------------------
// action = K13's on the row's W and H (255: cls < 0); info[5p .. 5p+4] = x1, y1, x2, y2 of the points and A_img
__global__ __launch_bounds__(K20_BLOCK) void k20_poly_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                             const int32_t *__restrict__ row_off, const int32_t *__restrict__ cls,
                                                             const double *__restrict__ width, const double *__restrict__ height,
                                                             int64_t n_rows, int64_t n_polys, int64_t n_points,
                                                             uint8_t *__restrict__ action, double *__restrict__ info,
                                                             int32_t *__restrict__ written, int32_t *__restrict__ cut,
                                                             int32_t *__restrict__ dropped) {
    __shared__ int32_t rows[2];
    const int64_t p0 = (int64_t)blockIdx.x * K20_BLOCK, p1 = min(p0 + K20_BLOCK, n_polys);
    poly_tile_rows(row_off, n_rows, p0, p1, rows);
    const int64_t p = p0 + threadIdx.x;
    if (p >= p1) return;
    const int64_t r = last_le(row_off, rows[0], rows[1], p);
    const double W = width[r], H = height[r];
    uint8_t act;
    double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0, area = 0.0;
    if (cls[p] < 0) {
        act = SEG_UNSELECTED;
    } else if (!k13_size_ok(W) || !k13_size_ok(H)) {
        act = SEG_NO_SIZE;
    } else {
        const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
        Poly pg;
        act = k13_prepare(xy, a, b, pg);
        if (act == 0xff) {
            const bool clip = k13_outside(pg, W, H);
            ClipWalk w;
            auto count = [&](double x, double y) {
                w.add(x, y);
                return true;
            };
            k13_vertices(pg, clip, W, H, count);
            if (w.empty()) {
                act = SEG_EMPTY;
            } else {
                act = clip ? SEG_CLIPPED : SEG_WRITTEN;
                area = w.area();
                x1 = pg.x1; y1 = pg.y1; x2 = pg.x2; y2 = pg.y2;
            }
        }
    }
    action[p] = act;
    double *q = info + 5 * p;
    q[0] = x1; q[1] = y1; q[2] = x2; q[3] = y2; q[4] = area;
    written[p] = 0;
    cut[p] = 0;
    dropped[p] = 0;
}

// ---- the walk over one tile that measure and print share -------------------------------------------------------
// A polygon seen from a tile: Poly's vertex list with every vertex moved by (-ox, -oy).  The box fields are the moved box of
// the points (x - ox is monotone in x, so the moved minimum is the minimum of the moved points).
struct TilePoly {
    const double *p;
    int n;
    double ox, oy, x1, y1, x2, y2;
    template <class F>
    __device__ __forceinline__ void each(F &f) const {
        if (n == 2) {
            if (f(x1, y1) && f(x2, y1) && f(x2, y2)) f(x1, y2);
            return;
        }
        for (int k = 0; k < n; ++k) {
            const double2 v = *reinterpret_cast<const double2 *>(p + 2 * k);
            if (!f(v.x - ox, v.y - oy)) return;
        }
    }
};

struct Tile {
    int64_t p0, p1;          // the row's polygons
    double ox, oy, tw, th;
};

// tile g -> its row's polygons, origin and extent; false for a row without tiles (never for g < T of a sound tile_off)
__device__ __forceinline__ bool k20_tile(int64_t g, const int64_t *__restrict__ tile_off, const int32_t *__restrict__ row_off,
                                         const double *__restrict__ width, const double *__restrict__ height, int64_t n_rows,
                                         int64_t n_polys, const TileParams &tp, Tile &t) {
    const int64_t r = last_le(tile_off, 0, n_rows - 1, g);
    int64_t nx, ny;
    const double W = width[r], H = height[r];
    if (k20_row_grid(W, H, tp, &nx, &ny) != 0) return false;
    const int64_t local = g - tile_off[r];
    if (local < 0 || local >= nx * ny) return false;
    int64_t ew, eh;
    const int64_t ox = k20_axis_tile((int64_t)W, tp.tile_w, tp.step_x, local % nx, &ew);
    const int64_t oy = k20_axis_tile((int64_t)H, tp.tile_h, tp.step_y, local / nx, &eh);
    t.ox = (double)ox; t.oy = (double)oy; t.tw = (double)ew; t.th = (double)eh;
    t.p0 = max((int64_t)row_off[r], (int64_t)0);
    t.p1 = min((int64_t)row_off[r + 1], n_polys);
    return true;
}

// The tile's polygons in order.  on_pair(p, written, cut) for every polygon with a part in the tile; for a written one
// line(p, cid, tpoly, cut, walk) first, which returns false to end the walk.
template <class OnPair, class Line>
__device__ __forceinline__ void k20_walk_tile(const Tile &t, const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                              const int32_t *__restrict__ cls, const uint8_t *__restrict__ action,
                                              const double *__restrict__ info, int64_t n_points, double min_vis, OnPair &on_pair,
                                              Line &line) {
    for (int64_t p = t.p0; p < t.p1; ++p) {
        if (action[p] > SEG_CLIPPED) continue;
        const double *q = info + 5 * p;
        TilePoly tp;
        tp.ox = t.ox; tp.oy = t.oy;
        tp.x1 = q[0] - t.ox; tp.y1 = q[1] - t.oy; tp.x2 = q[2] - t.ox; tp.y2 = q[3] - t.oy;
        // the cull: every moved vertex fails the same clip pass, so the clip would give no vertex and the walk `empty`
        if (tp.x2 < 0.0 || tp.x1 > t.tw || tp.y2 < 0.0 || tp.y1 > t.th) continue;
        const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
        tp.p = xy + 2 * (int64_t)a;
        tp.n = b - a;
        const bool is_cut = k13_outside(tp, t.tw, t.th);
        ClipWalk w;
        auto count = [&](double x, double y) {
            w.add(x, y);
            return true;
        };
        k13_vertices(tp, is_cut, t.tw, t.th, count);
        if (w.empty()) continue;
        const bool wr = w.area() >= min_vis * q[4];
        if (wr && !line(p, cls[p], tp, is_cut, w)) return;
        on_pair(p, wr, is_cut);
    }
}

// ---- 3. measure: a lane per tile -------------------------------------------------------------------------------
__global__ __launch_bounds__(K20_BLOCK) void k20_measure_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                                const int32_t *__restrict__ row_off, const int32_t *__restrict__ cls,
                                                                const double *__restrict__ width, const double *__restrict__ height,
                                                                int64_t n_rows, int64_t n_polys, int64_t n_points, TileParams tp,
                                                                const int64_t *__restrict__ tile_off, int64_t n_tiles,
                                                                const uint8_t *__restrict__ action, const double *__restrict__ info,
                                                                int32_t *__restrict__ line_count, int64_t *__restrict__ text_off,
                                                                int32_t *__restrict__ written, int32_t *__restrict__ cut,
                                                                int32_t *__restrict__ dropped) {
    const int64_t g = (int64_t)blockIdx.x * K20_BLOCK + threadIdx.x;
    if (g >= n_tiles) return;
    int64_t bytes = 0;
    int32_t lines = 0;
    Tile t;
    if (k20_tile(g, tile_off, row_off, width, height, n_rows, n_polys, tp, t)) {
        auto line = [&](int64_t, int32_t cid, const TilePoly &, bool, const ClipWalk &w) {
            bytes += (lines ? 1 : 0) + k13_digits(cid) + (tp.mode ? 36 : 18 * (int64_t)w.m);
            ++lines;
            return true;
        };
        auto on_pair = [&](int64_t p, bool wr, bool is_cut) {
            if (wr) {
                atomicAdd(written + p, 1);
                if (is_cut) atomicAdd(cut + p, 1);
            } else {
                atomicAdd(dropped + p, 1);
            }
        };
        k20_walk_tile(t, xy, pt_off, cls, action, info, n_points, tp.min_vis, on_pair, line);
    }
    line_count[g] = lines;
    text_off[g + 1] = bytes;
    if (g == 0) text_off[0] = 0;
}

// ---- 5. print: a workgroup per window, a lane per tile ---------------------------------------------------------
__global__ __launch_bounds__(K20_PRINT_BLOCK) void k20_print_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                                    const int32_t *__restrict__ row_off, const int32_t *__restrict__ cls,
                                                                    const double *__restrict__ width, const double *__restrict__ height,
                                                                    int64_t n_rows, int64_t n_polys, int64_t n_points, TileParams tp,
                                                                    const int64_t *__restrict__ tile_off, int64_t n_tiles,
                                                                    const uint8_t *__restrict__ action, const double *__restrict__ info,
                                                                    const int64_t *__restrict__ text_off, int64_t total, int64_t phase,
                                                                    uint8_t *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint8_t img[K20_WINDOW];
    __shared__ int64_t range[2];
    const TextWindow win = text_window(img, blockIdx.x, K20_WINDOW, phase, total);
    const int64_t wlo = win.wlo, whi = win.whi;
    if (threadIdx.x < 2) range[threadIdx.x] = min(last_le(text_off, 0, n_tiles, threadIdx.x == 0 ? wlo : whi - 1), n_tiles - 1);
    __syncthreads();
    for (int64_t g = range[0] + threadIdx.x; g <= range[1]; g += K20_PRINT_BLOCK) {
        const int64_t end = text_off[g + 1];
        int64_t at = text_off[g];                  // the next line's first byte (its "\n" when it is not the tile's first)
        if (end <= wlo || at >= whi || at >= end) continue;
        Tile t;
        if (!k20_tile(g, tile_off, row_off, width, height, n_rows, n_polys, tp, t)) continue;
        bool first = true;
        auto line = [&](int64_t, int32_t cid, const TilePoly &pg, bool is_cut, const ClipWalk &w) {
            if (at >= whi) return false;
            const int cd = k13_digits(cid);
            const int64_t len = (first ? 0 : 1) + cd + (tp.mode ? 36 : 18 * (int64_t)w.m);
            if (at + len > wlo) {
                int64_t a = at;
                if (!first) win.put(a++, '\n');
                win.class_id(a, cid, cd);
                a += cd;
                if (tp.mode) {
                    win.field(a, (w.lx + w.hx) / 2.0 / t.tw);
                    win.field(a + 9, (w.ly + w.hy) / 2.0 / t.th);
                    win.field(a + 18, (w.hx - w.lx) / t.tw);
                    win.field(a + 27, (w.hy - w.ly) / t.th);
                } else {
                    auto print = [&](double x, double y) {
                        if (a >= whi) return false;
                        if (a + 18 > wlo) {
                            win.field(a, x / t.tw);
                            win.field(a + 9, y / t.th);
                        }
                        a += 18;
                        return true;
                    };
                    k13_vertices(pg, is_cut, t.tw, t.th, print);
                }
            }
            at += len;
            first = false;
            return at < end;
        };
        auto on_pair = [](int64_t, bool, bool) {};
        k20_walk_tile(t, xy, pt_off, cls, action, info, n_points, tp.min_vis, on_pair, line);
    }
    __syncthreads();
    win.flush<K20_WINDOW, K20_PRINT_BLOCK>(text);
}

struct TileOut {
    uint8_t *row_status;
    int64_t *tile_off;
    int32_t *line_count;
    int64_t *text_off;
    uint8_t *action;
    int32_t *written, *cut, *dropped;
};

static int tile_params(int64_t tile_w, int64_t tile_h, int64_t step_x, int64_t step_y, double min_vis, int32_t mode,
                       int64_t max_tiles, TileParams *tp) {
    DYD_REQUIRE(step_x >= 1 && step_x <= tile_w && tile_w <= K20_MAX_TILE, "need 1 <= step_x <= tile_w <= 2^20");
    DYD_REQUIRE(step_y >= 1 && step_y <= tile_h && tile_h <= K20_MAX_TILE, "need 1 <= step_y <= tile_h <= 2^20");
    DYD_REQUIRE(min_vis >= 0.0 && min_vis <= 1.0, "min_visibility must lie in [0, 1]");   // false for NaN
    DYD_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (segment) or 1 (detect)");
    DYD_REQUIRE(max_tiles >= 1 && max_tiles <= K20_MAX_TILE, "max_tiles_per_row must lie in 1..2^20");
    *tp = TileParams{tile_w, tile_h, step_x, step_y, max_tiles, min_vis, mode};
    return DYD_OK;
}

constexpr SizedName K20_TEXT{"K20", "text", "bytes", 1};

// Steps 1 to 5 on device pointers.  `text` is asked for the buffer once the size is known (none: measure only).
// *n_tiles_out and *total_out are host values.
static int tile_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                       const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, const TileParams &tp,
                       int64_t tiles_cap, const TileOut &o, int64_t *n_tiles_out, int64_t *total_out, SizedOut &text, hipStream_t st) {
    // 1. the grid
    const size_t info_bytes = 40 * (size_t)max(n_polys, (int64_t)1);
    const int64_t row_parts = k13_scan_parts(n_rows);
    ScratchLease lease(st);
    void *scr = nullptr;
    int rc = lease.get(info_bytes + 8 * (size_t)row_parts, &scr);
    if (rc) return rc;
    double *info = static_cast<double *>(scr);
    hipLaunchKernelGGL(k20_grid_kernel, dim3((unsigned)ceil_div(n_rows, (int64_t)K20_BLOCK)), dim3(K20_BLOCK), 0, st, width, height,
                       n_rows, tp, o.row_status, o.tile_off);
    k13_scan_inclusive(o.tile_off + 1, n_rows, reinterpret_cast<int64_t *>(info + info_bytes / 8), st);
    // 2. the polygons (the scan's scratch lies behind info, so both may be in flight)
    if (n_polys > 0)
        hipLaunchKernelGGL(k20_poly_kernel, dim3((unsigned)ceil_div(n_polys, (int64_t)K20_BLOCK)), dim3(K20_BLOCK), 0, st, xy, pt_off,
                           row_off, cls, width, height, n_rows, n_polys, n_points, o.action, info, o.written, o.cut, o.dropped);
    int64_t n_tiles = 0, total = 0;
    if ((rc = read_totals("K20", "the grid step", {{&n_tiles, o.tile_off + n_rows}}, st))) return rc;
    *n_tiles_out = n_tiles;
    *total_out = 0;
    if (n_tiles > INT32_MAX) {
        set_error("K20: %lld tiles, more than 2^31 - 1", (long long)n_tiles);
        return DYD_ERR_RANGE;
    }
    if (n_tiles > tiles_cap) {
        set_error("K20: tile arrays too small (%lld tiles, room for %lld)", (long long)n_tiles, (long long)tiles_cap);
        return DYD_ERR_RANGE;
    }
    if (n_tiles == 0) {
        DYD_HIP(hipMemsetAsync(o.text_off, 0, 8, st));
        return DYD_OK;
    }
    // 3. and 4. measure, offsets
    DevBuf d_part;
    if ((rc = d_part.alloc(8 * (size_t)k13_scan_parts(n_tiles), st))) return rc;
    hipLaunchKernelGGL(k20_measure_kernel, dim3((unsigned)ceil_div(n_tiles, (int64_t)K20_BLOCK)), dim3(K20_BLOCK), 0, st, xy, pt_off,
                       row_off, cls, width, height, n_rows, n_polys, n_points, tp, o.tile_off, n_tiles, o.action, info, o.line_count,
                       o.text_off, o.written, o.cut, o.dropped);
    k13_scan_inclusive(o.text_off + 1, n_tiles, d_part.as<int64_t>(), st);
    if ((rc = read_totals("K20", "the measure step", {{&total, o.text_off + n_tiles}}, st))) return rc;
    *total_out = total;
    if (total == 0 || (rc = text.get(total)) || !text.p) return rc;
    // 5. print
    const TextWindows tw = text_windows(text.p, total, K20_WINDOW);
    hipLaunchKernelGGL(k20_print_kernel, dim3((unsigned)tw.count), dim3(K20_PRINT_BLOCK), 0, st, xy, pt_off, row_off, cls, width,
                       height, n_rows, n_polys, n_points, tp, o.tile_off, n_tiles, o.action, info, o.text_off, total, tw.phase,
                       text.as<uint8_t>());
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_yolo_tile_lines_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                            const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int64_t tile_w, int64_t tile_h,
                            int64_t step_x, int64_t step_y, double min_visibility, int32_t mode, int64_t max_tiles_per_row,
                            int64_t tiles_cap, uint8_t *out_row_status, int64_t *out_tile_off, int32_t *out_tile_line_count,
                            int64_t *out_text_off, uint8_t *out_action, int32_t *out_tiles_written, int32_t *out_tiles_cut,
                            int32_t *out_tiles_dropped, int64_t *out_n_tiles, uint8_t *out_text_or_null, int64_t text_cap,
                            int64_t *out_total, void *stream) {
    DYD_API_ENTER();
    TileParams tp;
    int rc = tile_params(tile_w, tile_h, step_x, step_y, min_visibility, mode, max_tiles_per_row, &tp);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && text_cap >= 0 && tiles_cap >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31) && n_rows < (1LL << 31) && tiles_cap < (1LL << 31),
                "size too large");   // 1-D grids of K20_BLOCK lanes over rows, polygons and tiles
    DYD_REQUIRE(out_tile_off && out_text_off && out_n_tiles && out_total, "null pointer");
    hipStream_t st = pick_stream(stream);
    if (n_rows == 0) {
        DYD_HIP(hipMemsetAsync(out_tile_off, 0, 8, st));
        DYD_HIP(hipMemsetAsync(out_text_off, 0, 8, st));
        *out_n_tiles = 0;
        *out_total = 0;
        return DYD_OK;
    }
    DYD_REQUIRE(row_off && width && height && out_row_status, "null pointer");
    DYD_REQUIRE(tiles_cap == 0 || out_tile_line_count, "null pointer");
    DYD_REQUIRE(n_polys == 0 || (pt_off && cls && out_action && out_tiles_written && out_tiles_cut && out_tiles_dropped), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    const TileOut o{out_row_status, out_tile_off, out_tile_line_count, out_text_off, out_action, out_tiles_written, out_tiles_cut,
                    out_tiles_dropped};
    SizedOut text(K20_TEXT, out_text_or_null, text_cap);
    return tile_launch(xy, pt_off, row_off, cls, width, height, n_rows, n_polys, n_points, tp, tiles_cap, o, out_n_tiles, out_total,
                       text, st);
}

int dyd_yolo_tile_lines(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cls, const double *width,
                        const double *height, int64_t n_rows, int64_t tile_w, int64_t tile_h, int64_t step_x, int64_t step_y,
                        double min_visibility, int32_t mode, int64_t max_tiles_per_row, int64_t tiles_cap, uint8_t *out_row_status,
                        int64_t *out_tile_off, int32_t *out_tile_line_count, int64_t *out_text_off, uint8_t *out_action,
                        int32_t *out_tiles_written, int32_t *out_tiles_cut, int32_t *out_tiles_dropped, int64_t *out_n_tiles,
                        uint8_t **out_text, int64_t *out_text_len) {
    DYD_API_ENTER();
    TileParams tp;
    int rc = tile_params(tile_w, tile_h, step_x, step_y, min_visibility, mode, max_tiles_per_row, &tp);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0 && tiles_cap >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31) && tiles_cap < (1LL << 31), "size too large");
    DYD_REQUIRE(out_tile_off && out_text_off && out_n_tiles && out_text && out_text_len, "null pointer");
    DYD_REQUIRE(tiles_cap == 0 || out_tile_line_count, "null pointer");
    *out_text = nullptr;
    *out_text_len = 0;
    *out_n_tiles = 0;
    out_tile_off[0] = 0;
    out_text_off[0] = 0;
    if (n_rows == 0) return DYD_OK;
    int64_t n_polys = 0, n_points = 0;
    rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, out_row_status != nullptr,
                          cls && out_action && out_tiles_written && out_tiles_cut && out_tiles_dropped, nullptr, 0, &n_polys, &n_points);
    if (rc) return rc;
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_cls, d_status, d_toff, d_lines, d_xoff, d_act, d_wr, d_cut, d_drop;
    const size_t nb4 = 4 * (size_t)n_polys;
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, n_polys, n_points)) || (rc = poly_column(d_cls, cls, nb4)) ||
        (rc = d_status.alloc((size_t)n_rows)) || (rc = d_toff.alloc(8 * (size_t)(n_rows + 1))) ||
        (rc = d_lines.alloc(4 * (size_t)tiles_cap)) || (rc = d_xoff.alloc(8 * (size_t)(tiles_cap + 1))) ||
        (rc = d_act.alloc((size_t)n_polys)) || (rc = d_wr.alloc(nb4)) || (rc = d_cut.alloc(nb4)) || (rc = d_drop.alloc(nb4)))
        return rc;
    const TileOut o{d_status.as<uint8_t>(), d_toff.as<int64_t>(), d_lines.as<int32_t>(), d_xoff.as<int64_t>(), d_act.as<uint8_t>(),
                    d_wr.as<int32_t>(), d_cut.as<int32_t>(), d_drop.as<int32_t>()};
    SizedOut text(K20_TEXT, st);
    int64_t n_tiles = 0, total = 0;
    KernelTimer timer(st);
    rc = tile_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), d_cls.as<int32_t>(), t.w.as<double>(),
                     t.h.as<double>(), n_rows, n_polys, n_points, tp, tiles_cap, o, &n_tiles, &total, text, st);
    *out_n_tiles = n_tiles;
    if (rc == DYD_ERR_RANGE && n_tiles > tiles_cap && n_tiles <= INT32_MAX) {   // the caller sizes its arrays from these and calls again
        DYD_HIP(hipMemcpyAsync(out_row_status, d_status.p, (size_t)n_rows, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_tile_off, d_toff.p, 8 * (size_t)(n_rows + 1), hipMemcpyDeviceToHost, st));
        DYD_HIP(hipStreamSynchronize(st));
    }
    if (rc) return rc;
    timer.finish();
    return hand_back_text(text.p, total,
                          {{out_row_status, d_status.p, (size_t)n_rows}, {out_tile_off, d_toff.p, 8 * (size_t)(n_rows + 1)},
                           {out_tile_line_count, d_lines.p, 4 * (size_t)n_tiles}, {out_text_off, d_xoff.p, 8 * (size_t)(n_tiles + 1)},
                           {out_action, d_act.p, (size_t)n_polys}, {out_tiles_written, d_wr.p, nb4}, {out_tiles_cut, d_cut.p, nb4},
                           {out_tiles_dropped, d_drop.p, nb4}},
                          st, out_text, out_text_len);
}

}  // extern "C"
