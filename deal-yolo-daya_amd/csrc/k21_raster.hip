// k21_raster.hip — K21: label masks, the annotation polygons of every image row scan-converted into one byte per pixel.
//
// A pixel is covered by a polygon when an odd number of the polygon's edges cross the pixel's scanline to the right of the
// pixel's centre (include/dyd.h has the rule, DESIGN §5s the mapping and its cost); it holds the value of the last polygon of
// its row that covers it, or the background.  The polygon code is K13's: k13_size_ok for the sizes, Poly / k13_prepare for the
// action and the box of a two-point polygon, k13_scan_inclusive for both offset arrays, last_le for the row search.  The pixel
// rule itself is k21_cover.h, shared with K22 (k22_poly_compare.hip): the row rule, the polygons of a row, the box cull and the
// edge step; the polygon kernel below also serves K22 through k21_polys.  This file keeps what a mask needs beyond coverage:
// the owner per pixel, the covered / owned counters and the byte stream-out.
//
// Layout in HBM: xy = P x (x, y) f64, pt_off = B+1 int32, row_off = N+1 int32, val = B int32, width / height = N f64.
// Outputs: row_status = N u8, pix_off = N+1 int64, action = B u8, covered / owned = B int64, pixels.  Scratch: 32 bytes per
// polygon (the bounding box of V), the rows' item offsets and the scan's partial sums.
//
// Steps (no hand-off between workgroups inside a launch):
//   1. rows, a lane per row: status, pixel count and item count; two scans give pix_off and item_off;
//   2. polygons, a lane per polygon: the action and the bounding box; the host reads the pixel total and the item count;
//   3. paint, a wave (one workgroup) per item = (row, scanline, strip of `strip` columns), items taken grid-stride.  The wave
//      keeps the strip's owner per pixel (a polygon index), a parity byte per pixel and a list of crossings in LDS.  Per polygon
//      of the row, in order, culled by its box (k21_reaches): k21_edges puts the crossings of the scanline into the list, lanes
//      then take pixels and XOR in xs > xc for the listed crossings.
//      After the polygon's last edge the pixels of parity 1 take it as owner; their count goes to covered and owned, every
//      overwritten owner is decremented (aggregated by old owner inside the wave), all by integer atomics, so no result
//      depends on the schedule.  At the end of the item the owners are translated to val / background in LDS and stream out in
//      16-byte stores, byte by byte where the destination's alignment cuts a chunk.
#include "k13_scan.h"
#include "k21_cover.h"
#include "poly_table.h"
#include "sized_out.h"

namespace dyd {

constexpr int K21_BLOCK = 256;
constexpr int K21_STRIP = 1024;              // columns per item (default and most); 4 + 1 + 1 bytes of LDS per column
constexpr int K21_CROSSINGS = 256;           // capacity of the crossing list (default and most)
constexpr int64_t K21_MAX_PIXELS = 1LL << 30;
constexpr int64_t K21_MAX_GRID = 1 << 20;    // paint workgroups; the items beyond are taken grid-stride

// ---- 1. rows: a lane per row -----------------------------------------------------------------------------------
__global__ __launch_bounds__(K21_BLOCK) void k21_rows_kernel(const double *__restrict__ width, const double *__restrict__ height,
                                                             int64_t n_rows, int64_t max_pixels, int strip,
                                                             uint8_t *__restrict__ row_status, int64_t *__restrict__ pix_off,
                                                             int64_t *__restrict__ item_off) {
    const int64_t i = (int64_t)blockIdx.x * K21_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    int64_t w, h;
    row_status[i] = k21_row_size(width[i], height[i], max_pixels, &w, &h);
    pix_off[i + 1] = w * h;
    item_off[i + 1] = h * ((w + strip - 1) / strip);
    if (i == 0) pix_off[0] = item_off[0] = 0;
}

// ---- 2. polygons: a lane per polygon ---------------------------------------------------------------------------
// action and info as k21_cover.h says; K22 launches it too, once per table
__global__ __launch_bounds__(K21_BLOCK) void k21_poly_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                             const int32_t *__restrict__ row_off, const int32_t *__restrict__ val,
                                                             const uint8_t *__restrict__ row_status, int64_t n_rows, int64_t n_polys,
                                                             int64_t n_points, uint8_t *__restrict__ action, double *__restrict__ info) {
    __shared__ int32_t rows[2];
    const int64_t p0 = (int64_t)blockIdx.x * K21_BLOCK, p1 = min(p0 + K21_BLOCK, n_polys);
    poly_tile_rows(row_off, n_rows, p0, p1, rows);
    const int64_t p = p0 + threadIdx.x;
    if (p >= p1) return;
    const int64_t r = last_le(row_off, rows[0], rows[1], p);
    uint8_t act;
    double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0;
    if (val[p] < 0) {
        act = SEG_UNSELECTED;
    } else if (row_status[r] != 0) {
        act = COVER_NO_ROW;
    } else {
        const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
        Poly pg;
        act = k13_prepare(xy, a, b, pg);
        if (act == 0xff) {
            act = COVER_DONE;
            x1 = pg.x1; y1 = pg.y1; x2 = pg.x2; y2 = pg.y2;
        }
    }
    action[p] = act;
    double *q = info + 4 * p;
    q[0] = x1; q[1] = y1; q[2] = x2; q[3] = y2;
}

void k21_polys(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const uint8_t *row_status,
               int64_t n_rows, int64_t n_polys, int64_t n_points, uint8_t *action, double *info, hipStream_t st) {
    if (n_polys > 0)
        hipLaunchKernelGGL(k21_poly_kernel, dim3((unsigned)ceil_div(n_polys, (int64_t)K21_BLOCK)), dim3(K21_BLOCK), 0, st, xy, pt_off,
                           row_off, val, row_status, n_rows, n_polys, n_points, action, info);
}

// ---- 3. paint: a wave per item ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void k21_paint_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                          const int32_t *__restrict__ row_off, const int32_t *__restrict__ val,
                                                          const double *__restrict__ width, const double *__restrict__ height,
                                                          int64_t n_rows, int64_t n_polys, int64_t n_points, int background,
                                                          int strip, int cap, const uint8_t *__restrict__ row_status,
                                                          const int64_t *__restrict__ pix_off, const int64_t *__restrict__ item_off,
                                                          int64_t n_items, const uint8_t *__restrict__ action,
                                                          const double *__restrict__ info, unsigned long long *__restrict__ covered,
                                                          unsigned long long *__restrict__ owned, uint8_t *__restrict__ pixels) {
    __shared__ int32_t owner[K21_STRIP];
    __shared__ uint8_t parity[K21_STRIP];
    __shared__ double list[K21_CROSSINGS];
    __shared__ __attribute__((aligned(16))) uint8_t img[K21_STRIP + 16];
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t r = last_le(item_off, 0, n_rows - 1, item);
        const int64_t local = item - item_off[r];
        const int64_t W = (int64_t)width[r], H = (int64_t)height[r];
        const int64_t n_strips = (W + strip - 1) / strip;
        if (row_status[r] != 0 || local < 0 || local >= H * n_strips) continue;   // never for a sound item_off
        const int64_t j = local / n_strips, x0 = (local - j * n_strips) * strip;
        const int npx = (int)min((int64_t)strip, W - x0);
        const K21Strip s{(double)j + 0.5, (double)x0 + 0.5, (double)(x0 + npx - 1) + 0.5, x0, npx, (npx + kWave - 1) / kWave};
        for (int px = lane; px < npx; px += kWave) {
            owner[px] = -1;
            parity[px] = 0;
        }
        __syncthreads();
        // the crossings listed so far, XORed into the parity of every pixel of the strip
        auto apply = [&](int n_listed) __attribute__((always_inline)) {
            __syncthreads();
            for (int px = lane; px < npx; px += kWave) {
                const double xc = (double)(x0 + px) + 0.5;
                uint8_t par = parity[px];
                for (int c = 0; c < n_listed; ++c) par ^= (uint8_t)(list[c] > xc);
                parity[px] = par;
            }
            __syncthreads();
        };
        int64_t pa, pb;
        k21_row_polys(row_off, r, n_polys, &pa, &pb);
        for (int64_t p = pa; p < pb; ++p) {
            if (!k21_reaches(action, info, p, s)) continue;
            const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
            k21_edges(reinterpret_cast<const double2 *>(xy) + a, b - a, info + 4 * p, s.yc, cap, list, apply);
            // the covered pixels change hands
            int n_covered = 0;
            for (int base = 0; base < npx; base += kWave) {
                const int px = base + lane;
                const bool cov = px < npx && parity[px] != 0;
                int32_t old = -1;
                if (cov) {
                    old = owner[px];
                    owner[px] = (int32_t)p;
                    parity[px] = 0;
                }
                n_covered += __popcll(__ballot(cov));
                const bool lost = cov && old >= 0;
                unsigned long long todo = __ballot(lost);
                while (todo) {   // one atomic per distinct old owner among these 64 pixels
                    const int leader = __ffsll((long long)todo) - 1;
                    const int32_t o = __shfl(old, leader);
                    const unsigned long long same = __ballot(lost && old == o);
                    if (lane == leader) atomicAdd(owned + o, 0ull - (unsigned long long)__popcll(same));
                    todo &= ~same;
                }
            }
            if (lane == 0 && n_covered > 0) {
                atomicAdd(covered + p, (unsigned long long)n_covered);
                atomicAdd(owned + p, (unsigned long long)n_covered);
            }
        }
        // owners -> bytes.  img[0] stands for the 16-byte aligned address at or below the strip's first pixel.
        uint8_t *dst = pixels + pix_off[r] + j * W + x0;
        const int phase = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
        __syncthreads();
        for (int px = lane; px < npx; px += kWave) {
            const int32_t o = owner[px];
            img[phase + px] = (uint8_t)(o < 0 ? background : val[o]);
        }
        __syncthreads();
        const int lo = phase, hi = phase + npx;
        for (int c = lane; 16 * c < hi; c += kWave) {
            const int at = 16 * c;
            if (at >= lo && at + 16 <= hi) {
                *reinterpret_cast<uint4 *>(dst - phase + at) = *reinterpret_cast<const uint4 *>(img + at);
            } else {
                for (int k = max(at, lo); k < min(at + 16, hi); ++k) dst[k - phase] = img[k];
            }
        }
        __syncthreads();   // img, owner and parity are written again by the next item
    }
}

// dyd_set_option("k21_strip" / "k21_crossings", n): the strip's width and the list's capacity; <= 0 restores the default, larger
// values are capped
static int g_k21_strip = K21_STRIP, g_k21_crossings = K21_CROSSINGS;

void set_k21_strip(int v) { g_k21_strip = k21_capped(v, K21_STRIP); }
void set_k21_crossings(int v) { g_k21_crossings = k21_capped(v, K21_CROSSINGS); }

struct RasterOut {
    uint8_t *row_status;
    int64_t *pix_off;
    uint8_t *action;
    int64_t *covered, *owned;
};

static int raster_params(int32_t background, int64_t max_pixels) {
    DYD_REQUIRE(background >= 0 && background <= 255, "background must lie in 0..255");
    DYD_REQUIRE(max_pixels >= 1 && max_pixels <= K21_MAX_PIXELS, "max_pixels_per_row must lie in 1..2^30");
    return DYD_OK;
}

constexpr SizedName K21_PIXELS{"K21", "pixel", "bytes", 1};

// Steps 1 to 3 on device pointers.  `pixels` is asked for the buffer once the size is known (none: measure only).
// *total_out is a host value.
static int raster_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const double *width,
                         const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int32_t background,
                         int64_t max_pixels, const RasterOut &o, int64_t *total_out, SizedOut &pixels, hipStream_t st) {
    const int strip = g_k21_strip, cap = g_k21_crossings;
    const size_t info_bytes = 32 * (size_t)max(n_polys, (int64_t)1), item_bytes = 8 * (size_t)(n_rows + 1);
    ScratchLease lease(st);
    void *scr = nullptr;
    int rc = lease.get(info_bytes + item_bytes + 8 * (size_t)k13_scan_parts(n_rows), &scr);
    if (rc) return rc;
    double *info = static_cast<double *>(scr);
    int64_t *item_off = reinterpret_cast<int64_t *>(info + info_bytes / 8), *part = item_off + n_rows + 1;
    hipLaunchKernelGGL(k21_rows_kernel, dim3((unsigned)ceil_div(n_rows, (int64_t)K21_BLOCK)), dim3(K21_BLOCK), 0, st, width, height,
                       n_rows, max_pixels, strip, o.row_status, o.pix_off, item_off);
    k13_scan_inclusive(o.pix_off + 1, n_rows, part, st);
    k13_scan_inclusive(item_off + 1, n_rows, part, st);   // after the first scan in the stream, so the partial sums are free again
    k21_polys(xy, pt_off, row_off, val, o.row_status, n_rows, n_polys, n_points, o.action, info, st);
    int64_t total = 0, n_items = 0;
    if ((rc = read_totals("K21", "the row and polygon steps", {{&total, o.pix_off + n_rows}, {&n_items, item_off + n_rows}}, st)))
        return rc;
    *total_out = total;
    if ((rc = pixels.get(total)) || !pixels.p) return rc;
    if (n_polys > 0) {
        hipError_t e = hipMemsetAsync(o.covered, 0, 8 * (size_t)n_polys, st);
        if (e == hipSuccess) e = hipMemsetAsync(o.owned, 0, 8 * (size_t)n_polys, st);
        if (e != hipSuccess) {
            set_error("K21: clearing the counters failed: %s", hipGetErrorString(e));
            return DYD_ERR_HIP;
        }
    }
    if (n_items > 0)
        hipLaunchKernelGGL(k21_paint_kernel, dim3((unsigned)(n_items < K21_MAX_GRID ? n_items : K21_MAX_GRID)), dim3(kWave), 0, st, xy, pt_off, row_off, val,
                           width, height, n_rows, n_polys, n_points, (int)background, strip, cap, o.row_status, o.pix_off, item_off,
                           n_items, o.action, info, reinterpret_cast<unsigned long long *>(o.covered),
                           reinterpret_cast<unsigned long long *>(o.owned), pixels.as<uint8_t>());
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_rasterize_polygons_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const double *width,
                               const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int32_t background,
                               int64_t max_pixels_per_row, uint8_t *out_row_status, int64_t *out_pix_off, uint8_t *out_action,
                               int64_t *out_covered, int64_t *out_owned, uint8_t *out_pixels_or_null, int64_t pix_cap,
                               int64_t *out_total, void *stream) {
    DYD_API_ENTER();
    int rc = raster_params(background, max_pixels_per_row);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && pix_cap >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31) && n_rows < (1LL << 31), "size too large");
    DYD_REQUIRE(out_pix_off && out_total, "null pointer");
    hipStream_t st = pick_stream(stream);
    if (n_rows == 0) {
        DYD_HIP(hipMemsetAsync(out_pix_off, 0, 8, st));
        *out_total = 0;
        return DYD_OK;
    }
    DYD_REQUIRE(row_off && width && height && out_row_status, "null pointer");
    DYD_REQUIRE(n_polys == 0 || (pt_off && val && out_action), "null pointer");
    DYD_REQUIRE(n_polys == 0 || !out_pixels_or_null || (out_covered && out_owned), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    const RasterOut o{out_row_status, out_pix_off, out_action, out_covered, out_owned};
    SizedOut pixels(K21_PIXELS, out_pixels_or_null, pix_cap);
    return raster_launch(xy, pt_off, row_off, val, width, height, n_rows, n_polys, n_points, background, max_pixels_per_row, o,
                         out_total, pixels, st);
}

int dyd_rasterize_polygons(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *val, const double *width,
                           const double *height, int64_t n_rows, int32_t background, int64_t max_pixels_per_row,
                           uint8_t *out_row_status, int64_t *out_pix_off, uint8_t *out_action, int64_t *out_covered,
                           int64_t *out_owned, uint8_t **out_pixels, int64_t *out_pixels_len) {
    DYD_API_ENTER();
    int rc = raster_params(background, max_pixels_per_row);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31), "size too large");
    DYD_REQUIRE(out_pix_off && out_pixels && out_pixels_len, "null pointer");
    *out_pixels = nullptr;
    *out_pixels_len = 0;
    out_pix_off[0] = 0;
    if (n_rows == 0) return DYD_OK;
    int64_t n_polys = 0, n_points = 0;
    rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, out_row_status != nullptr,
                          val && out_action && out_covered && out_owned, nullptr, 0, &n_polys, &n_points);
    if (rc) return rc;
    for (int64_t p = 0; p < n_polys; ++p) DYD_REQUIRE(val[p] <= 255, "val above 255");
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_val, d_status, d_poff, d_act, d_cov, d_own;
    const size_t nb8 = 8 * (size_t)n_polys;
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, n_polys, n_points)) ||
        (rc = poly_column(d_val, val, 4 * (size_t)n_polys)) || (rc = d_status.alloc((size_t)n_rows)) ||
        (rc = d_poff.alloc(8 * (size_t)(n_rows + 1))) || (rc = d_act.alloc((size_t)n_polys)) || (rc = d_cov.alloc(nb8)) ||
        (rc = d_own.alloc(nb8)))
        return rc;
    const RasterOut o{d_status.as<uint8_t>(), d_poff.as<int64_t>(), d_act.as<uint8_t>(), d_cov.as<int64_t>(), d_own.as<int64_t>()};
    SizedOut pixels(K21_PIXELS, st);
    int64_t total = 0;
    KernelTimer timer(st);
    rc = raster_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), d_val.as<int32_t>(), t.w.as<double>(),
                       t.h.as<double>(), n_rows, n_polys, n_points, background, max_pixels_per_row, o, &total, pixels, st);
    if (rc) return rc;
    timer.finish();
    return hand_back_text(pixels.p, total,
                          {{out_row_status, d_status.p, (size_t)n_rows}, {out_pix_off, d_poff.p, 8 * (size_t)(n_rows + 1)},
                           {out_action, d_act.p, (size_t)n_polys}, {out_covered, d_cov.p, nb8}, {out_owned, d_own.p, nb8}},
                          st, out_pixels, out_pixels_len);
}

}  // extern "C"
