// k17_obb.hip — K17: YOLO oriented-box label lines.
//
// One line per annotation polygon in the form YOLO OBB models read, "cls x1 y1 x2 y2 x3 y3 x4 y4" with every value normalised
// to [0, 1]: the four corners of a minimum-area rectangle that encloses the polygon's clipped vertices (include/dyd.h and
// DESIGN §5o have the definition):
//   - polygons, checks, the two-point rule, the clip to [0, W] x [0, H] and actions 0..5 are K13's (k13_poly.h, the same code);
//   - a gift-wrapping walk over the clipped vertices C visits the hull's edges from the lowest vertex; every edge gives the
//     rectangle of C's extents along and across it (an axis-aligned edge: C's own extent), the first of the smallest area is
//     kept; no area > 0: flat (6), no line;
//   - every min and max is a strict comparison (the first value wins a tie), never fmin / fmax, all of it IEEE f64 without
//     contraction (-ffp-contract=off), so a restatement in Python gives the same bits;
//   - a corner outside the image is clamped by the printer (K13's n) and the polygon's `clamped` is set;
//   - a line is digits(cls) + 72 bytes.
//
// Layout in HBM: xy = P x (x, y) f64 (16-B aligned), pt_off = B+1 int32, row_off = N+1 int32, optional sel = B u8, width /
// height = N f64, class_id = N int32.  Out: text_off = N+1 int64, flag = N u8, action = B u8, clamped = B u8, corners = B x 8 f64
// (optional), text = T bytes.
// Algorithmic bytes: 16*P + 4*(B+1) + B + 4*(N+1) + 20*N in, 8*(N+1) + N + 2*B + 64*B + T out.  Bound: HBM for short polygons;
// a polygon of m clipped vertices and h hull edges costs (h + 2) passes over its points, so long ones are bound by f64 VALU.
//
// Four steps, no hand-off between workgroups inside a launch:
//   1. walk, a lane per polygon over 256-polygon tiles (K14's mapping: two lanes find the tile's first and last row, every lane
//      searches between them): k13_prepare, then k17_rectangle (k17_walk.h): one pass over C for its count, extent and lowest
//      vertex, then one pass per hull edge that takes the extents along the edge found last and selects the next edge at once
//      (no operation on any single value differs from two separate passes).  Every pass runs the clip again: O(1) state, no
//      per-lane array.  An unclipped two-point polygon is its box.  Writes the action, `clamped` and the corners;
//   2. rows, a lane per row: the row's lines, each printed polygon's place among them, the row's flag and byte count;
//   3. k13_seg.hip's int64 scan over the rows' byte counts (k13_scan.h);
//   4. print, a workgroup per 256-polygon tile: the tile's lines are one range of the text (lines are in polygon order and of a
//      fixed length), so a lane prints its line from the stored corners into an LDS image of that range and the image streams
//      out with 16-byte stores; the range's cut ends go byte by byte.  A line's "\n" belongs to the line after it.
#include "k13_poly.h"
#include "k13_scan.h"
#include "k17_walk.h"
#include "poly_table.h"
#include "round6.h"
#include "sized_out.h"

namespace dyd {

constexpr int K17_BLOCK = 256;
constexpr int K17_VALUES = 72;              // 8 x " 0.123456"
constexpr int K17_LINE_MAX = 10 + K17_VALUES + 1;          // a class id below 2^31, the values, the "\n" before the line
constexpr int K17_IMAGE = K17_BLOCK * K17_LINE_MAX + 16;   // a tile's lines and the 16-byte phase of their first byte

// ---- 1. walk: a lane per polygon -------------------------------------------------------------------------------
__global__ __launch_bounds__(K17_BLOCK) void k17_walk_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                             const int32_t *__restrict__ row_off, const uint8_t *__restrict__ sel,
                                                             const double *__restrict__ width, const double *__restrict__ height,
                                                             int64_t n_rows, int64_t n_polys, int64_t n_points,
                                                             uint8_t *__restrict__ out_action, uint8_t *__restrict__ out_clamped,
                                                             double *__restrict__ corners) {
    __shared__ int32_t rows[2];
    const int64_t p0 = (int64_t)blockIdx.x * K17_BLOCK;
    poly_tile_rows(row_off, n_rows, p0, min(p0 + K17_BLOCK, n_polys), rows);
    const int64_t p = p0 + threadIdx.x;
    if (p >= n_polys) return;
    uint8_t act = SEG_UNSELECTED, clamped = 0;
    if (!sel || sel[p]) {
        const int64_t r = last_le(row_off, rows[0], rows[1], p);
        const double W = width[r], H = height[r];
        if (!k13_size_ok(W) || !k13_size_ok(H)) {
            act = SEG_NO_SIZE;
        } else {
            const int32_t a0 = max(pt_off[p], 0), b0 = (int32_t)min((int64_t)max(pt_off[p + 1], a0), n_points);   // as K13
            Poly pg;
            act = k13_prepare(xy, a0, b0, pg);
            if (act == 0xff) {
                double c[8];
                act = k17_rectangle(pg, k13_outside(pg, W, H), W, H, c, clamped);
                if (act <= SEG_CLIPPED) {
                    double2 *dst = reinterpret_cast<double2 *>(corners + 8 * p);
#pragma unroll
                    for (int k = 0; k < 4; ++k) dst[k] = make_double2(c[2 * k], c[2 * k + 1]);
                }
            }
        }
    }
    out_action[p] = act;
    out_clamped[p] = clamped;
}

// ---- 2. rows: a lane per row -----------------------------------------------------------------------------------
// rel[p] = the printed polygon's place among its row's lines; text_off[i + 1] = the row's byte count
__global__ __launch_bounds__(K17_BLOCK) void k17_rows_kernel(const int32_t *__restrict__ row_off, const double *__restrict__ width,
                                                             const double *__restrict__ height, const int32_t *__restrict__ class_id,
                                                             const uint8_t *__restrict__ action, int64_t n_rows, int64_t n_polys,
                                                             int64_t *__restrict__ text_off, uint8_t *__restrict__ flag,
                                                             int32_t *__restrict__ rel) {
    const int64_t i = (int64_t)blockIdx.x * K17_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const int32_t cid = class_id[i];
    const bool host = width[i] == 0.0 || height[i] == 0.0 || cid < 0;
    const int64_t p0 = max((int64_t)row_off[i], (int64_t)0), p1 = min((int64_t)row_off[i + 1], n_polys);
    int32_t lines = 0;
    for (int64_t p = p0; p < p1; ++p)
        if (action[p] <= SEG_CLIPPED) rel[p] = lines++;
    const uint8_t f = host ? 2 : (lines ? 0 : 1);
    flag[i] = f;
    text_off[i + 1] = f == 0 ? (int64_t)lines * (k13_digits(cid) + K17_VALUES + 1) - 1 : 0;
    if (i == 0) text_off[0] = 0;
}

// ---- 4. print: a workgroup per polygon tile --------------------------------------------------------------------
__global__ __launch_bounds__(K17_BLOCK) void k17_print_kernel(const int32_t *__restrict__ row_off, const double *__restrict__ width,
                                                              const double *__restrict__ height, const int32_t *__restrict__ class_id,
                                                              int64_t n_rows, int64_t n_polys, const int64_t *__restrict__ text_off,
                                                              const uint8_t *__restrict__ flag, const uint8_t *__restrict__ action,
                                                              const int32_t *__restrict__ rel, const double *__restrict__ corners,
                                                              int64_t total, uint8_t *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint8_t img[K17_IMAGE];
    __shared__ int32_t rows[2];
    __shared__ unsigned long long span[2];     // the tile's text bytes [span[0], span[1])
    if (threadIdx.x == 0) {
        span[0] = ~0ull;
        span[1] = 0;
    }
    const int64_t p0 = (int64_t)blockIdx.x * K17_BLOCK;
    poly_tile_rows(row_off, n_rows, p0, min(p0 + K17_BLOCK, n_polys), rows);
    const int64_t p = p0 + threadIdx.x;
    bool has = false;
    int64_t r = 0, start = 0;
    int32_t cid = 0, j = 0;
    int cd = 0;
    if (p < n_polys && action[p] <= SEG_CLIPPED) {
        r = last_le(row_off, rows[0], rows[1], p);
        if (flag[r] == 0) {
            has = true;
            cid = class_id[r];
            cd = k13_digits(cid);
            j = rel[p];
            start = text_off[r] + (int64_t)j * (cd + K17_VALUES + 1);
            atomicMin(&span[0], (unsigned long long)(j > 0 ? start - 1 : start));
            atomicMax(&span[1], (unsigned long long)(start + cd + K17_VALUES));
        }
    }
    __syncthreads();
    const int64_t lo = (int64_t)span[0], hi = (int64_t)span[1];
    if (hi == 0) return;                        // no line in this tile
    const int64_t base = lo - (int64_t)((reinterpret_cast<uintptr_t>(text) + (uint64_t)lo) & 15u);   // text + base is 16-byte aligned
    if (lo < 0 || hi > total || hi - base > K17_IMAGE) return;   // offsets that do not describe a table: write nothing
    if (has) {
        uint8_t *o = img + (start - base);
        if (j > 0) o[-1] = '\n';
        uint32_t v = (uint32_t)cid;
        for (int k = cd - 1; k >= 0; --k) {
            const uint32_t d = v / 10u;
            o[k] = (uint8_t)('0' + (v - d * 10u));
            v = d;
        }
        o += cd;
        const double W = width[r], H = height[r];
        const double2 *src = reinterpret_cast<const double2 *>(corners + 8 * p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double2 c = src[k];
            const uint64_t nx = k13_num8(c.x / W), ny = k13_num8(c.y / H);
            o[18 * k] = ' ';
#pragma unroll
            for (int b = 0; b < 8; ++b) o[18 * k + 1 + b] = (uint8_t)(nx >> (8 * b));
            o[18 * k + 9] = ' ';
#pragma unroll
            for (int b = 0; b < 8; ++b) o[18 * k + 10 + b] = (uint8_t)(ny >> (8 * b));
        }
    }
    __syncthreads();
    for (int64_t c = threadIdx.x; base + 16 * c < hi; c += K17_BLOCK) {
        const int64_t a = base + 16 * c;
        if (a >= lo && a + 16 <= hi) {
            *reinterpret_cast<uint4 *>(text + a) = *reinterpret_cast<const uint4 *>(img + 16 * c);
        } else {
            for (int k = 0; k < 16; ++k)
                if (a + k >= lo && a + k < hi) text[a + k] = img[16 * c + k];
        }
    }
}

constexpr SizedName K17_TEXT{"K17", "text", "bytes", 1};

// Walk, rows, scan and print on device pointers, n_rows > 0.  `text` is asked for the buffer once the size is known (none:
// measure only); *total_out is a host value.
static int obb_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel, const double *width,
                      const double *height, const int32_t *class_id, int64_t n_rows, int64_t n_polys, int64_t n_points,
                      int64_t *text_off, uint8_t *flag, uint8_t *action, uint8_t *clamped, double *corners_or_null, SizedOut &text,
                      int64_t *total_out, hipStream_t st) {
    DevBuf d_rel, d_part, d_corners;
    int rc;
    if ((rc = d_rel.alloc(4 * (size_t)n_polys, st)) || (rc = d_part.alloc(8 * (size_t)k13_scan_parts(n_rows), st))) return rc;
    double *cor = corners_or_null;             // the caller's corners, or d_corners
    if (!cor) {
        if ((rc = d_corners.alloc(64 * (size_t)n_polys, st))) return rc;
        cor = d_corners.as<double>();
    }
    if (n_polys > 0)
        hipLaunchKernelGGL(k17_walk_kernel, dim3((unsigned)ceil_div(n_polys, (int64_t)K17_BLOCK)), dim3(K17_BLOCK), 0, st, xy, pt_off,
                           row_off, sel, width, height, n_rows, n_polys, n_points, action, clamped, cor);
    hipLaunchKernelGGL(k17_rows_kernel, dim3((unsigned)ceil_div(n_rows, (int64_t)K17_BLOCK)), dim3(K17_BLOCK), 0, st, row_off, width,
                       height, class_id, action, n_rows, n_polys, text_off, flag, d_rel.as<int32_t>());
    k13_scan_inclusive(text_off + 1, n_rows, d_part.as<int64_t>(), st);
    int64_t total = 0;
    if ((rc = read_totals("K17", "the measure step", {{&total, text_off + n_rows}}, st))) return rc;
    *total_out = total;
    if (total == 0 || (rc = text.get(total)) || !text.p) return rc;
    hipLaunchKernelGGL(k17_print_kernel, dim3((unsigned)ceil_div(n_polys, (int64_t)K17_BLOCK)), dim3(K17_BLOCK), 0, st, row_off, width,
                       height, class_id, n_rows, n_polys, text_off, flag, action, d_rel.as<int32_t>(), cor, total, text.as<uint8_t>());
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_yolo_obb_lines_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                           const double *width, const double *height, const int32_t *class_id, int64_t n_rows, int64_t n_polys,
                           int64_t n_points, int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_action, uint8_t *out_clamped,
                           double *out_corners_or_null, uint8_t *out_text_or_null, int64_t text_cap, int64_t *out_total,
                           void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && text_cap >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31) && n_rows < (1LL << 31), "size exceeds int32 offsets");
    DYD_REQUIRE(out_text_off, "null pointer");
    hipStream_t st = pick_stream(stream);
    if (n_rows == 0) {
        DYD_HIP(hipMemsetAsync(out_text_off, 0, 8, st));
        if (out_total) *out_total = 0;
        return DYD_OK;
    }
    DYD_REQUIRE(row_off && width && height && class_id && out_flag, "null pointer");
    DYD_REQUIRE(n_polys == 0 || (pt_off && out_action && out_clamped), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(xy) & 15) == 0, "xy must be 16-byte aligned");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(out_corners_or_null) & 15) == 0, "out_corners must be 16-byte aligned");
    SizedOut text(K17_TEXT, out_text_or_null, text_cap);
    int64_t total = 0;
    const int rc = obb_launch(xy, pt_off, row_off, sel_or_null, width, height, class_id, n_rows, n_polys, n_points, out_text_off,
                              out_flag, out_action, out_clamped, out_corners_or_null, text, &total, st);
    if (out_total && (rc == DYD_OK || rc == DYD_ERR_RANGE)) *out_total = total;
    return rc;
}

int dyd_yolo_obb_lines(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                       const double *width, const double *height, const int32_t *class_id, int64_t n_rows, int64_t *out_text_off,
                       uint8_t *out_flag, uint8_t *out_action, uint8_t *out_clamped, double *out_corners_or_null, uint8_t **out_text,
                       int64_t *out_text_len) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31), "size exceeds int32 offsets");
    DYD_REQUIRE(out_text_off && out_text && out_text_len, "null pointer");
    *out_text = nullptr;
    *out_text_len = 0;
    out_text_off[0] = 0;
    if (n_rows == 0) return DYD_OK;
    int64_t n_polys = 0, n_points = 0;
    int rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, class_id && out_flag, out_action && out_clamped, nullptr, 0,
                              &n_polys, &n_points);
    if (rc) return rc;
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_sel, d_cid, d_toff, d_flag, d_act, d_cl, d_cor;
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, n_polys, n_points)) ||
        (rc = poly_column(d_sel, sel_or_null, (size_t)n_polys)) || (rc = poly_column(d_cid, class_id, 4 * (size_t)n_rows)) ||
        (rc = d_toff.alloc(8 * (size_t)(n_rows + 1))) || (rc = d_flag.alloc((size_t)n_rows)) || (rc = d_act.alloc((size_t)n_polys)) ||
        (rc = d_cl.alloc((size_t)n_polys)))
        return rc;
    // the caller's corners go up first, so that a polygon without a line keeps what the caller had there
    if (out_corners_or_null && (rc = poly_column(d_cor, out_corners_or_null, 64 * (size_t)n_polys))) return rc;
    const uint8_t *sel = sel_or_null ? d_sel.as<uint8_t>() : nullptr;
    SizedOut text(K17_TEXT, st);
    int64_t total = 0;
    KernelTimer timer(st);
    rc = obb_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), sel, t.w.as<double>(), t.h.as<double>(),
                    d_cid.as<int32_t>(), n_rows, n_polys, n_points, d_toff.as<int64_t>(), d_flag.as<uint8_t>(), d_act.as<uint8_t>(),
                    d_cl.as<uint8_t>(), out_corners_or_null ? d_cor.as<double>() : nullptr, text, &total, st);
    if (rc) return rc;
    timer.finish();
    return hand_back_text(text.p, total,
                          {{out_text_off, d_toff.p, 8 * (size_t)(n_rows + 1)}, {out_flag, d_flag.p, (size_t)n_rows},
                           {out_action, d_act.p, (size_t)n_polys}, {out_clamped, d_cl.p, (size_t)n_polys},
                           {out_corners_or_null, d_cor.p, out_corners_or_null ? 64 * (size_t)n_polys : 0}},
                          st, out_text, out_text_len);
}

}  // extern "C"
