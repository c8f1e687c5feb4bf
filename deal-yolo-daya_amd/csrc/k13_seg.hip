// k13_seg.hip — K13: YOLO segmentation label lines.
//
// One line per annotation polygon in the form YOLO segment models read, "cls x1 y1 ... xn yn" with every value
// normalised to [0, 1], for the polygons of a split-sheet row that carry the row's label (include/dyd.h has the
// definition):
//   - a polygon of exactly two points is the box they span, as four corners;
//   - Sutherland-Hodgman clips it to [0, W] x [0, H], passes x >= 0, x <= W, y >= 0, y <= H in that order, every
//     intersection computed from the edge's first point towards its second in IEEE f64 (-ffp-contract=off);
//   - every value prints as "%.6f" of n(v / W) or n(v / H), n clamping to [0, 1], so it is exactly 8 bytes and a line is
//     digits(cls) + 18 * m bytes for m clipped vertices.  round6.h rounds half-to-even on the exact binary value.
// The four passes run as a pipeline, vertex by vertex, with O(1) state per pass: a pass emits p before the crossing of
// the edge (p, q), so feeding each pass's output straight into the next gives the same sequence as four whole passes.
//
// Layout in HBM: xy = P x (x, y) f64, pt_off = B+1 int32, row_off = N+1 int32, optional sel = B u8, width / height = N f64,
// class_id = N int32.  Outputs: text_off = N+1 int64, flag = N u8, action = B u8, text = T bytes.
// Algorithmic bytes: 16*P + 4*(B+1) + B + 4*(N+1) + 20*N in, 8*(N+1) + N + B + T out.  Bound: HBM.
//
// Three steps, no hand-off between workgroups inside a launch:
//   1. measure, a lane per row: per polygon the action and the clipped vertex count m (a polygon whose bounding box lies
//      in the image needs no clipping: its vertices are the line), the line's place in the row, the row's byte count;
//   2. an exclusive scan of the row byte counts into text_off (reduce, scan of the block sums, apply);
//   3. print, a workgroup per K13_WINDOW bytes of output: the polygons whose line meets the window print the part inside
//      it into LDS (a lane per polygon, clipping again where needed), and the window streams out with 16-byte stores.
//      The window is aligned to 16 bytes of the text's address, so neighbouring workgroups share no 16-byte chunk.
#include "k13_poly.h"
#include "k13_scan.h"
#include "poly_table.h"
#include "round6.h"
#include "sized_out.h"
#include "text_window.h"

namespace dyd {

constexpr int K13_BLOCK = 256;
constexpr int K13_SCAN_PER_LANE = 8;
constexpr int K13_SCAN_TILE = K13_BLOCK * K13_SCAN_PER_LANE;
constexpr int K13_WINDOW = 32 * 1024;       // bytes of text per print workgroup (multiple of 16)
constexpr int K13_ROWS_LDS = 1024;          // row_off entries a print workgroup stages in LDS for its row lookups

// ---- 1. measure: a lane per row ------------------------------------------------------------------------------
// rel[p] = the line's first byte within the row, m[p] = its clipped vertex count; text_off[i + 1] = the row's byte count
__global__ __launch_bounds__(K13_BLOCK) void k13_measure_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                                const int32_t *__restrict__ row_off, const uint8_t *__restrict__ sel,
                                                                const double *__restrict__ width, const double *__restrict__ height,
                                                                const int32_t *__restrict__ class_id, int64_t n_rows, int64_t n_polys,
                                                                int64_t n_points, int64_t *__restrict__ text_off,
                                                                uint8_t *__restrict__ flag, uint8_t *__restrict__ action,
                                                                int64_t *__restrict__ rel, int32_t *__restrict__ mcount) {
    const int64_t i = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const double W = width[i], H = height[i];
    const int32_t cid = class_id[i];
    const bool size_ok = k13_size_ok(W) && k13_size_ok(H);
    const bool host = W == 0.0 || H == 0.0 || cid < 0;
    const int cd = cid >= 0 ? k13_digits(cid) : 0;
    const int64_t p0 = max((int64_t)row_off[i], (int64_t)0), p1 = min((int64_t)row_off[i + 1], n_polys);
    int64_t bytes = 0, lines = 0;
    for (int64_t p = p0; p < p1; ++p) {
        uint8_t act;
        int m = 0;
        if (sel && !sel[p]) {
            act = SEG_UNSELECTED;
        } else if (!size_ok) {
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
                    m = w.m;
                }
            }
        }
        action[p] = act;
        mcount[p] = m;
        if (act <= SEG_CLIPPED) {
            const int64_t at = bytes + (lines ? 1 : 0);
            rel[p] = at;
            bytes = at + cd + 18 * (int64_t)m;
            ++lines;
        }
    }
    const uint8_t f = host ? 2 : (lines ? 0 : 1);
    flag[i] = f;
    text_off[i + 1] = f == 0 ? bytes : 0;
    if (i == 0) text_off[0] = 0;
}

// ---- 2. exclusive scan of the row byte counts: v[0..n) inclusive, in place -------------------------------------------
__device__ __forceinline__ int64_t k13_block_incl_scan(int64_t x, int64_t *sh) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int d = 1; d < K13_BLOCK; d <<= 1) {
        const int64_t y = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    const int64_t r = sh[t];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(K13_BLOCK) void k13_scan_reduce_kernel(const int64_t *__restrict__ v, int64_t n, int64_t *__restrict__ part) {
    __shared__ int64_t sh[K13_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * K13_SCAN_TILE;
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < K13_SCAN_PER_LANE; ++k) {
        const int64_t j = base + (int64_t)k * K13_BLOCK + threadIdx.x;
        if (j < n) s += v[j];
    }
    s = k13_block_incl_scan(s, sh);
    if (threadIdx.x == K13_BLOCK - 1) part[blockIdx.x] = s;
}

// one workgroup: part[0..np) -> exclusive prefix
__global__ __launch_bounds__(K13_BLOCK) void k13_scan_parts_kernel(int64_t *__restrict__ part, int64_t np) {
    __shared__ int64_t sh[K13_BLOCK];
    int64_t carry = 0;
    for (int64_t b = 0; b < np; b += K13_BLOCK) {
        const int64_t j = b + threadIdx.x;
        const int64_t x = j < np ? part[j] : 0;
        const int64_t inc = k13_block_incl_scan(x, sh);
        if (j < np) part[j] = carry + inc - x;
        carry += sh[K13_BLOCK - 1];   // the chunk's total (sh is not written again before the barrier below)
        __syncthreads();
    }
}

__global__ __launch_bounds__(K13_BLOCK) void k13_scan_apply_kernel(int64_t *__restrict__ v, int64_t n, const int64_t *__restrict__ part) {
    __shared__ int64_t sh[K13_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * K13_SCAN_TILE + (int64_t)threadIdx.x * K13_SCAN_PER_LANE;
    int64_t x[K13_SCAN_PER_LANE], s = 0;
#pragma unroll
    for (int k = 0; k < K13_SCAN_PER_LANE; ++k) {
        x[k] = base + k < n ? v[base + k] : 0;
        s += x[k];
    }
    int64_t run = k13_block_incl_scan(s, sh) - s + part[blockIdx.x];
#pragma unroll
    for (int k = 0; k < K13_SCAN_PER_LANE; ++k) {
        run += x[k];
        if (base + k < n) v[base + k] = run;
    }
}

// the three launches on v[0..n), part = ceil(n / K13_SCAN_TILE) int64 of scratch (K16 scans its polygons' byte counts with them)
int64_t k13_scan_parts(int64_t n) { return ceil_div(n, (int64_t)K13_SCAN_TILE); }

void k13_scan_inclusive(int64_t *v, int64_t n, int64_t *part, hipStream_t st) {
    const int64_t n_parts = k13_scan_parts(n);
    hipLaunchKernelGGL(k13_scan_reduce_kernel, dim3((unsigned)n_parts), dim3(K13_BLOCK), 0, st, v, n, part);
    hipLaunchKernelGGL(k13_scan_parts_kernel, dim3(1), dim3(K13_BLOCK), 0, st, part, n_parts);
    hipLaunchKernelGGL(k13_scan_apply_kernel, dim3((unsigned)n_parts), dim3(K13_BLOCK), 0, st, v, n, part);
}

// ---- 3. print ------------------------------------------------------------------------------------------------
// window t = text bytes [t * K13_WINDOW - phase, (t + 1) * K13_WINDOW - phase) within [0, T): rows[2t], rows[2t + 1] = the rows
// holding its first and its last byte
__global__ __launch_bounds__(K13_BLOCK) void k13_tile_rows_kernel(const int64_t *__restrict__ text_off, int64_t n_rows, int64_t total,
                                                                  int64_t phase, int64_t n_tiles, int64_t *__restrict__ rows) {
    const int64_t t = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x;
    if (t >= n_tiles) return;
    const int64_t lo = max(t * K13_WINDOW - phase, (int64_t)0), hi = min((t + 1) * K13_WINDOW - phase, total);
    rows[2 * t] = min(last_le(text_off, 0, n_rows, lo), n_rows - 1);
    rows[2 * t + 1] = min(last_le(text_off, 0, n_rows, hi - 1), n_rows - 1);
}

__global__ __launch_bounds__(K13_BLOCK) void k13_print_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                              const int32_t *__restrict__ row_off, const double *__restrict__ width,
                                                              const double *__restrict__ height, const int32_t *__restrict__ class_id,
                                                              int64_t n_polys, int64_t n_points, const int64_t *__restrict__ text_off,
                                                              const uint8_t *__restrict__ flag, const uint8_t *__restrict__ action,
                                                              const int64_t *__restrict__ rel, const int32_t *__restrict__ mcount,
                                                              const int64_t *__restrict__ tile_rows, int64_t total, int64_t phase,
                                                              uint8_t *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint8_t img[K13_WINDOW];
    __shared__ int32_t srow[K13_ROWS_LDS];
    const int64_t t = blockIdx.x;
    const int64_t base = t * K13_WINDOW - phase;   // text byte at img[0]
    const int64_t wlo = max(base, (int64_t)0), whi = min(base + K13_WINDOW, total);
    const int64_t ra = tile_rows[2 * t], rb = tile_rows[2 * t + 1];
    const int64_t nr = rb - ra + 2;                // row_off[ra .. rb + 1]
    const bool staged = nr <= K13_ROWS_LDS;
    if (staged)
        for (int64_t k = threadIdx.x; k < nr; k += K13_BLOCK) srow[k] = row_off[ra + k];
    __syncthreads();
    const int64_t q0 = max((int64_t)(staged ? srow[0] : row_off[ra]), (int64_t)0);
    const int64_t q1 = min((int64_t)(staged ? srow[nr - 1] : row_off[rb + 1]), n_polys);
    auto put = [&](int64_t a, uint8_t c) {
        if (a >= wlo && a < whi) img[a - base] = c;
    };
    for (int64_t p = q0 + threadIdx.x; p < q1; p += K13_BLOCK) {
        if (action[p] > SEG_CLIPPED) continue;
        const int64_t r = staged ? ra + last_le(srow, 0, nr - 2, p) : last_le(row_off, ra, rb, p);
        if (flag[r] != 0) continue;
        const int32_t cid = class_id[r];
        const int cd = k13_digits(cid);
        const int64_t start = text_off[r] + rel[p];
        const int64_t len = cd + 18 * (int64_t)mcount[p];
        const int64_t first = rel[p] > 0 ? start - 1 : start;
        if (start + len <= wlo || first >= whi) continue;
        if (first < start) put(first, '\n');
        {
            uint32_t v = (uint32_t)cid;
            for (int k = cd - 1; k >= 0; --k) {
                const uint32_t d = v / 10u;
                put(start + k, (uint8_t)('0' + (v - d * 10u)));
                v = d;
            }
        }
        const double W = width[r], H = height[r];
        const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
        Poly pg;
        (void)k13_prepare(xy, a, b, pg);
        int64_t at = start + cd;                   // the next vertex's " x y"
        auto print = [&](double x, double y) {
            if (at >= whi) return false;
            if (at + 18 > wlo) {
                const uint64_t nx = k13_num8(x / W), ny = k13_num8(y / H);
                put(at, ' ');
#pragma unroll
                for (int k = 0; k < 8; ++k) put(at + 1 + k, (uint8_t)(nx >> (8 * k)));
                put(at + 9, ' ');
#pragma unroll
                for (int k = 0; k < 8; ++k) put(at + 10 + k, (uint8_t)(ny >> (8 * k)));
            }
            at += 18;
            return true;
        };
        k13_vertices(pg, k13_outside(pg, W, H), W, H, print);
    }
    __syncthreads();
    // stream the window out: text + base is 16-byte aligned; chunks cut by the text's ends go byte by byte
    for (int64_t c = threadIdx.x; c < K13_WINDOW / 16; c += K13_BLOCK) {
        const int64_t a = base + 16 * c;
        if (a + 16 <= wlo || a >= whi) continue;
        if (a >= wlo && a + 16 <= whi) {
            *reinterpret_cast<uint4 *>(text + a) = *reinterpret_cast<const uint4 *>(img + 16 * c);
        } else {
            for (int k = 0; k < 16; ++k)
                if (a + k >= wlo && a + k < whi) text[a + k] = img[16 * c + k];
        }
    }
}

constexpr SizedName K13_TEXT{"K13", "text", "bytes", 1};

// Measure, scan and print on device pointers.  `text` is asked for the buffer once the size is known (none: measure only);
// *total_out is a host value.
static int seg_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel, const double *width,
                      const double *height, const int32_t *class_id, int64_t n_rows, int64_t n_polys, int64_t n_points,
                      int64_t *text_off, uint8_t *flag, uint8_t *action, SizedOut &text, int64_t *total_out, hipStream_t st) {
    const int64_t n_parts = k13_scan_parts(n_rows);
    const size_t rel_bytes = 8 * (size_t)max(n_polys, (int64_t)1), m_bytes = 4 * (size_t)max(n_polys, (int64_t)1);
    const size_t part_bytes = 8 * (size_t)n_parts;
    ScratchLease lease(st);
    void *scr = nullptr;
    int rc = lease.get(rel_bytes + part_bytes + m_bytes, &scr);
    if (rc) return rc;
    int64_t *rel = static_cast<int64_t *>(scr), *part = rel + rel_bytes / 8;
    int32_t *mcount = reinterpret_cast<int32_t *>(part + n_parts);
    hipLaunchKernelGGL(k13_measure_kernel, dim3((unsigned)ceil_div(n_rows, (int64_t)K13_BLOCK)), dim3(K13_BLOCK), 0, st, xy, pt_off,
                       row_off, sel, width, height, class_id, n_rows, n_polys, n_points, text_off, flag, action, rel, mcount);
    k13_scan_inclusive(text_off + 1, n_rows, part, st);
    int64_t total = 0;
    if ((rc = read_totals("K13", "the measure step", {{&total, text_off + n_rows}}, st))) return rc;
    if (total_out) *total_out = total;
    if (total == 0 || (rc = text.get(total)) || !text.p) return rc;
    const TextWindows tw = text_windows(text.p, total, K13_WINDOW);
    DevBuf d_tiles;
    if ((rc = d_tiles.alloc(16 * (size_t)tw.count, st))) return rc;
    hipLaunchKernelGGL(k13_tile_rows_kernel, dim3((unsigned)ceil_div(tw.count, (int64_t)K13_BLOCK)), dim3(K13_BLOCK), 0, st, text_off,
                       n_rows, total, tw.phase, tw.count, d_tiles.as<int64_t>());
    hipLaunchKernelGGL(k13_print_kernel, dim3((unsigned)tw.count), dim3(K13_BLOCK), 0, st, xy, pt_off, row_off, width, height,
                       class_id, n_polys, n_points, text_off, flag, action, rel, mcount, d_tiles.as<int64_t>(), total, tw.phase,
                       text.as<uint8_t>());
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_yolo_seg_lines_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                           const double *width, const double *height, const int32_t *class_id, int64_t n_rows, int64_t n_polys,
                           int64_t n_points, int64_t *out_text_off, uint8_t *out_flag, uint8_t *out_action,
                           uint8_t *out_text_or_null, int64_t text_cap, int64_t *out_total, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && text_cap >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31) && n_rows < (1LL << 40), "size too large");
    DYD_REQUIRE(out_text_off, "null pointer");
    hipStream_t st = pick_stream(stream);
    if (n_rows == 0) {
        DYD_HIP(hipMemsetAsync(out_text_off, 0, 8, st));
        if (out_total) *out_total = 0;
        return DYD_OK;
    }
    DYD_REQUIRE(row_off && width && height && class_id && out_flag, "null pointer");
    DYD_REQUIRE(n_polys == 0 || (pt_off && out_action), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    SizedOut text(K13_TEXT, out_text_or_null, text_cap);
    return seg_launch(xy, pt_off, row_off, sel_or_null, width, height, class_id, n_rows, n_polys, n_points, out_text_off, out_flag,
                      out_action, text, out_total, st);
}

int dyd_yolo_seg_lines(const double *xy, const int32_t *pt_off, const int32_t *row_off, const uint8_t *sel_or_null,
                       const double *width, const double *height, const int32_t *class_id, int64_t n_rows, int64_t *out_text_off,
                       uint8_t *out_flag, uint8_t *out_action, uint8_t **out_text, int64_t *out_text_len) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(out_text_off && out_text && out_text_len, "null pointer");
    *out_text = nullptr;
    *out_text_len = 0;
    out_text_off[0] = 0;
    if (n_rows == 0) return DYD_OK;
    int64_t n_polys = 0, n_points = 0;
    int rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, class_id && out_flag, out_action, nullptr, 0, &n_polys,
                              &n_points);
    if (rc) return rc;
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_sel, d_cid, d_toff, d_flag, d_act;
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, n_polys, n_points)) ||
        (rc = poly_column(d_sel, sel_or_null, (size_t)n_polys)) || (rc = poly_column(d_cid, class_id, 4 * (size_t)n_rows)) ||
        (rc = d_toff.alloc(8 * (size_t)(n_rows + 1))) || (rc = d_flag.alloc((size_t)n_rows)) || (rc = d_act.alloc((size_t)n_polys)))
        return rc;
    const uint8_t *sel = sel_or_null ? d_sel.as<uint8_t>() : nullptr;
    SizedOut text(K13_TEXT, st);
    int64_t total = 0;
    KernelTimer timer(st);
    rc = seg_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), sel, t.w.as<double>(), t.h.as<double>(),
                    d_cid.as<int32_t>(), n_rows, n_polys, n_points, d_toff.as<int64_t>(), d_flag.as<uint8_t>(), d_act.as<uint8_t>(),
                    text, &total, st);
    if (rc) return rc;
    timer.finish();
    return hand_back_text(text.p, total,
                          {{out_text_off, d_toff.p, 8 * (size_t)(n_rows + 1)}, {out_flag, d_flag.p, (size_t)n_rows},
                           {out_action, d_act.p, (size_t)n_polys}},
                          st, out_text, out_text_len);
}

}  // extern "C"
