// k16_coco.hip — K16: COCO annotation objects from the annotation polygons (the COCO export step).
//
// One JSON object per selected polygon that K13 would write, in the form COCO's "annotations" list holds (include/dyd.h and
// DESIGN §5n have the definition):
//   {"id":A,"image_id":I,"category_id":K,"bbox":[bx,by,bw,bh],"area":a,"iscrowd":0,"segmentation":[[px0,py0,px1,...]]}
//   - the polygon's checks, its vertex list and its clip to [0, W] x [0, H] are K13's (k13_poly.h, the same code), the area is
//     K14's |shoelace sum| * 0.5 over the clipped vertices C;
//   - P = C with every coordinate clamped into the image (no -0.0, no rounding overshoot); the box is the extent of P;
//   - every number prints as "%.2f", exactly (round6.h fix2), which needs values below 2^43: a written or clipped polygon
//     whose area is not is too_large (6) and not printed;
//   - A = ann_id_base + polygon index, I = image_id_base + row index, K = cat_id (<= 0: not selected, 255);
//   - flag bit 0 clear leaves the segmentation list empty.
// The text of a call is the objects in polygon order joined with ",".
//
// Layout in HBM: xy = P x (x, y) f64 (16-B aligned), pt_off = B+1 int32, row_off = N+1 int32, cat_id = B int32, width / height =
// N f64, size_status = N u8.  Out: action = B u8, area = B f64 (NaN unless printed), row_kept = N int32, text = T bytes.
// Algorithmic bytes: 16*P + 4*(B+1) + 4*B + 4*(N+1) + 17*N in, 9*B + 4*N + T out.  Bound: HBM.
//
// Three steps, K13's, with no hand-off between workgroups inside a launch:
//   1. measure, a lane per polygon over 256-polygon tiles (K14's mapping: two lanes find the tile's first and last row, every
//      lane searches between them): k13_prepare, then one streaming pass over C gives the action, the shoelace sum, the
//      extent of P and the sum of the numbers' lengths.  It writes the action, the area, the box and the object's byte count.
//      Every printed object counts one byte more than it has, for the comma after it: the text's length is the sum less one,
//      and the last object's comma falls outside the text and is never written.  So every byte has one owner, no lane needs
//      to know whether its polygon is the first or the last printed one, and a window edge may fall before or after a comma.
//   2. k13_seg.hip's int64 scan over the polygons' byte counts (k13_scan.h), and a lane per row counts the row's printed polygons;
//   3. print, a workgroup per K16_WINDOW bytes of text: two lanes find the first and the last polygon that meet the window,
//      a lane per polygon prints the part inside it into LDS (the head from the stored box and area; the segmentation by
//      running the clip again, counting bytes up to the window and stopping at its end), and the window streams out with
//      16-byte stores.  Windows are aligned to 16 bytes of the text's address, so neighbours share no chunk.
// No kernel indexes a per-lane array at run time: no scratch.
#include "k13_poly.h"
#include "k13_scan.h"
#include "poly_table.h"
#include "round6.h"
#include "sized_out.h"
#include "text_window.h"

namespace dyd {

constexpr int K16_BLOCK = 256;
constexpr int K16_WINDOW = 32 * 1024;       // bytes of text per print workgroup (multiple of 16)
constexpr uint8_t COCO_TOO_LARGE = 6;
constexpr uint32_t COCO_SEGMENTATION = 1u;  // flags bit 0
constexpr int64_t K16_ID_LIMIT = 1LL << 53;

// the fixed text of an object: {"id": ,"image_id": ,"category_id": ,"bbox":[ , , , ],"area": ,"iscrowd":0,"segmentation":[ ]} ,
constexpr int K16_FIXED = 6 + 12 + 15 + 9 + 3 + 9 + 29 + 2 + 1;

__device__ __forceinline__ int k16_digits(uint64_t n) {   // n < 10^17
    int d = 1;
    uint64_t p = 10;
#pragma unroll
    for (int k = 1; k < 17; ++k) {
        d += n >= p ? 1 : 0;
        p *= 10;
    }
    return d;
}

// bytes of "%.2f" from fix2's integer: its digits, at least three, and the dot
__device__ __forceinline__ int k16_fix2_len(uint64_t n) { return max(k16_digits(n), 3) + 1; }

__device__ __forceinline__ double k16_clamp(double v, double hi) { return !(v > 0.0) ? 0.0 : (v > hi ? hi : v); }

// ---- 1. measure: a lane per polygon --------------------------------------------------------------------------
// poff[p + 1] = the object's bytes with its comma (0: not printed), box[4p..] = bx, by, bw, bh
__global__ __launch_bounds__(K16_BLOCK) void k16_measure_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                                const int32_t *__restrict__ row_off,
                                                                const int32_t *__restrict__ cat_id, const double *__restrict__ width,
                                                                const double *__restrict__ height,
                                                                const uint8_t *__restrict__ size_status, int64_t n_rows,
                                                                int64_t n_polys, int64_t n_points, int64_t image_id_base,
                                                                int64_t ann_id_base, uint32_t flags, uint8_t *__restrict__ out_action,
                                                                double *__restrict__ out_area, int64_t *__restrict__ poff,
                                                                double *__restrict__ box) {
    __shared__ int32_t rows[2];
    const int64_t p0 = (int64_t)blockIdx.x * K16_BLOCK;
    poly_tile_rows(row_off, n_rows, p0, min(p0 + K16_BLOCK, n_polys), rows);
    const int64_t p = p0 + threadIdx.x;
    if (p >= n_polys) return;
    if (p == 0) poff[0] = 0;
    const int32_t cat = cat_id[p];
    uint8_t act = SEG_UNSELECTED;
    double area = __builtin_nan("");
    int64_t bytes = 0;
    if (cat > 0) {
        const int64_t r = last_le(row_off, rows[0], rows[1], p);
        const double W = width[r], H = height[r];
        if (size_status[r] != 0 || !k13_size_ok(W) || !k13_size_ok(H)) {
            act = SEG_NO_SIZE;
        } else {
            const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);   // as K13
            Poly pg;
            act = k13_prepare(xy, a, b, pg);
            if (act == 0xff) {
                const bool clip = k13_outside(pg, W, H);
                const bool seg = flags & COCO_SEGMENTATION;
                int64_t nlen = 0;              // bytes of the segmentation's numbers
                ClipWalk w;
                double plx = 0.0, ply = 0.0, phx = 0.0, phy = 0.0;   // the extent of P
                auto walk = [&](double x, double y) {
                    const double cx = k16_clamp(x, W), cy = k16_clamp(y, H);
                    if (w.m == 0) { plx = phx = cx; ply = phy = cy; }
                    plx = fmin(plx, cx); phx = fmax(phx, cx);
                    ply = fmin(ply, cy); phy = fmax(phy, cy);
                    if (seg) nlen += k16_fix2_len(fix2(cx)) + k16_fix2_len(fix2(cy));
                    w.add(x, y);
                    return true;
                };
                k13_vertices(pg, clip, W, H, walk);
                if (w.empty()) {
                    act = SEG_EMPTY;
                } else {
                    const double ar = w.area();
                    if (!(ar < K13_LIMIT)) {
                        act = COCO_TOO_LARGE;
                    } else {
                        act = clip ? SEG_CLIPPED : SEG_WRITTEN;
                        area = ar;
                        const double bw = phx - plx, bh = phy - ply;
                        box[4 * p] = plx; box[4 * p + 1] = ply; box[4 * p + 2] = bw; box[4 * p + 3] = bh;
                        bytes = K16_FIXED + k16_digits((uint64_t)(ann_id_base + p)) + k16_digits((uint64_t)(image_id_base + r)) +
                                k16_digits((uint64_t)cat) + k16_fix2_len(fix2(plx)) + k16_fix2_len(fix2(ply)) +
                                k16_fix2_len(fix2(bw)) + k16_fix2_len(fix2(bh)) + k16_fix2_len(fix2(ar));
                        if (seg) bytes += 2 + nlen + (2 * (int64_t)w.m - 1);
                    }
                }
            }
        }
    }
    out_action[p] = act;
    out_area[p] = area;
    poff[p + 1] = bytes;
}

// ---- 2b. the printed polygons per row: a lane per row ---------------------------------------------------------
__global__ __launch_bounds__(K16_BLOCK) void k16_row_kept_kernel(const int32_t *__restrict__ row_off, const uint8_t *__restrict__ action,
                                                                 int64_t n_rows, int64_t n_polys, int32_t *__restrict__ out_row_kept) {
    const int64_t i = (int64_t)blockIdx.x * K16_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t p0 = max((int64_t)row_off[i], (int64_t)0), p1 = min((int64_t)row_off[i + 1], n_polys);
    int32_t kept = 0;
    for (int64_t p = p0; p < p1; ++p) kept += action[p] <= SEG_CLIPPED ? 1 : 0;
    out_row_kept[i] = kept;
}

// ---- 3. print ------------------------------------------------------------------------------------------------
// what a print lane writes through: text position `at`, bytes outside the window [wlo, whi) dropped
struct K16Out : TextWindow {
    int64_t at;

    __device__ __forceinline__ bool meets(int64_t len) const { return at + len > wlo && at < whi; }
    __device__ __forceinline__ void ch(uint8_t c) {
        put(at, c);
        ++at;
    }
    template <int N>
    __device__ __forceinline__ void lit(const char (&s)[N]) {
        if (meets(N - 1)) {
#pragma unroll
            for (int k = 0; k < N - 1; ++k) put(at + k, (uint8_t)s[k]);
        }
        at += N - 1;
    }
    // n in d decimal digits at [a, a + d)
    __device__ __forceinline__ void digits(int64_t a, uint64_t n, int d) const {
        int k = d - 1;
        for (; n >> 32; --k) {
            const uint64_t q = n / 10u;
            put(a + k, (uint8_t)('0' + (uint32_t)(n - q * 10u)));
            n = q;
        }
        uint32_t v = (uint32_t)n;
        for (; k >= 0; --k) {
            const uint32_t q = v / 10u;
            put(a + k, (uint8_t)('0' + (v - q * 10u)));
            v = q;
        }
    }
    __device__ __forceinline__ void integer(uint64_t n) {
        const int d = k16_digits(n);
        if (meets(d)) digits(at, n, d);
        at += d;
    }
    // "%.2f" of v
    __device__ __forceinline__ void num(double v) {
        const uint64_t n = fix2(v);
        const int len = k16_fix2_len(n);
        if (meets(len)) {
            const uint64_t q = n / 100u;
            const uint32_t r = (uint32_t)(n - q * 100u), r10 = r / 10u;
            put(at + len - 1, (uint8_t)('0' + (r - r10 * 10u)));
            put(at + len - 2, (uint8_t)('0' + r10));
            put(at + len - 3, '.');
            digits(at, q, len - 3);
        }
        at += len;
    }
};

__global__ __launch_bounds__(K16_BLOCK) void k16_print_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                              const int32_t *__restrict__ row_off, const int32_t *__restrict__ cat_id,
                                                              const double *__restrict__ width, const double *__restrict__ height,
                                                              int64_t n_rows, int64_t n_polys, int64_t n_points, int64_t image_id_base,
                                                              int64_t ann_id_base, uint32_t flags, const double *__restrict__ area,
                                                              const int64_t *__restrict__ poff, const double *__restrict__ box,
                                                              int64_t total, int64_t phase, uint8_t *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint8_t img[K16_WINDOW];
    __shared__ int64_t ends[4];                // first and last polygon of the window, and their rows
    const TextWindow win = text_window(img, blockIdx.x, K16_WINDOW, phase, total);
    const int64_t wlo = win.wlo, whi = win.whi;
    if (threadIdx.x < 2) {
        // poff[n_polys] = total + 1 > whi - 1, so both answers are polygons
        const int64_t q = last_le(poff, 0, n_polys, threadIdx.x == 0 ? wlo : whi - 1);
        ends[threadIdx.x] = q;
        ends[2 + threadIdx.x] = last_le(row_off, 0, n_rows - 1, q);
    }
    __syncthreads();
    const int64_t q0 = ends[0], q1 = ends[1], ra = ends[2], rb = ends[3];
    for (int64_t p = q0 + threadIdx.x; p <= q1; p += K16_BLOCK) {
        const int64_t start = poff[p], end = poff[p + 1];
        if (end == start || end <= wlo || start >= whi) continue;
        const int64_t r = last_le(row_off, ra, rb, p);
        K16Out o{win, start};
        o.lit("{\"id\":");
        o.integer((uint64_t)(ann_id_base + p));
        o.lit(",\"image_id\":");
        o.integer((uint64_t)(image_id_base + r));
        o.lit(",\"category_id\":");
        o.integer((uint64_t)cat_id[p]);
        o.lit(",\"bbox\":[");
        o.num(box[4 * p]);
        o.ch(',');
        o.num(box[4 * p + 1]);
        o.ch(',');
        o.num(box[4 * p + 2]);
        o.ch(',');
        o.num(box[4 * p + 3]);
        o.lit("],\"area\":");
        o.num(area[p]);
        o.lit(",\"iscrowd\":0,\"segmentation\":[");
        if ((flags & COCO_SEGMENTATION) && o.at < whi) {
            const double W = width[r], H = height[r];
            const int32_t a = max(pt_off[p], 0), b = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
            Poly pg;
            (void)k13_prepare(xy, a, b, pg);
            o.ch('[');
            bool first = true;
            auto vertex = [&](double x, double y) {
                if (!first) o.ch(',');
                first = false;
                o.num(k16_clamp(x, W));
                o.ch(',');
                o.num(k16_clamp(y, H));
                return o.at < whi;
            };
            k13_vertices(pg, k13_outside(pg, W, H), W, H, vertex);
            // stopped early: the rest lies past the window, and so does what follows
        }
        // the object's last three bytes, from its end: a lane that stopped early does not know where its list closes
        if (flags & COCO_SEGMENTATION) o.put(end - 4, ']');
        o.put(end - 3, ']');
        o.put(end - 2, '}');
        o.put(end - 1, ',');
    }
    __syncthreads();
    win.flush<K16_WINDOW, K16_BLOCK>(text);
}


constexpr SizedName K16_TEXT{"K16", "text", "bytes", 1};

// Measure, scan and print on device pointers.  `text` is asked for the buffer once the size is known (none: measure only);
// *total_out is a host value.
static int coco_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cat_id, const double *width,
                       const double *height, const uint8_t *size_status, int64_t n_rows, int64_t n_polys, int64_t n_points,
                       int64_t image_id_base, int64_t ann_id_base, uint32_t flags, uint8_t *out_action, double *out_area,
                       int32_t *out_row_kept, SizedOut &text, int64_t *total_out, hipStream_t st) {
    *total_out = 0;
    if (n_rows == 0) return DYD_OK;
    if (n_polys == 0) {
        DYD_HIP(hipMemsetAsync(out_row_kept, 0, 4 * (size_t)n_rows, st));
        return DYD_OK;
    }
    DevBuf d_poff, d_box, d_part;
    int rc;
    if ((rc = d_poff.alloc(8 * (size_t)(n_polys + 1), st)) || (rc = d_box.alloc(32 * (size_t)n_polys, st)) ||
        (rc = d_part.alloc(8 * (size_t)k13_scan_parts(n_polys), st)))
        return rc;
    int64_t *poff = d_poff.as<int64_t>();
    hipLaunchKernelGGL(k16_measure_kernel, dim3((unsigned)ceil_div(n_polys, (int64_t)K16_BLOCK)), dim3(K16_BLOCK), 0, st, xy, pt_off,
                       row_off, cat_id, width, height, size_status, n_rows, n_polys, n_points, image_id_base, ann_id_base, flags,
                       out_action, out_area, poff, d_box.as<double>());
    k13_scan_inclusive(poff + 1, n_polys, d_part.as<int64_t>(), st);
    hipLaunchKernelGGL(k16_row_kept_kernel, dim3((unsigned)ceil_div(n_rows, (int64_t)K16_BLOCK)), dim3(K16_BLOCK), 0, st, row_off,
                       out_action, n_rows, n_polys, out_row_kept);
    int64_t sum = 0;
    if ((rc = read_totals("K16", "the measure step", {{&sum, poff + n_polys}}, st))) return rc;
    const int64_t total = sum > 0 ? sum - 1 : 0;   // the last object's comma is not part of the text
    *total_out = total;
    if (total == 0 || (rc = text.get(total)) || !text.p) return rc;
    const TextWindows tw = text_windows(text.p, total, K16_WINDOW);
    hipLaunchKernelGGL(k16_print_kernel, dim3((unsigned)tw.count), dim3(K16_BLOCK), 0, st, xy, pt_off, row_off, cat_id, width, height,
                       n_rows, n_polys, n_points, image_id_base, ann_id_base, flags, out_area, poff, d_box.as<double>(), total,
                       tw.phase, text.as<uint8_t>());
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_coco_annotations_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cat_id,
                             const double *width, const double *height, const uint8_t *size_status, int64_t n_rows, int64_t n_polys,
                             int64_t n_points, int64_t image_id_base, int64_t ann_id_base, uint32_t flags, uint8_t *out_action,
                             double *out_area, int32_t *out_row_kept, uint8_t *out_text_or_null, int64_t text_cap, int64_t *out_total,
                             void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && text_cap >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31) && n_rows < (1LL << 31), "size exceeds int32 offsets");
    DYD_REQUIRE(image_id_base >= 0 && ann_id_base >= 0, "negative id base");
    DYD_REQUIRE(image_id_base < K16_ID_LIMIT - n_rows && ann_id_base < K16_ID_LIMIT - n_polys, "ids reach 2^53");
    DYD_REQUIRE(n_rows == 0 || (row_off && width && height && size_status && out_row_kept), "null pointer");
    DYD_REQUIRE(n_polys == 0 || (n_rows > 0 && pt_off && cat_id && out_action && out_area), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(xy) & 15) == 0, "xy must be 16-byte aligned");
    SizedOut text(K16_TEXT, out_text_or_null, text_cap);
    int64_t total = 0;
    const int rc = coco_launch(xy, pt_off, row_off, cat_id, width, height, size_status, n_rows, n_polys, n_points, image_id_base,
                               ann_id_base, flags, out_action, out_area, out_row_kept, text, &total, pick_stream(stream));
    if (out_total && (rc == DYD_OK || rc == DYD_ERR_RANGE)) *out_total = total;
    return rc;
}

int dyd_coco_annotations(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *cat_id, const double *width,
                         const double *height, const uint8_t *size_status, int64_t n_rows, int64_t image_id_base, int64_t ann_id_base,
                         uint32_t flags, uint8_t *out_action, double *out_area, int32_t *out_row_kept, uint8_t **out_text,
                         int64_t *out_text_len) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31), "size exceeds int32 offsets");
    DYD_REQUIRE(out_text && out_text_len, "null pointer");
    *out_text = nullptr;
    *out_text_len = 0;
    DYD_REQUIRE(image_id_base >= 0 && ann_id_base >= 0, "negative id base");
    int64_t nb = 0, np = 0;
    int rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, size_status && out_row_kept,
                              cat_id && out_action && out_area, nullptr, 0, &nb, &np);
    if (rc) return rc;
    DYD_REQUIRE(image_id_base < K16_ID_LIMIT - n_rows && ann_id_base < K16_ID_LIMIT - nb, "ids reach 2^53");
    if (n_rows == 0) return DYD_OK;
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_cat, d_st, d_act, d_area, d_kept;
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, nb, np)) || (rc = poly_column(d_cat, cat_id, 4 * (size_t)nb)) ||
        (rc = poly_column(d_st, size_status, (size_t)n_rows)) || (rc = d_act.alloc((size_t)nb)) ||
        (rc = d_area.alloc(8 * (size_t)nb)) || (rc = d_kept.alloc(4 * (size_t)n_rows)))
        return rc;
    SizedOut text(K16_TEXT, st);
    int64_t total = 0;
    KernelTimer timer(st);
    rc = coco_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), d_cat.as<int32_t>(), t.w.as<double>(),
                     t.h.as<double>(), d_st.as<uint8_t>(), n_rows, nb, np, image_id_base, ann_id_base, flags, d_act.as<uint8_t>(),
                     d_area.as<double>(), d_kept.as<int32_t>(), text, &total, st);
    if (rc) return rc;
    timer.finish();
    return hand_back_text(text.p, total,
                          {{out_action, d_act.p, (size_t)nb}, {out_area, d_area.p, 8 * (size_t)nb},
                           {out_row_kept, d_kept.p, 4 * (size_t)n_rows}},
                          st, out_text, out_text_len);
}

}  // extern "C"
