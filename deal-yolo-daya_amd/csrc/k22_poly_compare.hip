// k22_poly_compare.hip — K22: two polygon tables of the same image rows compared by mask IoU.
//
// cover(p) is K21's pixel set (centre sampling, canonical edge direction, even-odd rule; include/dyd.h has the rule, DESIGN §5t
// the mapping and its cost).  Per pair of polygons of a row the kernel counts |cover(a) & cover(b)|, per polygon |cover(p)|; K18's
// greedy matching then runs on the quotient of those integers, and the pixel confusion matrix comes out of the same pass.  The
// polygon code is K13's (k13_scan_inclusive, last_le); the pixel rule is K21's own, from k21_cover.h: the row rule, the polygon
// kernel (k21_polys, defined in k21_raster.hip), the polygons of a row, the box cull and the edge -> crossing list -> parity
// step.  The greedy matcher's keys and confusion count are K18's, from k18_pick.h.
//
// Layout in HBM, per table: xy = P x (x, y) f64, pt_off = B+1 int32, row_off = N+1 int32, cls = B int32; width / height = N f64.
// Scratch: 32 bytes per polygon (its box), the rows' item offsets, the scan's partial sums; the pair counts (u32 per pair of a
// compared row) in the caller's buffer or one of the library's.
//
// Steps (no hand-off between workgroups inside a launch):
//   1. rows, a lane per row: status, item count and pair count; two scans give item_off and pair_off; the host reads both totals;
//   2. polygons of either side, a lane per polygon: the action and the bounding box;
//   3. paint, a wave (one workgroup) per item = (row, scanline, strip of `strip` columns), items taken grid-stride.  A polygon's
//      coverage of the strip is a bitmap of one u64 word per 64 pixels, straight from __ballot(parity); the parity of a lane's
//      pixels (pixel 64 c + lane is bit c) lives in a register.  The B polygons that pass K21's box cull are taken in chunks of
//      `chunk` bitmaps; for each chunk every A polygon that passes the cull gets its bitmap, and lane j adds
//      popcount(wordA & wordB_j) over the strip's words to the pair cell (one u32 atomic when not zero).  Ownership (the last
//      polygon in table order) and the pixel counts are taken when a bitmap is built: B's with its chunk, A's on the first chunk.
//      At the end of the item the owners give (class A, class B) per pixel; the wave counts each distinct pair of classes of
//      the strip once and adds it with one u64 atomic.  Integer atomics only: no result depends on the schedule;
//   4. match, a wave per row: K18's big-row scheme.  Lanes stride over the A polygons, the B polygons are taken in order, the
//      arg-max (largest IoU, then lowest index) by shuffles; the matched state is out_a_match, which only the owning lane touches.
// Steps 1 to 3 are also K25's pair step (k25_poly_eval.hip, through compare_pairs_launch of k22_pairs.h), with the paint kernel
// in its evaluation flavour (the template argument), which keeps no owners and counts no pixel classes.
#include "k13_scan.h"
#include "k18_pick.h"
#include "k21_cover.h"
#include "k22_pairs.h"
#include "poly_table.h"

namespace dyd {

constexpr int K22_BLOCK = 256;
constexpr int K22_STRIP = 1024;              // columns per item (default and most): 16 words per bitmap
constexpr int K22_WORDS = K22_STRIP / kWave;
constexpr int K22_CROSSINGS = 256;           // capacity of the crossing list (default and most)
constexpr int K22_CHUNK = 32;                // B bitmaps held at a time (default and most); at most one per lane
constexpr int K22_PITCH = K22_WORDS + 1;     // words per stored B bitmap: lanes j and j + 1 on different banks
constexpr int64_t K22_MAX_PIXELS = 1LL << 30;
constexpr int64_t K22_MAX_PAIRS = 1LL << 24;
constexpr int64_t K22_MAX_GRID = 1 << 20;    // paint workgroups; the items beyond are taken grid-stride

// ---- 1. rows: a lane per row -----------------------------------------------------------------------------------
__global__ __launch_bounds__(K22_BLOCK) void k22_rows_kernel(const double *__restrict__ width, const double *__restrict__ height,
                                                             const int32_t *__restrict__ a_row_off, const int32_t *__restrict__ b_row_off,
                                                             int64_t n_rows, int64_t n_a, int64_t n_b, int64_t max_pixels,
                                                             int64_t max_pairs, int strip, uint8_t *__restrict__ row_status,
                                                             int64_t *__restrict__ pair_off, int64_t *__restrict__ item_off) {
    const int64_t i = (int64_t)blockIdx.x * K22_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    int64_t w, h, a0, a1, b0, b1;
    uint8_t st = k21_row_size(width[i], height[i], max_pixels, &w, &h);
    k21_row_polys(a_row_off, i, n_a, &a0, &a1);
    k21_row_polys(b_row_off, i, n_b, &b0, &b1);
    const int64_t pairs = (a1 - a0) * (b1 - b0);   // both counts stay below 2^31
    if (st == 0 && pairs > max_pairs) st = CMP_ROW_PAIRS;
    row_status[i] = st;
    pair_off[i + 1] = st == 0 ? pairs : 0;
    item_off[i + 1] = st == 0 ? h * ((w + strip - 1) / strip) : 0;
    if (i == 0) pair_off[0] = item_off[0] = 0;
}

// ---- 2. polygons: K21's kernel, launched through k21_polys (k21_cover.h), once per table ----------------------------

// ---- 3. paint and intersect: a wave per item -------------------------------------------------------------------
// one side of the comparison as the paint kernel reads it
struct K22Side {
    const double *xy;
    const int32_t *pt_off, *row_off, *cls;
    const uint8_t *action;
    const double *info;
    unsigned long long *pixels;
    int64_t n_polys, n_points;
};

// The bitmap of polygon p over the strip: words[c] bit l = pixel 64 c + l covered, for c < n_words; -> the number of covered
// pixels.  *par_out: the lane's own pixels, bit c = pixel 64 c + lane.
__device__ __forceinline__ int k22_bitmap(const K22Side &t, int64_t p, const K21Strip &s, int cap, double *list,
                                          unsigned long long *words, uint32_t *par_out) {
    const int lane = threadIdx.x;
    const int32_t a = max(t.pt_off[p], 0), b = (int32_t)min((int64_t)max(t.pt_off[p + 1], a), t.n_points);
    uint32_t par = 0;
    // the crossings listed so far, XORed into the parity of the lane's pixels
    auto apply = [&](int n_listed) __attribute__((always_inline)) {
        __syncthreads();
        for (int c = 0; c < s.n_words; ++c) {
            const double xc = (double)(s.x0 + c * kWave + lane) + 0.5;
            uint32_t bit = 0;
            for (int k = 0; k < n_listed; ++k) bit ^= (uint32_t)(list[k] > xc);
            par ^= bit << c;
        }
        __syncthreads();
    };
    k21_edges(reinterpret_cast<const double2 *>(t.xy) + a, b - a, t.info + 4 * p, s.yc, cap, list, apply);
    int n_covered = 0;
    for (int c = 0; c < s.n_words; ++c) {
        const bool in = ((par >> c) & 1u) != 0 && c * kWave + lane < s.npx;
        const unsigned long long w = __ballot(in);
        if (!in) par &= ~(1u << c);
        if (lane == 0) words[c] = w;
        n_covered += __popcll(w);
    }
    __syncthreads();
    *par_out = par;
    return n_covered;
}

// EVAL: the flavour of K25 (scored evaluation), which needs the pair cells of equal classes and the pixel counts only: no
// owners, no class-pair pass, no row_pixels; a pair of different classes is neither intersected nor added.
template <bool EVAL>
__global__ __launch_bounds__(kWave) void k22_paint_kernel(K22Side A, K22Side B, const double *__restrict__ width,
                                                          const double *__restrict__ height, int64_t n_rows, int32_t C, int strip,
                                                          int cap, int chunk, const uint8_t *__restrict__ row_status,
                                                          const int64_t *__restrict__ pair_off, const int64_t *__restrict__ item_off,
                                                          int64_t n_items, int64_t pair_total, uint32_t *__restrict__ pairs,
                                                          unsigned long long *__restrict__ pixel_conf,
                                                          unsigned long long *__restrict__ row_pixels) {
    __shared__ int32_t owner_a[EVAL ? 1 : K22_STRIP];   // polygon index, then the pixel's class pair
    __shared__ int32_t owner_b[EVAL ? 1 : K22_STRIP];
    __shared__ double list[K22_CROSSINGS];
    __shared__ unsigned long long bits_b[K22_CHUNK * K22_PITCH];
    __shared__ unsigned long long bits_a[K22_WORDS];
    __shared__ int32_t idx_b[K22_CHUNK];
    __shared__ int32_t cls_b[EVAL ? K22_CHUNK : 1];
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t r = last_le(item_off, 0, n_rows - 1, item);
        const int64_t local = item - item_off[r];
        const int64_t W = (int64_t)width[r], H = (int64_t)height[r];
        const int64_t n_strips = (W + strip - 1) / strip;
        if (row_status[r] != 0 || local < 0 || local >= H * n_strips) continue;   // never for a sound item_off
        const int64_t j = local / n_strips, x0 = (local - j * n_strips) * strip;
        const int npx = (int)min((int64_t)strip, W - x0);   // at most K22_WORDS words: strip <= K22_STRIP
        const K21Strip s{(double)j + 0.5, (double)x0 + 0.5, (double)(x0 + npx - 1) + 0.5, x0, npx, (npx + kWave - 1) / kWave};
        if constexpr (!EVAL)
            for (int px = lane; px < s.npx; px += kWave) owner_a[px] = owner_b[px] = -1;
        int64_t a0, a1, b0, b1;
        k21_row_polys(A.row_off, r, A.n_polys, &a0, &a1);
        k21_row_polys(B.row_off, r, B.n_polys, &b0, &b1);
        const int64_t nb = b1 - b0, cell0 = pair_off[r];
        int64_t q = b0;
        for (bool first = true;; first = false) {
            // the next chunk of B bitmaps; B's ownership and pixel counts
            int n_chunk = 0;
            for (; q < b1 && n_chunk < chunk; ++q) {
                if (!k21_reaches(B.action, B.info, q, s)) continue;
                uint32_t par;
                const int n_cov = k22_bitmap(B, q, s, cap, list, bits_b + n_chunk * K22_PITCH, &par);
                if constexpr (!EVAL)
                    for (int c = 0; c < s.n_words; ++c)
                        if ((par >> c) & 1u) owner_b[c * kWave + lane] = (int32_t)q;
                if (lane == 0) {
                    idx_b[n_chunk] = (int32_t)(q - b0);
                    if constexpr (EVAL) cls_b[n_chunk] = B.cls[q];
                    if (n_cov > 0) atomicAdd(B.pixels + q, (unsigned long long)n_cov);
                }
                ++n_chunk;
            }
            if (n_chunk == 0 && !first) break;
            __syncthreads();
            for (int64_t p = a0; p < a1; ++p) {
                if (!k21_reaches(A.action, A.info, p, s)) continue;
                uint32_t par;
                const int n_cov = k22_bitmap(A, p, s, cap, list, bits_a, &par);
                if (first) {
                    if constexpr (!EVAL)
                        for (int c = 0; c < s.n_words; ++c)
                            if ((par >> c) & 1u) owner_a[c * kWave + lane] = (int32_t)p;
                    if (lane == 0 && n_cov > 0) atomicAdd(A.pixels + p, (unsigned long long)n_cov);
                }
                bool mine = lane < n_chunk && n_cov > 0;
                if constexpr (EVAL) mine = mine && cls_b[lane] == A.cls[p];
                if (mine) {
                    const unsigned long long *wb = bits_b + lane * K22_PITCH;
                    unsigned int sum = 0;
                    for (int c = 0; c < s.n_words; ++c) sum += (unsigned int)__popcll(bits_a[c] & wb[c]);
                    const int64_t cell = cell0 + (p - a0) * nb + idx_b[lane];
                    if (sum != 0 && cell < pair_total) atomicAdd(pairs + cell, sum);   // always inside for a sound pair_off
                }
                __syncthreads();   // bits_a is written again by the next polygon
            }
            if (q >= b1) break;
        }
        if constexpr (EVAL) continue;   // the chunk loop ends behind a barrier or without a bitmap since the last one
        // owners -> class pairs, kept in owner_a; the row's two pixel counts
        const int32_t stride = C + 1;
        uint32_t rem = 0;
        int n_agree = 0, n_fg = 0;
        for (int c = 0; c < s.n_words; ++c) {
            const int px = c * kWave + lane;
            bool agree = false, fg = false;
            if (px < s.npx) {
                const int32_t oa = owner_a[px], ob = owner_b[px];
                const int32_t ca = oa < 0 ? C : A.cls[oa], cb = ob < 0 ? C : B.cls[ob];
                agree = oa >= 0 && ob >= 0 && ca == cb;
                fg = oa >= 0 || ob >= 0;
                if ((uint32_t)ca <= (uint32_t)C && (uint32_t)cb <= (uint32_t)C) {   // a class id outside the list is not counted
                    owner_a[px] = ca * stride + cb;
                    rem |= 1u << c;
                }
            }
            n_agree += __popcll(__ballot(agree));
            n_fg += __popcll(__ballot(fg));
        }
        if (lane == 0 && n_agree > 0) atomicAdd(row_pixels + 2 * r, (unsigned long long)n_agree);
        if (lane == 0 && n_fg > 0) atomicAdd(row_pixels + 2 * r + 1, (unsigned long long)n_fg);
        // one atomic per distinct class pair of the strip: the first lane with pixels left names a pair, every lane hands in
        // its pixels of that pair.  The leader's first pixel leaves in every round, so the loop ends.
        for (;;) {
            const unsigned long long any = __ballot(rem != 0);
            if (!any) break;
            const int leader = __ffsll((long long)any) - 1;
            const int32_t mine = rem ? owner_a[(__ffs((int)rem) - 1) * kWave + lane] : 0;
            const int32_t key = __shfl(mine, leader);
            int n = 0;
            for (int c = 0; c < s.n_words; ++c) {
                const bool hit = ((rem >> c) & 1u) != 0 && owner_a[c * kWave + lane] == key;
                n += __popcll(__ballot(hit));
                if (hit) rem &= ~(1u << c);
            }
            if (lane == leader) atomicAdd(pixel_conf + key, (unsigned long long)n);
        }
        __syncthreads();   // the owners are written again by the next item
    }
}

// ---- 4. match: a wave per row ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void k22_match_kernel(const int32_t *__restrict__ a_row_off, const int32_t *__restrict__ a_cls,
                                                          const uint8_t *__restrict__ a_action, const unsigned long long *__restrict__ a_pixels,
                                                          const int32_t *__restrict__ b_row_off, const int32_t *__restrict__ b_cls,
                                                          const uint8_t *__restrict__ b_action, const unsigned long long *__restrict__ b_pixels,
                                                          int64_t n_rows, int64_t n_a, int64_t n_b, int32_t C, double thr, int by_label,
                                                          const uint8_t *__restrict__ row_status, const int64_t *__restrict__ pair_off,
                                                          const uint32_t *__restrict__ pairs, int32_t *out_a_match,
                                                          int32_t *__restrict__ out_b_match, double *__restrict__ out_b_iou,
                                                          double *out_a_best, double *__restrict__ out_b_best,
                                                          int32_t *__restrict__ out_rows, unsigned long long *__restrict__ conf) {
    const int lane = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        int64_t a0, a1, b0, b1;
        k21_row_polys(a_row_off, r, n_a, &a0, &a1);
        k21_row_polys(b_row_off, r, n_b, &b0, &b1);
        const int64_t na = a1 - a0, nb = b1 - b0;
        for (int64_t i = lane; i < na; i += kWave) {
            out_a_match[a0 + i] = -1;
            out_a_best[a0 + i] = 0.0;
        }
        int same = 0, diff = 0, a_live = 0, b_live = 0;
        const bool compared = row_status[r] == 0;
        const int64_t cell0 = pair_off[r];
        for (int64_t j = 0; j < nb; ++j) {   // wave-uniform
            const bool b_ok = compared && b_action[b0 + j] == COVER_DONE;
            unsigned long long key = 0ull, bk = 0ull;
            int64_t idx = INT64_MAX;
            if (b_ok) {
                ++b_live;
                const int32_t cb = b_cls[b0 + j];
                const unsigned long long pb = b_pixels[b0 + j];
                for (int64_t i = lane; i < na; i += kWave) {   // ascending: the first of equal keys stays
                    if (a_action[a0 + i] != COVER_DONE) continue;
                    const uint32_t inter = pairs[cell0 + i * nb + j];
                    if (inter == 0) continue;
                    const double iou = (double)inter / (double)(a_pixels[a0 + i] + pb - inter);
                    if (iou > out_a_best[a0 + i]) out_a_best[a0 + i] = iou;
                    const unsigned long long bits = k18_bits(iou), cand = k18_cand_key(iou);   // iou > 0: ordered like its bits
                    bk = bits > bk ? bits : bk;
                    if (out_a_match[a0 + i] < 0 && (!by_label || a_cls[a0 + i] == cb) && iou >= thr && cand > key) {
                        key = cand;
                        idx = i;
                    }
                }
            }
            unsigned long long wk = key, wb = bk;
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long oc = __shfl_xor(wk, d), ob = __shfl_xor(wb, d);
                wk = oc > wk ? oc : wk;
                wb = ob > wb ? ob : wb;
            }
            int64_t wi = key == wk && key != 0ull ? idx : INT64_MAX;
            for (int d = 32; d >= 1; d >>= 1) {
                const int64_t oi = __shfl_xor(wi, d);
                wi = oi < wi ? oi : wi;
            }
            const bool hit = wk != 0ull;
            if (hit && wi % kWave == lane) {   // the owner of the matched A polygon
                out_a_match[a0 + wi] = (int32_t)j;
                const int32_t ca = a_cls[a0 + wi], cb = b_cls[b0 + j];
                if (ca == cb) ++same; else ++diff;
                k18_count(conf, C, ca, cb);
            }
            if (lane == 0) {
                out_b_match[b0 + j] = hit ? (int32_t)wi : -1;
                out_b_iou[b0 + j] = hit ? k18_value(wk - 1ull) : 0.0;
                out_b_best[b0 + j] = k18_value(wb);
                if (b_ok && !hit) k18_count(conf, C, C, b_cls[b0 + j]);
            }
        }
        if (compared)
            for (int64_t i = lane; i < na; i += kWave)
                if (a_action[a0 + i] == COVER_DONE) {
                    ++a_live;
                    if (out_a_match[a0 + i] < 0) k18_count(conf, C, a_cls[a0 + i], C);
                }
        for (int d = 32; d >= 1; d >>= 1) {
            same += __shfl_xor(same, d);
            diff += __shfl_xor(diff, d);
            a_live += __shfl_xor(a_live, d);
        }
        if (lane == 0) {
            int32_t *o = out_rows + 4 * r;
            o[0] = same;
            o[1] = diff;
            o[2] = a_live - same - diff;
            o[3] = b_live - same - diff;
        }
    }
}

// dyd_set_option("k22_strip" / "k22_crossings" / "k22_chunk" / "k22_grid", n): the strip's width, the list's capacity, the B
// bitmaps per chunk and a cap on the paint workgroups; <= 0 restores the default, larger values are capped
static int g_k22_strip = K22_STRIP, g_k22_crossings = K22_CROSSINGS, g_k22_chunk = K22_CHUNK;
static int64_t g_k22_grid = K22_MAX_GRID;

void set_k22_strip(int v) { g_k22_strip = k21_capped(v, K22_STRIP); }
void set_k22_crossings(int v) { g_k22_crossings = k21_capped(v, K22_CROSSINGS); }
void set_k22_chunk(int v) { g_k22_chunk = k21_capped(v, K22_CHUNK); }
void set_k22_grid(int v) { g_k22_grid = k21_capped(v, (int)K22_MAX_GRID); }

int compare_params(int32_t n_classes, int64_t max_pixels, int64_t max_pairs) {
    DYD_REQUIRE(n_classes >= 1 && n_classes <= 1023, "n_classes must lie in 1..1023");
    DYD_REQUIRE(max_pixels >= 1 && max_pixels <= K22_MAX_PIXELS, "max_pixels_per_row must lie in 1..2^30");
    DYD_REQUIRE(max_pairs >= 1 && max_pairs <= K22_MAX_PAIRS, "max_pairs_per_row must lie in 1..2^24");
    return DYD_OK;
}

constexpr SizedName K22_PAIRS{"K22", "pair", "elements", 4};

// Steps 1 to 3 on device pointers (k22_pairs.h).
int compare_pairs_launch(const K22Table &a, const K22Table &b, const double *width, const double *height, int64_t n_rows, int32_t C,
                         int64_t max_pixels, int64_t max_pairs, const K22Out &o, bool for_eval, SizedOut &pairs_out, hipStream_t st) {
    const int strip = g_k22_strip, cap = g_k22_crossings, chunk = g_k22_chunk;
    const size_t info_a = 32 * (size_t)max(a.n_polys, (int64_t)1), info_b = 32 * (size_t)max(b.n_polys, (int64_t)1);
    ScratchLease lease(st);
    void *scr = nullptr;
    int rc = lease.get(info_a + info_b + 8 * (size_t)(n_rows + 1) + 8 * (size_t)k13_scan_parts(n_rows), &scr);
    if (rc) return rc;
    double *inf_a = static_cast<double *>(scr), *inf_b = inf_a + info_a / 8;
    int64_t *item_off = reinterpret_cast<int64_t *>(inf_b + info_b / 8), *part = item_off + n_rows + 1;
    const dim3 row_grid((unsigned)ceil_div(n_rows, (int64_t)K22_BLOCK));
    hipLaunchKernelGGL(k22_rows_kernel, row_grid, dim3(K22_BLOCK), 0, st, width, height, a.row_off, b.row_off, n_rows, a.n_polys,
                       b.n_polys, max_pixels, max_pairs, strip, o.row_status, o.pair_off, item_off);
    k13_scan_inclusive(o.pair_off + 1, n_rows, part, st);
    k13_scan_inclusive(item_off + 1, n_rows, part, st);   // after the first scan in the stream, so the partial sums are free again
    int64_t pair_total = 0, n_items = 0;
    if ((rc = read_totals("K22", "the row step", {{&pair_total, o.pair_off + n_rows}, {&n_items, item_off + n_rows}}, st)) ||
        (rc = pairs_out.get(pair_total)))
        return rc;
    uint32_t *pairs = pairs_out.as<uint32_t>();
    const size_t cells = 8 * (size_t)(C + 1) * (size_t)(C + 1);
    hipError_t e = hipSuccess;
    if (!for_eval) {
        e = hipMemsetAsync(o.confusion, 0, cells, st);
        if (e == hipSuccess) e = hipMemsetAsync(o.pixel_confusion, 0, cells, st);
        if (e == hipSuccess) e = hipMemsetAsync(o.row_pixels, 0, 16 * (size_t)n_rows, st);
    }
    if (e == hipSuccess && pair_total > 0) e = hipMemsetAsync(pairs, 0, 4 * (size_t)pair_total, st);
    if (e == hipSuccess && a.n_polys > 0) e = hipMemsetAsync(a.pixels, 0, 8 * (size_t)a.n_polys, st);
    if (e == hipSuccess && b.n_polys > 0) e = hipMemsetAsync(b.pixels, 0, 8 * (size_t)b.n_polys, st);
    if (e != hipSuccess) {
        set_error("K22: clearing the counters failed: %s", hipGetErrorString(e));
        return DYD_ERR_HIP;
    }
    k21_polys(a.xy, a.pt_off, a.row_off, a.cls, o.row_status, n_rows, a.n_polys, a.n_points, a.action, inf_a, st);
    k21_polys(b.xy, b.pt_off, b.row_off, b.cls, o.row_status, n_rows, b.n_polys, b.n_points, b.action, inf_b, st);
    unsigned long long *a_pix = reinterpret_cast<unsigned long long *>(a.pixels);
    unsigned long long *b_pix = reinterpret_cast<unsigned long long *>(b.pixels);
    if (n_items > 0) {
        const K22Side A{a.xy, a.pt_off, a.row_off, a.cls, a.action, inf_a, a_pix, a.n_polys, a.n_points};
        const K22Side B{b.xy, b.pt_off, b.row_off, b.cls, b.action, inf_b, b_pix, b.n_polys, b.n_points};
        const dim3 grid((unsigned)(n_items < g_k22_grid ? n_items : g_k22_grid));
        if (for_eval)
            hipLaunchKernelGGL(k22_paint_kernel<true>, grid, dim3(kWave), 0, st, A, B, width, height, n_rows, C, strip, cap, chunk,
                               o.row_status, o.pair_off, item_off, n_items, pair_total, pairs, (unsigned long long *)nullptr,
                               (unsigned long long *)nullptr);
        else
            hipLaunchKernelGGL(k22_paint_kernel<false>, grid, dim3(kWave), 0, st, A, B, width, height, n_rows, C, strip, cap, chunk,
                               o.row_status, o.pair_off, item_off, n_items, pair_total, pairs,
                               reinterpret_cast<unsigned long long *>(o.pixel_confusion),
                               reinterpret_cast<unsigned long long *>(o.row_pixels));
    }
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

// Steps 1 to 4 on device pointers.  `pairs` is asked for the pair buffer once its size is known; it fails before anything but
// row_status and pair_off is written.
static int compare_launch(const K22Table &a, const K22Table &b, const double *width, const double *height, int64_t n_rows,
                          int32_t C, double thr, int by_label, int64_t max_pixels, int64_t max_pairs, const K22Out &o,
                          SizedOut &pairs_out, hipStream_t st) {
    const int rc = compare_pairs_launch(a, b, width, height, n_rows, C, max_pixels, max_pairs, o, false, pairs_out, st);
    if (rc) return rc;
    const uint32_t *pairs = pairs_out.as<uint32_t>();
    const unsigned long long *a_pix = reinterpret_cast<const unsigned long long *>(a.pixels);
    const unsigned long long *b_pix = reinterpret_cast<const unsigned long long *>(b.pixels);
    unsigned long long *conf = reinterpret_cast<unsigned long long *>(o.confusion);
    const int64_t want = (int64_t)ctx().num_cu * 32;
    hipLaunchKernelGGL(k22_match_kernel, dim3((unsigned)(n_rows < want ? n_rows : want)), dim3(kWave), 0, st, a.row_off, a.cls,
                       a.action, a_pix, b.row_off, b.cls, b.action, b_pix, n_rows, a.n_polys, b.n_polys, C, thr, by_label,
                       o.row_status, o.pair_off, pairs, a.match, b.match, o.b_iou, a.best, b.best, o.row_counts, conf);
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_compare_polygons_dev(const double *a_xy, const int32_t *a_pt_off, const int32_t *a_row_off, const int32_t *a_cls,
                             const double *b_xy, const int32_t *b_pt_off, const int32_t *b_row_off, const int32_t *b_cls,
                             const double *width, const double *height, int64_t n_rows, int64_t n_a, int64_t n_a_points, int64_t n_b,
                             int64_t n_b_points, int32_t n_classes, double thr, int by_label, int64_t max_pixels_per_row,
                             int64_t max_pairs_per_row, uint8_t *out_row_status, int64_t *out_pair_off, uint8_t *out_a_action,
                             uint8_t *out_b_action, int64_t *out_a_pixels, int64_t *out_b_pixels, int32_t *out_a_match,
                             int32_t *out_b_match, double *out_b_iou, double *out_a_best, double *out_b_best,
                             int32_t *out_row_counts, uint64_t *out_confusion, uint64_t *out_pixel_confusion, int64_t *out_row_pixels,
                             uint32_t *out_pairs_or_null, int64_t pair_cap, void *stream) {
    DYD_API_ENTER();
    int rc = compare_params(n_classes, max_pixels_per_row, max_pairs_per_row);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0 && n_a >= 0 && n_b >= 0 && n_a_points >= 0 && n_b_points >= 0 && pair_cap >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31) && n_a < (1LL << 31) && n_b < (1LL << 31) && n_a_points < (1LL << 31) &&
                    n_b_points < (1LL << 31), "size too large");
    if (n_rows == 0) return DYD_OK;
    hipStream_t st = pick_stream(stream);
    DYD_REQUIRE(a_row_off && b_row_off && width && height && out_row_status && out_pair_off && out_row_counts && out_confusion &&
                    out_pixel_confusion && out_row_pixels, "null pointer");
    DYD_REQUIRE(n_a == 0 || (a_pt_off && a_cls && out_a_action && out_a_pixels && out_a_match && out_a_best), "null pointer");
    DYD_REQUIRE(n_b == 0 || (b_pt_off && b_cls && out_b_action && out_b_pixels && out_b_match && out_b_iou && out_b_best),
                "null pointer");
    DYD_REQUIRE((n_a_points == 0 || a_xy) && (n_b_points == 0 || b_xy), "null pointer");
    const K22Table a{a_xy, a_pt_off, a_row_off, a_cls, n_a, n_a_points, out_a_action, out_a_pixels, out_a_match, out_a_best};
    const K22Table b{b_xy, b_pt_off, b_row_off, b_cls, n_b, n_b_points, out_b_action, out_b_pixels, out_b_match, out_b_best};
    const K22Out o{out_row_status, out_pair_off, out_b_iou, out_row_counts, out_confusion, out_pixel_confusion, out_row_pixels};
    // no buffer from the caller is not "measure only" here: the pair counts then live in one the library allocates in st
    SizedOut given(K22_PAIRS, out_pairs_or_null, pair_cap), own(K22_PAIRS, st);
    return compare_launch(a, b, width, height, n_rows, n_classes, thr, by_label != 0, max_pixels_per_row, max_pairs_per_row, o,
                          out_pairs_or_null ? given : own, st);
}

int dyd_compare_polygons(const double *a_xy, const int32_t *a_pt_off, const int32_t *a_row_off, const int32_t *a_cls,
                         const double *b_xy, const int32_t *b_pt_off, const int32_t *b_row_off, const int32_t *b_cls,
                         const double *width, const double *height, int64_t n_rows, int32_t n_classes, double thr, int by_label,
                         int64_t max_pixels_per_row, int64_t max_pairs_per_row, uint8_t *out_row_status, int64_t *out_pair_off,
                         uint8_t *out_a_action, uint8_t *out_b_action, int64_t *out_a_pixels, int64_t *out_b_pixels,
                         int32_t *out_a_match, int32_t *out_b_match, double *out_b_iou, double *out_a_best, double *out_b_best,
                         int32_t *out_row_counts, uint64_t *out_confusion, uint64_t *out_pixel_confusion, int64_t *out_row_pixels) {
    DYD_API_ENTER();
    int rc = compare_params(n_classes, max_pixels_per_row, max_pairs_per_row);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31), "size too large");
    if (n_rows == 0) return DYD_OK;
    DYD_REQUIRE(out_pair_off && out_row_counts && out_confusion && out_pixel_confusion && out_row_pixels, "null pointer");
    int64_t na = 0, npa = 0, nb = 0, npb = 0;
    if ((rc = poly_table_check(a_xy, a_pt_off, a_row_off, n_rows, width, height, out_row_status != nullptr,
                               a_cls && out_a_action && out_a_pixels && out_a_match && out_a_best, nullptr, 0, &na, &npa)) ||
        (rc = poly_table_check(b_xy, b_pt_off, b_row_off, n_rows, width, height, out_row_status != nullptr,
                               b_cls && out_b_action && out_b_pixels && out_b_match && out_b_iou && out_b_best, nullptr, 0, &nb, &npb)))
        return rc;
    for (int64_t p = 0; p < na; ++p) DYD_REQUIRE(a_cls[p] < n_classes, "class id outside the list");
    for (int64_t p = 0; p < nb; ++p) DYD_REQUIRE(b_cls[p] < n_classes, "class id outside the list");
    hipStream_t st = ctx().stream;
    PolyTableDev ta;
    DevBuf b_xyd, b_pt, b_row, d_ca, d_cb, d_status, d_poff, d_aact, d_bact, d_apix, d_bpix, d_am, d_bm, d_bi, d_ab, d_bb, d_rows,
        d_conf, d_pconf, d_rpix;
    const size_t cells = 8 * (size_t)(n_classes + 1) * (size_t)(n_classes + 1);
    if ((rc = ta.upload(a_xy, a_pt_off, a_row_off, width, height, n_rows, na, npa)) ||
        (rc = poly_column(b_xyd, npb ? b_xy : nullptr, 16 * (size_t)npb)) ||
        (rc = poly_column(b_pt, nb ? b_pt_off : nullptr, nb ? 4 * (size_t)(nb + 1) : 0)) ||
        (rc = poly_column(b_row, b_row_off, 4 * (size_t)(n_rows + 1))) || (rc = poly_column(d_ca, a_cls, 4 * (size_t)na)) ||
        (rc = poly_column(d_cb, b_cls, 4 * (size_t)nb)) || (rc = d_status.alloc((size_t)n_rows)) ||
        (rc = d_poff.alloc(8 * (size_t)(n_rows + 1))) || (rc = d_aact.alloc((size_t)na)) || (rc = d_bact.alloc((size_t)nb)) ||
        (rc = d_apix.alloc(8 * (size_t)na)) || (rc = d_bpix.alloc(8 * (size_t)nb)) || (rc = d_am.alloc(4 * (size_t)na)) ||
        (rc = d_bm.alloc(4 * (size_t)nb)) || (rc = d_bi.alloc(8 * (size_t)nb)) || (rc = d_ab.alloc(8 * (size_t)na)) ||
        (rc = d_bb.alloc(8 * (size_t)nb)) || (rc = d_rows.alloc(16 * (size_t)n_rows)) || (rc = d_conf.alloc(cells)) ||
        (rc = d_pconf.alloc(cells)) || (rc = d_rpix.alloc(16 * (size_t)n_rows)))
        return rc;
    const K22Table a{ta.xy.as<double>(), ta.pt.as<int32_t>(), ta.row.as<int32_t>(), d_ca.as<int32_t>(), na, npa,
                     d_aact.as<uint8_t>(), d_apix.as<int64_t>(), d_am.as<int32_t>(), d_ab.as<double>()};
    const K22Table b{b_xyd.as<double>(), b_pt.as<int32_t>(), b_row.as<int32_t>(), d_cb.as<int32_t>(), nb, npb,
                     d_bact.as<uint8_t>(), d_bpix.as<int64_t>(), d_bm.as<int32_t>(), d_bb.as<double>()};
    const K22Out o{d_status.as<uint8_t>(), d_poff.as<int64_t>(), d_bi.as<double>(), d_rows.as<int32_t>(), d_conf.as<uint64_t>(),
                   d_pconf.as<uint64_t>(), d_rpix.as<int64_t>()};
    SizedOut pairs(K22_PAIRS, st);
    KernelTimer timer(st);
    rc = compare_launch(a, b, ta.w.as<double>(), ta.h.as<double>(), n_rows, n_classes, thr, by_label != 0, max_pixels_per_row,
                        max_pairs_per_row, o, pairs, st);
    if (rc) return rc;
    timer.finish();
    const CopyBack back[] = {{out_row_status, d_status.p, (size_t)n_rows}, {out_pair_off, d_poff.p, 8 * (size_t)(n_rows + 1)},
                             {out_a_action, d_aact.p, (size_t)na}, {out_b_action, d_bact.p, (size_t)nb},
                             {out_a_pixels, d_apix.p, 8 * (size_t)na}, {out_b_pixels, d_bpix.p, 8 * (size_t)nb},
                             {out_a_match, d_am.p, 4 * (size_t)na}, {out_b_match, d_bm.p, 4 * (size_t)nb},
                             {out_b_iou, d_bi.p, 8 * (size_t)nb}, {out_a_best, d_ab.p, 8 * (size_t)na},
                             {out_b_best, d_bb.p, 8 * (size_t)nb}, {out_row_counts, d_rows.p, 16 * (size_t)n_rows},
                             {out_confusion, d_conf.p, cells}, {out_pixel_confusion, d_pconf.p, cells},
                             {out_row_pixels, d_rpix.p, 16 * (size_t)n_rows}};
    for (const CopyBack &c : back)
        if (c.bytes) DYD_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
