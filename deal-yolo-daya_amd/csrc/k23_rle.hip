// k23_rle.hip — K23: COCO run-length masks, the column-major run lengths of every selected polygon's own mask and their
// "counts" string, with the mask's pixel area and pixel box.
//
// cover(p) is K21's pixel set (include/dyd.h has the rule and the run / string definition, DESIGN §5u the mapping and its cost).
// The pixel rule comes from k21_cover.h: the row rule, the polygon kernel (k21_polys, defined in k21_raster.hip) and the edge ->
// crossing list -> parity step (k21_edges).  This file keeps what runs need beyond coverage: the box of columns and scanlines a
// polygon can reach, the transitions in column-major order, their differences and the string.
//
// Layout in HBM: xy = P x (x, y) f64, pt_off = B+1 int32, row_off = N+1 int32, sel = B int32, width / height = N f64.
// Outputs: row_status = N u8, action = B u8, area = B int64, bbox = 4B int32, run_off = B+1 int64, runs = R u32, text_off = B+1
// int64, text.  Scratch: 112 bytes per polygon (box of V, reach, counters, three offsets), 10 bytes per reach column, 4 bytes
// per cell (a reach column within a band of `band` scanlines), 4 bytes per transition, 8 bytes per run, the scans' partial
// sums.  Nothing is sized by an image; the band height is doubled until the cells fit K23_MAX_CELLS.
//
// A polygon's reach: the columns [c0, c1) and scanlines [j0, j1) outside of which it covers nothing.  No edge crosses a
// scanline unless by1 <= yc < by2, which gives j0 and j1 exactly; a column with xc <= bx1 - 1 or xc >= bx2 + 1 is not covered
// (k21_reaches' argument), and the reach keeps one such column on its right, so the column after the reach never sees a
// covered pixel above it.  Both are clamped to the image.  An item is (polygon, strip of `strip` <= 1024 columns of the reach,
// band of `band` scanlines of the reach): lane l holds the columns 64 c + l of the strip as bit c of 32-bit masks (K22's
// layout), so a lane's state is a few registers; the per-column counters live in LDS, where a lane touches only its own
// columns.  No kernel indexes a per-lane array: no scratch.
//
// Steps (no hand-off between workgroups inside a launch):
//   1. rows, a lane per row: the status; polygons, a lane per polygon: K21's action and box, then the reach and its items,
//      columns and cells; three scans give their offsets; the host reads the totals;
//   2. count, a wave (one workgroup) per item, items taken grid-stride: the wave walks the band's scanlines (after the one
//      before the band, for the bits to compare the first with), k21_edges lists the crossings of each, every lane XORs xs > xc
//      of its columns and compares the bits with the previous scanline's.  A change is a transition at i * H + j.  The item
//      stores its transitions per column (its cells), the band at the image's top the columns' first bits, the band at its
//      bottom their last bits; the covered pixels and their extent leave by integer atomics;
//   3. columns, a lane per reach column: the top of a column continues the bottom of the column to its left, so a transition
//      at line 0 exists when those two bits differ; then the column's cells become exclusive sums down the bands and its
//      total goes to a scan over all columns.  A lane per polygon gives run_off, area and bbox; a scan; the host reads the totals;
//   4. write, a wave per item: the walk again, every lane storing the transitions of its columns at the column's offset plus
//      the cell's;
//   5. runs, a lane per run: differences of the transitions, out of place, and the byte count of the run's code; a scan gives
//      the codes' offsets, a lane per polygon text_off; the host reads the text's length;
//   6. print, a lane per run: the code of run i from runs[i] and runs[i - 2].
#include "k13_scan.h"
#include "k21_cover.h"
#include "poly_table.h"
#include "sized_out.h"

#include <climits>

namespace dyd {

constexpr int K23_BLOCK = 256;
constexpr int K23_STRIP = 1024;              // columns per item (default and most): 16 columns per lane, a bit each
constexpr int K23_BAND = 64;                 // scanlines per item (default)
constexpr int K23_CROSSINGS = 256;           // capacity of the crossing list (default and most)
constexpr int64_t K23_MAX_PIXELS = 1LL << 30;
constexpr int64_t K23_MAX_GRID = 1 << 20;    // walk workgroups; the items beyond are taken grid-stride
constexpr int64_t K23_MAX_CELLS = 1LL << 26; // cells beyond which the band height is doubled

// a polygon's reach and its image
struct K23Geo {
    int32_t c0, c1, j0, j1, W, H;
};

// what the count step gathers per polygon: covered pixels and their extent (first / last column and line)
struct K23Ext {
    unsigned long long area;
    int32_t x0, y0, x1, y1;
};

// ---- 1. rows and polygons ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(K23_BLOCK) void k23_rows_kernel(const double *__restrict__ width, const double *__restrict__ height,
                                                             int64_t n_rows, int64_t max_pixels, uint8_t *__restrict__ row_status) {
    const int64_t i = (int64_t)blockIdx.x * K23_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    int64_t w, h;
    row_status[i] = k21_row_size(width[i], height[i], max_pixels, &w, &h);
}

__device__ __forceinline__ int32_t k23_clamp(double v, int64_t hi) {   // v is a whole number or infinite
    return v > 0.0 ? (v < (double)hi ? (int32_t)v : (int32_t)hi) : 0;
}

// after k21_polys: the reach; the items, reach columns and cells (item_off / col_off / cell_off [p + 1], before their scans)
// and cleared counters
__global__ __launch_bounds__(K23_BLOCK) void k23_reach_kernel(const int32_t *__restrict__ row_off, const double *__restrict__ width,
                                                              const double *__restrict__ height, int64_t n_rows, int64_t n_polys,
                                                              int strip, int band, const uint8_t *__restrict__ action,
                                                              const double *__restrict__ info, K23Geo *__restrict__ geo,
                                                              int64_t *__restrict__ item_off, int64_t *__restrict__ col_off,
                                                              int64_t *__restrict__ cell_off, K23Ext *__restrict__ ext) {
    __shared__ int32_t rows[2];
    const int64_t p0 = (int64_t)blockIdx.x * K23_BLOCK, p1 = min(p0 + K23_BLOCK, n_polys);
    poly_tile_rows(row_off, n_rows, p0, p1, rows);
    const int64_t p = p0 + threadIdx.x;
    if (p >= p1) return;
    K23Geo g{0, 0, 0, 0, 0, 0};
    int64_t items = 0, cols = 0, cells = 0;
    if (action[p] == COVER_DONE) {   // so the row's status is 0: W and H are whole numbers with W * H <= 2^30
        const int64_t r = last_le(row_off, rows[0], rows[1], p);
        const int64_t W = (int64_t)width[r], H = (int64_t)height[r];
        const double *q = info + 4 * p;
        g.W = (int32_t)W;
        g.H = (int32_t)H;
        g.c0 = k23_clamp(floor(q[0] - 1.5) + 1.0, W);
        g.c1 = k23_clamp(ceil(q[2] + 0.5) + 1.0, W);
        g.j0 = k23_clamp(ceil(q[1] - 0.5), H);
        g.j1 = k23_clamp(ceil(q[3] - 0.5), H);
        if (g.c1 > g.c0 && g.j1 > g.j0) {
            const int64_t n_bands = ((int64_t)g.j1 - g.j0 + band - 1) / band;
            cols = g.c1 - g.c0;
            items = ((cols + strip - 1) / strip) * n_bands;
            cells = cols * n_bands;
        } else {
            g.c0 = g.c1 = g.j0 = g.j1 = 0;
        }
    }
    geo[p] = g;
    item_off[p + 1] = items;
    col_off[p + 1] = cols;
    cell_off[p + 1] = cells;
    if (p == 0) item_off[0] = col_off[0] = cell_off[0] = 0;
    ext[p] = K23Ext{0ull, INT_MAX, INT_MAX, -1, -1};
}

// one item: its polygon, strip, band and points
struct K23Item {
    int64_t p, x0, col, cell;   // the strip's first column, its index among the reach columns, the item's first cell
    int npx, n, ja, jb;         // columns; points; the band's scanlines [ja, jb)
    bool first, last;           // the reach's first / last band
    const double2 *pts;
    K23Geo g;
};

__device__ __forceinline__ K23Item k23_item(const double *__restrict__ xy, const int32_t *__restrict__ pt_off, int64_t n_polys,
                                            int64_t n_points, int strip, int band, const int64_t *__restrict__ item_off,
                                            const int64_t *__restrict__ col_off, const int64_t *__restrict__ cell_off,
                                            const K23Geo *__restrict__ geo, int64_t item) {
    K23Item it;
    it.p = last_le(item_off, 0, n_polys, item);   // item_off[n_polys] is the item count, so p < n_polys
    it.g = geo[it.p];
    const int64_t local = item - item_off[it.p];
    const int64_t n_bands = max(((int64_t)it.g.j1 - it.g.j0 + band - 1) / band, (int64_t)1);
    const int64_t s = local / n_bands, b = local - s * n_bands;   // the bands of a strip are neighbours
    it.x0 = it.g.c0 + s * strip;
    it.npx = (int)max(min((int64_t)strip, it.g.c1 - it.x0), (int64_t)0);
    it.col = col_off[it.p] + s * strip;
    it.cell = cell_off[it.p] + s * strip * n_bands + b * it.npx;   // [strip][band][column]: the strips before are full
    it.ja = (int)(it.g.j0 + b * band);
    it.jb = (int)min((int64_t)it.ja + band, (int64_t)it.g.j1);
    it.first = b == 0;
    it.last = b == n_bands - 1;
    const int32_t a = max(pt_off[it.p], 0), e = (int32_t)min((int64_t)max(pt_off[it.p + 1], a), n_points);
    it.pts = reinterpret_cast<const double2 *>(xy) + a;
    it.n = e - a;
    return it;
}

// ---- the walk of one item by a wave ------------------------------------------------------------------------------
// The item's columns are x0 + 64 c + lane for c < n_words: bit c of a lane's masks is its column of word c (K22's layout).
// seen(j, covered bits) for every scanline of the band, emit(j, bits) for the columns with a transition at a line j > 0,
// lines ascending; a transition at line 0 is the columns step's.  *top: the bits of line 0 (first band of a reach that
// begins there, else 0), *bot: the bits of the image's last line (last band of a reach that ends there, else 0).
template <class Seen, class Emit>
__device__ __forceinline__ void k23_walk(const K23Item &it, const double *__restrict__ box, int cap, double *list, Seen seen, Emit emit,
                                         uint32_t *top_out, uint32_t *bot_out) {
    const int lane = threadIdx.x;
    const int n_words = (it.npx + kWave - 1) / kWave;
    uint32_t valid = 0;
    for (int c = 0; c < n_words; ++c) valid |= (uint32_t)(c * kWave + lane < it.npx) << c;
    uint32_t prev = 0, top = 0;
    for (int j = it.first ? it.ja : it.ja - 1; j < it.jb; ++j) {   // wave-uniform; a later band begins a line early
        uint32_t par = 0;
        // the crossings listed so far, XORed into the parity of the lane's columns
        auto apply = [&](int n_listed) __attribute__((always_inline)) {
            __syncthreads();
            for (int c = 0; c < n_words; ++c) {
                const double xc = (double)(it.x0 + c * kWave + lane) + 0.5;
                uint32_t bit = 0;
                for (int k = 0; k < n_listed; ++k) bit ^= (uint32_t)(list[k] > xc);
                par ^= bit << c;
            }
            __syncthreads();
        };
        k21_edges(it.pts, it.n, box, (double)j + 0.5, cap, list, apply);
        const uint32_t cur = par & valid;
        if (j >= it.ja) {
            seen(j, cur);
            if (j == 0) top = cur;
            else if (cur != prev) emit(j, cur ^ prev);
        }
        prev = cur;
    }
    const bool closes = it.last && it.g.j1 < it.g.H;   // the line below the reach is not covered
    if (closes && prev) emit(it.g.j1, prev);
    *top_out = top;
    *bot_out = it.last && !closes ? prev : 0u;
}

__device__ __forceinline__ int64_t k23_wave_sum(int64_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int k23_wave_min(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int k23_wave_max(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// ---- 2. count: a wave per item -----------------------------------------------------------------------------------
// cells[it.cell + column] = the transitions of the item's column below line 0; top / bot [it.col + column] by the first /
// last band
__global__ __launch_bounds__(kWave) void k23_count_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                          int64_t n_polys, int64_t n_points, int strip, int band, int cap,
                                                          const int64_t *__restrict__ item_off, const int64_t *__restrict__ col_off,
                                                          const int64_t *__restrict__ cell_off, int64_t n_items, int64_t n_cols,
                                                          int64_t n_cells, const K23Geo *__restrict__ geo,
                                                          const double *__restrict__ info, uint32_t *__restrict__ cells,
                                                          uint8_t *__restrict__ top, uint8_t *__restrict__ bot,
                                                          K23Ext *__restrict__ ext) {
    __shared__ double list[K23_CROSSINGS];
    __shared__ uint32_t cnt[K23_STRIP];   // per column; a lane touches its own columns only
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const K23Item it = k23_item(xy, pt_off, n_polys, n_points, strip, band, item_off, col_off, cell_off, geo, item);
        const int n_words = (it.npx + kWave - 1) / kWave;
        for (int c = 0; c < n_words; ++c) cnt[c * kWave + lane] = 0;
        int64_t cov = 0;
        int jmin = INT_MAX, jmax = -1;
        uint32_t ever = 0;   // the lane's columns that hold a covered pixel
        auto seen = [&](int j, uint32_t cur) __attribute__((always_inline)) {
            if (cur) {
                cov += __popc(cur);
                jmin = min(jmin, j);
                jmax = j;
                ever |= cur;
            }
        };
        auto emit = [&](int, uint32_t bits) __attribute__((always_inline)) {
            for (; bits; bits &= bits - 1) ++cnt[(__ffs((int)bits) - 1) * kWave + lane];
        };
        uint32_t tbits, bbits;
        k23_walk(it, info + 4 * it.p, cap, list, seen, emit, &tbits, &bbits);
        for (int c = 0; c < n_words; ++c) {
            const int x = c * kWave + lane;
            if (x >= it.npx) continue;
            if (it.cell + x < n_cells) cells[it.cell + x] = cnt[x];   // always inside for sound offsets
            if (it.col + x < n_cols) {
                if (it.first) top[it.col + x] = (uint8_t)((tbits >> c) & 1u);
                if (it.last) bot[it.col + x] = (uint8_t)((bbits >> c) & 1u);
            }
        }
        const int col = (int)it.x0 + lane;
        const int x_lo = k23_wave_min(ever ? col + (__ffs((int)ever) - 1) * kWave : INT_MAX);
        const int x_hi = k23_wave_max(ever ? col + (31 - __clz((int)ever)) * kWave : -1);
        const int y_lo = k23_wave_min(jmin), y_hi = k23_wave_max(jmax);
        const int64_t n_cov = k23_wave_sum(cov);
        if (lane == 0 && n_cov > 0) {
            K23Ext *e = ext + it.p;
            atomicAdd(&e->area, (unsigned long long)n_cov);
            atomicMin(&e->x0, x_lo);
            atomicMin(&e->y0, y_lo);
            atomicMax(&e->x1, x_hi);
            atomicMax(&e->y1, y_hi);
        }
    }
}

// ---- 3. columns: a lane per reach column ---------------------------------------------------------------------------
// The column's cells become exclusive sums down its bands, beginning at 1 when the column has a transition at line 0;
// col_tr[g + 1] = its transitions (before the scan).
__global__ __launch_bounds__(K23_BLOCK) void k23_columns_kernel(int64_t n_polys, int strip, int band, const int64_t *__restrict__ col_off,
                                                                const int64_t *__restrict__ cell_off, int64_t n_cols, int64_t n_cells,
                                                                const K23Geo *__restrict__ geo, const uint8_t *__restrict__ top,
                                                                const uint8_t *__restrict__ bot, uint32_t *__restrict__ cells,
                                                                int64_t *__restrict__ col_tr) {
    const int64_t g = (int64_t)blockIdx.x * K23_BLOCK + threadIdx.x;
    if (g >= n_cols) return;
    if (g == 0) col_tr[0] = 0;
    const int64_t p = last_le(col_off, 0, n_polys, g);   // col_off[n_polys] = n_cols > g, so p < n_polys
    const K23Geo q = geo[p];
    const int64_t ci = g - col_off[p], cols = (int64_t)q.c1 - q.c0;
    const int64_t n_bands = max(((int64_t)q.j1 - q.j0 + band - 1) / band, (int64_t)1);
    const int64_t s = ci / strip, x = ci - s * strip, npx = min((int64_t)strip, cols - s * strip);
    const uint8_t left = ci > 0 ? bot[g - 1] : (uint8_t)0;   // nothing is covered before the reach
    uint32_t run = left != top[g] ? 1u : 0u;
    const int64_t first = cell_off[p] + s * strip * n_bands + x;
    for (int64_t b = 0; b < n_bands; ++b) {
        const int64_t at = first + b * npx;
        if (at >= n_cells) break;   // never for sound offsets
        const uint32_t v = cells[at];
        cells[at] = run;
        run += v;
    }
    col_tr[g + 1] = run;
}

// a lane per polygon: run count (run_off[p + 1], before its scan), area and box
__global__ __launch_bounds__(K23_BLOCK) void k23_poly_kernel(int64_t n_polys, const uint8_t *__restrict__ action,
                                                             const int64_t *__restrict__ col_off, const int64_t *__restrict__ col_tr,
                                                             const K23Ext *__restrict__ ext, int64_t *__restrict__ run_off,
                                                             int64_t *__restrict__ area, int32_t *__restrict__ bbox) {
    const int64_t p = (int64_t)blockIdx.x * K23_BLOCK + threadIdx.x;
    if (p >= n_polys) return;
    const bool done = action[p] == COVER_DONE;
    run_off[p + 1] = done ? col_tr[col_off[p + 1]] - col_tr[col_off[p]] + 1 : 0;
    if (p == 0) run_off[0] = 0;
    const K23Ext e = ext[p];
    const bool some = done && e.area > 0;
    area[p] = some ? (int64_t)e.area : 0;
    int32_t *b = bbox + 4 * p;
    b[0] = some ? e.x0 : 0;
    b[1] = some ? e.y0 : 0;
    b[2] = some ? e.x1 - e.x0 + 1 : 0;
    b[3] = some ? e.y1 - e.y0 + 1 : 0;
}

// ---- 4. write: a wave per item -----------------------------------------------------------------------------------
// trans[col_tr[column] + the cell's sum ..) = the transitions of the item's columns, ascending
__global__ __launch_bounds__(kWave) void k23_write_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                          int64_t n_polys, int64_t n_points, int strip, int band, int cap,
                                                          const int64_t *__restrict__ item_off, const int64_t *__restrict__ col_off,
                                                          const int64_t *__restrict__ cell_off, int64_t n_items, int64_t n_cols,
                                                          int64_t n_cells, const K23Geo *__restrict__ geo,
                                                          const double *__restrict__ info, const uint32_t *__restrict__ cells,
                                                          const int64_t *__restrict__ col_tr, int64_t tr_total,
                                                          uint32_t *__restrict__ trans) {
    __shared__ double list[K23_CROSSINGS];
    __shared__ uint32_t pos[K23_STRIP];   // per column: where its next transition goes, from the polygon's first; own columns only
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const K23Item it = k23_item(xy, pt_off, n_polys, n_points, strip, band, item_off, col_off, cell_off, geo, item);
        const int n_words = (it.npx + kWave - 1) / kWave;
        const int64_t base = col_tr[col_off[it.p]];   // the polygon's first transition; a polygon has at most 2^30
        const uint32_t H = (uint32_t)it.g.H, k0 = ((uint32_t)it.x0 + lane) * H;   // indices stay below W * H <= 2^30
        for (int c = 0; c < n_words; ++c) {
            const int x = c * kWave + lane;
            if (x >= it.npx || it.col + x >= n_cols || it.cell + x >= n_cells) continue;
            const int64_t at = col_tr[it.col + x];
            const uint32_t before = cells[it.cell + x];
            pos[x] = (uint32_t)(at - base) + before;
            // the first band's sum begins at 1 when the column has a transition at line 0
            if (it.first && before != 0 && at < tr_total) trans[at] = k0 + (uint32_t)(c * kWave) * H;
        }
        auto nothing = [](int, uint32_t) __attribute__((always_inline)) {};
        auto store = [&](int j, uint32_t bits) __attribute__((always_inline)) {
            for (; bits; bits &= bits - 1) {
                const int c = __ffs((int)bits) - 1;
                const int64_t at = base + pos[c * kWave + lane]++;
                if (at < tr_total) trans[at] = k0 + (uint32_t)(c * kWave) * H + (uint32_t)j;   // always inside for sound offsets
            }
        };
        uint32_t tbits, bbits;
        k23_walk(it, info + 4 * it.p, cap, list, nothing, store, &tbits, &bbits);
    }
}

// ---- 5. runs: a lane per run ---------------------------------------------------------------------------------------
// bytes of the code of x (COCO's rleToString): five bits per byte, until the rest is the sign
__device__ __forceinline__ int k23_code_len(int32_t x) {
    int n = 0;
    for (bool more = true; more;) {
        const int32_t b = x & 0x1f;
        x >>= 5;
        more = (b & 0x10) ? x != -1 : x != 0;
        ++n;
    }
    return n;
}

// run q of polygon p is T(q) - T(q - 1) over the polygon's m transitions, with T(-1) = 0 and T(m) = W * H.
// code_off[g + 1] = the bytes of run g's code, before their scan.
__global__ __launch_bounds__(K23_BLOCK) void k23_runs_kernel(int64_t n_polys, const int64_t *__restrict__ col_off,
                                                             const int64_t *__restrict__ col_tr, const K23Geo *__restrict__ geo,
                                                             const int64_t *__restrict__ run_off, int64_t n_runs,
                                                             const uint32_t *__restrict__ trans, uint32_t *__restrict__ runs,
                                                             int64_t *__restrict__ code_off) {
    const int64_t g = (int64_t)blockIdx.x * K23_BLOCK + threadIdx.x;
    if (g >= n_runs) return;
    const int64_t p = last_le(run_off, 0, n_polys, g);   // run_off[n_polys] = n_runs > g, so p < n_polys
    const int64_t q = g - run_off[p], m = run_off[p + 1] - run_off[p] - 1;
    const uint32_t *t = trans + col_tr[col_off[p]];
    const int64_t WH = (int64_t)geo[p].W * geo[p].H;
    auto T = [&](int64_t i) -> int64_t { return i < 0 ? 0 : (i >= m ? WH : (int64_t)t[i]); };
    const int64_t c = T(q) - T(q - 1);
    runs[g] = (uint32_t)c;
    const int64_t x = q > 2 ? c - (T(q - 2) - T(q - 3)) : c;
    code_off[g + 1] = k23_code_len((int32_t)x);
    if (g == 0) code_off[0] = 0;
}

__global__ __launch_bounds__(K23_BLOCK) void k23_text_off_kernel(int64_t n_polys, const int64_t *__restrict__ run_off,
                                                                 const int64_t *__restrict__ code_off, int64_t *__restrict__ text_off) {
    const int64_t p = (int64_t)blockIdx.x * K23_BLOCK + threadIdx.x;
    if (p <= n_polys) text_off[p] = code_off[run_off[p]];
}

// ---- 6. print: a lane per run --------------------------------------------------------------------------------------
__global__ __launch_bounds__(K23_BLOCK) void k23_print_kernel(int64_t n_polys, const int64_t *__restrict__ run_off, int64_t n_runs,
                                                              const uint32_t *__restrict__ runs, const int64_t *__restrict__ code_off,
                                                              int64_t total, uint8_t *__restrict__ text) {
    const int64_t g = (int64_t)blockIdx.x * K23_BLOCK + threadIdx.x;
    if (g >= n_runs) return;
    const int64_t p = last_le(run_off, 0, n_polys, g);
    int32_t x = (int32_t)runs[g];
    if (g - run_off[p] > 2) x -= (int32_t)runs[g - 2];
    int64_t at = code_off[g];
    for (bool more = true; more; ++at) {
        int32_t b = x & 0x1f;
        x >>= 5;
        more = (b & 0x10) ? x != -1 : x != 0;
        if (more) b |= 0x20;
        if (at < total) text[at] = (uint8_t)(b + 48);   // always inside for sound offsets
    }
}

// dyd_set_option("k23_strip" / "k23_band" / "k23_crossings" / "k23_grid", n): the strip's width, the band's height, the list's
// capacity and a cap on the walk workgroups; <= 0 restores the default, larger values are capped
static int g_k23_strip = K23_STRIP, g_k23_band = K23_BAND, g_k23_crossings = K23_CROSSINGS;
static int64_t g_k23_grid = K23_MAX_GRID;

void set_k23_strip(int v) { g_k23_strip = k21_capped(v, K23_STRIP); }
void set_k23_band(int v) { g_k23_band = v > 0 ? k21_capped(v, 1 << 30) : K23_BAND; }
void set_k23_crossings(int v) { g_k23_crossings = k21_capped(v, K23_CROSSINGS); }
void set_k23_grid(int v) { g_k23_grid = k21_capped(v, (int)K23_MAX_GRID); }

struct RleOut {
    uint8_t *row_status, *action;
    int64_t *area;
    int32_t *bbox;
    int64_t *run_off, *text_off;
};

// v[0..n) -> its inclusive prefix sums; the partial sums live until the scan has run
static int rle_scan(int64_t *v, int64_t n, hipStream_t st) {
    if (n <= 0) return DYD_OK;
    DevBuf part;
    int rc = part.alloc(8 * (size_t)k13_scan_parts(n), st);
    if (rc) return rc;
    k13_scan_inclusive(v, n, part.as<int64_t>(), st);
    return DYD_OK;
}

static inline dim3 rle_grid(int64_t n) { return dim3((unsigned)ceil_div(n, (int64_t)K23_BLOCK)); }

constexpr SizedName K23_RUNS{"K23", "run", "runs", 4}, K23_TEXT{"K23", "text", "bytes", 1};

// Steps 1 to 6 on device pointers, n_rows > 0.  `runs_out` and `text_out` are asked for the buffers once their sizes are known
// (none: stop there).  *run_total and *text_total are host values; st is synchronised on return.
static int rle_launch(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *sel, const double *width,
                      const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int64_t max_pixels, const RleOut &o,
                      int64_t *run_total, int64_t *text_total, SizedOut &runs_out, SizedOut &text_out, hipStream_t st) {
    const int strip = g_k23_strip, cap = g_k23_crossings;
    *run_total = *text_total = 0;
    hipLaunchKernelGGL(k23_rows_kernel, rle_grid(n_rows), dim3(K23_BLOCK), 0, st, width, height, n_rows, max_pixels, o.row_status);
    DYD_HIP(hipMemsetAsync(o.run_off, 0, 8, st));
    if (n_polys == 0) {
        DYD_HIP(hipGetLastError());
        DYD_HIP(hipStreamSynchronize(st));
        const int rc = runs_out.get(0);
        if (rc || !runs_out.p) return rc;
        DYD_HIP(hipMemsetAsync(o.text_off, 0, 8, st));
        DYD_HIP(hipStreamSynchronize(st));
        return text_out.get(0);
    }
    DevBuf d_info, d_geo, d_ext, d_off, d_cells, d_bits, d_col_tr, d_trans, d_code_off;
    int rc;
    const size_t off_len = (size_t)(n_polys + 1);
    if ((rc = d_info.alloc(32 * (size_t)n_polys, st)) || (rc = d_geo.alloc(sizeof(K23Geo) * (size_t)n_polys, st)) ||
        (rc = d_ext.alloc(sizeof(K23Ext) * (size_t)n_polys, st)) || (rc = d_off.alloc(24 * off_len, st)))
        return rc;
    double *info = d_info.as<double>();
    K23Geo *geo = d_geo.as<K23Geo>();
    K23Ext *ext = d_ext.as<K23Ext>();
    int64_t *item_off = d_off.as<int64_t>(), *col_off = item_off + off_len, *cell_off = col_off + off_len;
    k21_polys(xy, pt_off, row_off, sel, o.row_status, n_rows, n_polys, n_points, o.action, info, st);
    // the reach and its items; a band height that keeps the cells within K23_MAX_CELLS (at most one cell per reach column)
    int band = g_k23_band;
    int64_t n_items = 0, n_cols = 0, n_cells = 0;
    for (;;) {
        hipLaunchKernelGGL(k23_reach_kernel, rle_grid(n_polys), dim3(K23_BLOCK), 0, st, row_off, width, height, n_rows, n_polys, strip,
                           band, o.action, info, geo, item_off, col_off, cell_off, ext);
        if ((rc = rle_scan(item_off + 1, n_polys, st)) || (rc = rle_scan(col_off + 1, n_polys, st)) ||
            (rc = rle_scan(cell_off + 1, n_polys, st)))
            return rc;
        if ((rc = read_totals("K23", "the row and polygon steps",
                              {{&n_items, item_off + n_polys}, {&n_cols, col_off + n_polys}, {&n_cells, cell_off + n_polys}}, st)))
            return rc;
        if (n_cells <= K23_MAX_CELLS || n_cells == n_cols || band >= (1 << 30)) break;
        band *= 2;
    }
    // the count step, the columns' offsets and the offsets of the runs
    if ((rc = d_cells.alloc(4 * (size_t)n_cells, st)) || (rc = d_bits.alloc(2 * (size_t)n_cols, st)) ||
        (rc = d_col_tr.alloc(8 * (size_t)(n_cols + 1), st)))
        return rc;
    uint32_t *cells = d_cells.as<uint32_t>();
    uint8_t *top = d_bits.as<uint8_t>(), *bot = top + n_cols;
    int64_t *col_tr = d_col_tr.as<int64_t>();
    DYD_HIP(hipMemsetAsync(col_tr, 0, 8, st));
    const dim3 walk_grid((unsigned)(n_items < g_k23_grid ? n_items : g_k23_grid));
    if (n_items > 0) {
        hipLaunchKernelGGL(k23_count_kernel, walk_grid, dim3(kWave), 0, st, xy, pt_off, n_polys, n_points, strip, band, cap, item_off,
                           col_off, cell_off, n_items, n_cols, n_cells, geo, info, cells, top, bot, ext);
        hipLaunchKernelGGL(k23_columns_kernel, rle_grid(n_cols), dim3(K23_BLOCK), 0, st, n_polys, strip, band, col_off, cell_off, n_cols,
                           n_cells, geo, top, bot, cells, col_tr);
    }
    if ((rc = rle_scan(col_tr + 1, n_cols, st))) return rc;
    hipLaunchKernelGGL(k23_poly_kernel, rle_grid(n_polys), dim3(K23_BLOCK), 0, st, n_polys, o.action, col_off, col_tr, ext, o.run_off,
                       o.area, o.bbox);
    if ((rc = rle_scan(o.run_off + 1, n_polys, st))) return rc;
    int64_t n_runs = 0, n_trans = 0;
    if ((rc = read_totals("K23", "the count step", {{&n_runs, o.run_off + n_polys}, {&n_trans, col_tr + n_cols}}, st))) return rc;
    *run_total = n_runs;
    if ((rc = runs_out.get(n_runs)) || !runs_out.p) return rc;
    uint32_t *runs = runs_out.as<uint32_t>();
    // the transitions, the runs and the offsets of their codes
    if ((rc = d_trans.alloc(4 * (size_t)n_trans, st)) || (rc = d_code_off.alloc(8 * (size_t)(n_runs + 1), st))) return rc;
    int64_t *code_off = d_code_off.as<int64_t>();
    DYD_HIP(hipMemsetAsync(code_off, 0, 8, st));
    if (n_trans > 0)
        hipLaunchKernelGGL(k23_write_kernel, walk_grid, dim3(kWave), 0, st, xy, pt_off, n_polys, n_points, strip, band, cap, item_off,
                           col_off, cell_off, n_items, n_cols, n_cells, geo, info, cells, col_tr, n_trans, d_trans.as<uint32_t>());
    if (n_runs > 0)
        hipLaunchKernelGGL(k23_runs_kernel, rle_grid(n_runs), dim3(K23_BLOCK), 0, st, n_polys, col_off, col_tr, geo, o.run_off, n_runs,
                           d_trans.as<uint32_t>(), runs, code_off);
    if ((rc = rle_scan(code_off + 1, n_runs, st))) return rc;
    hipLaunchKernelGGL(k23_text_off_kernel, rle_grid(n_polys + 1), dim3(K23_BLOCK), 0, st, n_polys, o.run_off, code_off, o.text_off);
    int64_t total = 0;
    if ((rc = read_totals("K23", "the run step", {{&total, code_off + n_runs}}, st))) return rc;
    *text_total = total;
    if ((rc = text_out.get(total)) || !text_out.p) return rc;
    if (n_runs > 0)
        hipLaunchKernelGGL(k23_print_kernel, rle_grid(n_runs), dim3(K23_BLOCK), 0, st, n_polys, o.run_off, n_runs, runs, code_off, total,
                           text_out.as<uint8_t>());
    DYD_HIP(hipGetLastError());
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

static int rle_params(int64_t max_pixels) {
    DYD_REQUIRE(max_pixels >= 1 && max_pixels <= K23_MAX_PIXELS, "max_pixels_per_row must lie in 1..2^30");
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_polygon_rle_dev(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *sel, const double *width,
                        const double *height, int64_t n_rows, int64_t n_polys, int64_t n_points, int64_t max_pixels_per_row,
                        uint8_t *out_row_status, uint8_t *out_action, int64_t *out_area, int32_t *out_bbox, int64_t *out_run_off,
                        uint32_t *out_runs_or_null, int64_t runs_cap, int64_t *out_text_off, uint8_t *out_text_or_null,
                        int64_t text_cap, int64_t *out_run_total, int64_t *out_text_total) {
    DYD_API_ENTER();
    int rc = rle_params(max_pixels_per_row);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0 && n_polys >= 0 && n_points >= 0 && runs_cap >= 0 && text_cap >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31) && n_rows < (1LL << 31), "size too large");
    DYD_REQUIRE(out_run_off && out_run_total && out_text_total, "null pointer");
    DYD_REQUIRE(!out_text_or_null || out_runs_or_null, "text without runs");
    DYD_REQUIRE(!out_runs_or_null || out_text_off, "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(xy) & 15) == 0, "xy must be 16-byte aligned");
    hipStream_t st = ctx().stream;
    *out_run_total = *out_text_total = 0;
    if (n_rows == 0) {
        DYD_HIP(hipMemsetAsync(out_run_off, 0, 8, st));
        if (out_text_off) DYD_HIP(hipMemsetAsync(out_text_off, 0, 8, st));
        DYD_HIP(hipStreamSynchronize(st));
        return DYD_OK;
    }
    DYD_REQUIRE(row_off && width && height && out_row_status, "null pointer");
    DYD_REQUIRE(n_polys == 0 || (pt_off && sel && out_action && out_area && out_bbox), "null pointer");
    DYD_REQUIRE(n_points == 0 || xy, "null pointer");
    const RleOut o{out_row_status, out_action, out_area, out_bbox, out_run_off, out_text_off};
    SizedOut runs(K23_RUNS, out_runs_or_null, runs_cap), text(K23_TEXT, out_text_or_null, text_cap);
    return rle_launch(xy, pt_off, row_off, sel, width, height, n_rows, n_polys, n_points, max_pixels_per_row, o, out_run_total,
                      out_text_total, runs, text, st);
}

int dyd_polygon_rle(const double *xy, const int32_t *pt_off, const int32_t *row_off, const int32_t *sel, const double *width,
                    const double *height, int64_t n_rows, int64_t max_pixels_per_row, uint8_t *out_row_status, uint8_t *out_action,
                    int64_t *out_area, int32_t *out_bbox, int64_t *out_run_off, int64_t *out_text_off, uint32_t **out_runs,
                    int64_t *out_runs_len, uint8_t **out_text, int64_t *out_text_len) {
    DYD_API_ENTER();
    int rc = rle_params(max_pixels_per_row);
    if (rc) return rc;
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31), "size too large");
    DYD_REQUIRE(out_run_off && out_text_off && out_runs && out_runs_len && out_text && out_text_len, "null pointer");
    *out_runs = nullptr;
    *out_text = nullptr;
    *out_runs_len = *out_text_len = 0;
    out_run_off[0] = out_text_off[0] = 0;
    if (n_rows == 0) return DYD_OK;
    int64_t n_polys = 0, n_points = 0;
    rc = poly_table_check(xy, pt_off, row_off, n_rows, width, height, out_row_status != nullptr,
                          sel && out_action && out_area && out_bbox, nullptr, 0, &n_polys, &n_points);
    if (rc) return rc;
    hipStream_t st = ctx().stream;
    PolyTableDev t;
    DevBuf d_sel, d_status, d_act, d_area, d_bbox, d_roff, d_toff;
    const size_t off_bytes = 8 * (size_t)(n_polys + 1);
    if ((rc = t.upload(xy, pt_off, row_off, width, height, n_rows, n_polys, n_points)) ||
        (rc = poly_column(d_sel, sel, 4 * (size_t)n_polys)) || (rc = d_status.alloc((size_t)n_rows)) ||
        (rc = d_act.alloc((size_t)n_polys)) || (rc = d_area.alloc(8 * (size_t)n_polys)) || (rc = d_bbox.alloc(16 * (size_t)n_polys)) ||
        (rc = d_roff.alloc(off_bytes)) || (rc = d_toff.alloc(off_bytes)))
        return rc;
    const RleOut o{d_status.as<uint8_t>(), d_act.as<uint8_t>(), d_area.as<int64_t>(), d_bbox.as<int32_t>(), d_roff.as<int64_t>(),
                   d_toff.as<int64_t>()};
    SizedOut runs(K23_RUNS, st), text(K23_TEXT, st);
    int64_t n_runs = 0, total = 0;
    KernelTimer timer(st);
    rc = rle_launch(t.xy.as<double>(), t.pt.as<int32_t>(), t.row.as<int32_t>(), d_sel.as<int32_t>(), t.w.as<double>(),
                    t.h.as<double>(), n_rows, n_polys, n_points, max_pixels_per_row, o, &n_runs, &total, runs, text, st);
    if (rc) return rc;
    timer.finish();
    uint8_t *host_runs = nullptr;
    int64_t run_bytes = 0;
    if ((rc = hand_back_text(runs.p, 4 * n_runs, {}, st, &host_runs, &run_bytes))) return rc;
    rc = hand_back_text(text.p, total,
                        {{out_row_status, d_status.p, (size_t)n_rows}, {out_action, d_act.p, (size_t)n_polys},
                         {out_area, d_area.p, 8 * (size_t)n_polys}, {out_bbox, d_bbox.p, 16 * (size_t)n_polys},
                         {out_run_off, d_roff.p, off_bytes}, {out_text_off, d_toff.p, off_bytes}},
                        st, out_text, out_text_len);
    if (rc) {
        free(host_runs);
        return rc;
    }
    *out_runs = reinterpret_cast<uint32_t *>(host_runs);
    *out_runs_len = n_runs;
    return DYD_OK;
}

}  // extern "C"
