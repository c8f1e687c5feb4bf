// k10_audit.hip — K10: per-class box statistics of an annotation table (the box audit step).
//
// For every box: one category (no_size, bad_coords, degenerate, writable), the out-of-image flag and the COCO area bucket of a
// writable box, written as one flag byte.  Around it, exact integer counts: per image row, per class, the two per-class 2-D
// histograms over writable boxes ([c, bin(w/W), bin(h/H)] and [c, bin(xc), bin(yc)]) and the boxes-per-image histogram.  The
// arithmetic is the YOLO step's (reference core/processor.py:1046-1058) on float(v) in IEEE f64, with no contraction:
//     bw = max(x2 - x1, 0), bh = max(y2 - y1, 0); degenerate iff bw <= 0 or bh <= 0
//     xc = (x1 + x2) / 2 / W, yc = (y1 + y2) / 2 / H, wn = bw / W, hn = bh / H
//     bin(v) = min(max(floor(v * nb), 0), nb - 1), clamped in double before the integer conversion (inf can occur)
//     out_of_image = x1 < 0 or y1 < 0 or x2 > W or y2 > H; area a = bw * bh: small < 32^2 <= medium < 96^2 <= large
//
// Layout in HBM: box4 = B x (x1, y1, x2, y2) f64 (16-B aligned), row_off = N+1 int32, cls = B int32 (-1 or out of range: the name
// is no str, the box is counted per row only), width / height = N f64, size_status = N u8 (0 ok, 1 missing, 2 invalid).
// Out: flag = B u8, row_counts = N x 6 int32, class_counts = C x 9 int64, hist_wh / hist_xy = C x nb x nb int64, bpi = 257 int64.
//
// Mapping.  A persistent grid; a wave takes tiles of K10_WROWS consecutive rows (lane L holds the offset, size and status of row
// r0 + L) and walks the tile's boxes 64 at a time, one box per lane; a lane finds its row by a 5-step binary search over the lane
// offsets (ds_bpermute).  Accumulation, Guideline 12 style — reduce on chip, then one atomic per destination:
//   - per-row counts: LDS counters of the wave's tile (a tile's rows belong to one wave), stored once per tile;
//   - per-class counters: a match-any walk over the wave's class ids (leader's class -> ballot of equal lanes -> one popcount
//     per counter), then one add per (class, counter) into the block's LDS copy when C <= K10_LDS_CLASSES, else one u64 global
//     atomic;
//   - histograms: a block-private u32 copy in LDS when 2 * C * nb^2 <= K10_HIST_WORDS (20 classes at nb = 16: 40 KiB), flushed
//     once per block with u64 global atomics of the non-zero bins; otherwise (nb = 64, thousands of classes) one u64 global
//     atomic per writable box and histogram;
//   - "images" (rows with a box of the class): a box counts when no earlier box of its row has its class — the earlier lanes of
//     its row in the wave's LDS copy of the class ids, and for a row that started in an earlier 64-box chunk its earlier ids in
//     HBM (L2).
#include "box_table.h"

namespace dyd {

constexpr int K10_BLOCK = 512;
constexpr int K10_WAVES = K10_BLOCK / kWave;
constexpr int K10_WROWS = 32;               // image rows per wave tile
constexpr int K10_ROWC = 6;                 // per-row counters: unmatchable, no_size, bad_coords, degenerate, writable, out_of_image
constexpr int K10_CLSC = 9;                 // per-class counters: no_size, bad_coords, degenerate, writable, out_of_image, small,
                                            //                     medium, large, images
constexpr int K10_BPI = 257;
constexpr int K10_LDS_CLASSES = 256;
constexpr int K10_HIST_WORDS = 12288;       // 48 KiB of u32 bins

// flag byte: bits 0-1 category, bit 2 out_of_image, bits 3-4 area bucket (writable only), bit 7 name is no str (nothing else set)
constexpr uint8_t K10_UNMATCHABLE = 0x80;

struct K10Shared {
    uint32_t cls_cnt[K10_LDS_CLASSES * K10_CLSC];
    uint32_t bpi[K10_BPI];
    uint32_t rowc[K10_WAVES][K10_WROWS * K10_ROWC];
    int32_t ids[K10_WAVES][kWave];
};

__device__ __forceinline__ int k10_bin(double v, int nb) {
    double f = floor(v * (double)nb);
    f = (f < 0.0) ? 0.0 : f;
    f = (f > (double)(nb - 1)) ? (double)(nb - 1) : f;
    return (int)f;
}

__device__ __forceinline__ void k10_add_u64(int64_t *p, uint32_t v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

template <bool LDS_HIST>
__global__ __launch_bounds__(K10_BLOCK) void k10_audit_kernel(const double *__restrict__ box4, const int32_t *__restrict__ row_off,
                                                              int64_t n_rows, const int32_t *__restrict__ cls,
                                                              const double *__restrict__ width, const double *__restrict__ height,
                                                              const uint8_t *__restrict__ size_status, int32_t n_classes, int32_t nb,
                                                              uint8_t *__restrict__ out_flag, int32_t *__restrict__ out_rows,
                                                              int64_t *__restrict__ out_cls, int64_t *__restrict__ out_wh,
                                                              int64_t *__restrict__ out_xy, int64_t *__restrict__ out_bpi) {
    __shared__ K10Shared S;
    __shared__ uint32_t s_hist[LDS_HIST ? K10_HIST_WORDS : 1];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const bool lds_cls = n_classes <= K10_LDS_CLASSES;
    const int64_t hist_c = (int64_t)nb * nb;               // bins per class
    const int64_t hist_n = (int64_t)n_classes * hist_c;    // bins per histogram
    for (int k = threadIdx.x; k < K10_LDS_CLASSES * K10_CLSC; k += K10_BLOCK) S.cls_cnt[k] = 0u;
    for (int k = threadIdx.x; k < K10_BPI; k += K10_BLOCK) S.bpi[k] = 0u;
    if (LDS_HIST)
        for (int k = threadIdx.x; k < 2 * hist_n; k += K10_BLOCK) s_hist[k] = 0u;
    __syncthreads();

    uint32_t *rowc = S.rowc[wave];
    int32_t *ids = S.ids[wave];
    const int64_t n_tiles = (n_rows + K10_WROWS - 1) / K10_WROWS;
    for (int64_t tile = (int64_t)blockIdx.x * K10_WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * K10_WAVES) {
        const int64_t r0 = tile * K10_WROWS;
        const int nr = (n_rows - r0 < K10_WROWS) ? (int)(n_rows - r0) : K10_WROWS;
        const int32_t my_off = (lane <= nr) ? row_off[r0 + lane] : 0;
        double my_w = 0.0, my_h = 0.0;
        int my_st = 1;
        if (lane < nr) {
            my_st = size_status[r0 + lane];
            my_w = width[r0 + lane];
            my_h = height[r0 + lane];
            const int32_t n_row = row_off[r0 + lane + 1] - my_off;
            atomicAdd(&S.bpi[n_row < K10_BPI - 1 ? n_row : K10_BPI - 1], 1u);
        }
        for (int k = lane; k < K10_WROWS * K10_ROWC; k += kWave) rowc[k] = 0u;
        box_wave_sync();
        const int32_t base = __shfl(my_off, 0);
        const int32_t end = __shfl(my_off, nr);
        for (int32_t cb = base; cb < end; cb += kWave) {   // wave-uniform
            const int32_t b = cb + lane;
            const bool valid = b < end;
            // the lane's row: the last r < nr with off[r] <= b (empty rows before it share its offset)
            int r = 0;
#pragma unroll
            for (int step = 16; step >= 1; step >>= 1) {
                const int cand = r + step;
                const int32_t o = __shfl(my_off, cand < nr ? cand : 0);
                if (cand < nr && o <= b) r = cand;
            }
            const int32_t rs = __shfl(my_off, r);
            const double W = __shfl(my_w, r);
            const double H = __shfl(my_h, r);
            const int st = __shfl(my_st, r);

            int32_t c = -1;
            uint32_t bits = 0u;   // per-class counter bits of this box (0: no class)
            uint8_t flag = 0;
            int bin_w = 0, bin_h = 0, bin_x = 0, bin_y = 0;
            if (valid) {
                c = cls[b];
                if (c < 0 || c >= n_classes) c = -1;
                const double2 *g = reinterpret_cast<const double2 *>(box4 + 4 * (int64_t)b);
                const double2 p = g[0], q = g[1];
                const double x1 = p.x, y1 = p.y, x2 = q.x, y2 = q.y;
                int cat;
                uint32_t ooi = 0u, area = 0u;
                if (st != 0) {
                    cat = 0;
                } else if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) {
                    cat = 1;
                } else {
                    const double dx = x2 - x1, dy = y2 - y1;
                    const double bw = (0.0 > dx) ? 0.0 : dx;     // max(x2 - x1, 0.0): first argument unless 0.0 is larger
                    const double bh = (0.0 > dy) ? 0.0 : dy;
                    if (bw <= 0.0 || bh <= 0.0) {
                        cat = 2;
                    } else {
                        cat = 3;
                        ooi = (x1 < 0.0 || y1 < 0.0 || x2 > W || y2 > H) ? 1u : 0u;
                        const double a = bw * bh;
                        area = (a < 1024.0) ? 0u : (a < 9216.0) ? 1u : 2u;
                        const double xc = (x1 + x2) / 2.0 / W;
                        const double yc = (y1 + y2) / 2.0 / H;
                        const double wn = bw / W;
                        const double hn = bh / H;
                        bin_w = k10_bin(wn, nb);
                        bin_h = k10_bin(hn, nb);
                        bin_x = k10_bin(xc, nb);
                        bin_y = k10_bin(yc, nb);
                    }
                }
                const int row = r;
                if (c < 0) {
                    flag = K10_UNMATCHABLE;
                    atomicAdd(&rowc[row * K10_ROWC + 0], 1u);
                } else {
                    flag = (uint8_t)(cat | (ooi << 2) | (area << 3));
                    atomicAdd(&rowc[row * K10_ROWC + 1 + cat], 1u);
                    if (ooi) atomicAdd(&rowc[row * K10_ROWC + 5], 1u);
                    bits = (1u << cat) | (ooi << 4) | ((cat == 3) ? (1u << (5 + area)) : 0u);
                }
                out_flag[b] = flag;
            }
            // images: first box of its class in its row
            ids[lane] = c;
            box_wave_sync();
            if (c >= 0) {
                const int j0 = rs - cb;   // the row's first lane in this chunk (negative: the row started earlier)
                bool seen = false;
                for (int j = (j0 > 0 ? j0 : 0); j < lane; ++j)
                    if (ids[j] == c) { seen = true; break; }
                if (!seen && j0 < 0)
                    for (int32_t k = rs; k < cb; ++k)
                        if (cls[k] == c) { seen = true; break; }
                if (!seen) bits |= 1u << 8;
            }
            box_wave_sync();   // the next chunk overwrites ids
            // per-class counters: one group of equal class ids at a time
            unsigned long long pending = __ballot(bits != 0u);
            while (pending) {
                const int leader = __ffsll((long long)pending) - 1;
                const int32_t gc = __builtin_amdgcn_readlane(c, leader);
                const bool in = bits != 0u && c == gc;
                pending &= ~__ballot(in);
                uint32_t mine = 0u;
#pragma unroll
                for (int k = 0; k < K10_CLSC; ++k) {
                    const uint32_t n = (uint32_t)__popcll(__ballot(in && ((bits >> k) & 1u)));
                    if (lane == k) mine = n;
                }
                if (lane < K10_CLSC && mine) {
                    if (lds_cls) atomicAdd(&S.cls_cnt[gc * K10_CLSC + lane], mine);
                    else k10_add_u64(out_cls + (int64_t)gc * K10_CLSC + lane, mine);
                }
            }
            // histograms over writable boxes
            if (c >= 0 && (flag & 3) == 3) {
                const int64_t iw = (int64_t)c * hist_c + (int64_t)bin_w * nb + bin_h;
                const int64_t ix = (int64_t)c * hist_c + (int64_t)bin_x * nb + bin_y;
                if (LDS_HIST) {
                    atomicAdd(&s_hist[iw], 1u);
                    atomicAdd(&s_hist[hist_n + ix], 1u);
                } else {
                    k10_add_u64(out_wh + iw, 1u);
                    k10_add_u64(out_xy + ix, 1u);
                }
            }
        }
        box_wave_sync();
        for (int k = lane; k < nr * K10_ROWC; k += kWave) out_rows[r0 * K10_ROWC + k] = (int32_t)rowc[k];
        box_wave_sync();   // the next tile clears rowc
    }

    __syncthreads();
    for (int k = threadIdx.x; k < K10_BPI; k += K10_BLOCK)
        if (S.bpi[k]) k10_add_u64(out_bpi + k, S.bpi[k]);
    if (lds_cls)
        for (int k = threadIdx.x; k < n_classes * K10_CLSC; k += K10_BLOCK)
            if (S.cls_cnt[k]) k10_add_u64(out_cls + k, S.cls_cnt[k]);
    if (LDS_HIST)
        for (int64_t k = threadIdx.x; k < 2 * hist_n; k += K10_BLOCK)
            if (s_hist[k]) k10_add_u64(k < hist_n ? out_wh + k : out_xy + (k - hist_n), s_hist[k]);
}

int launch_k10(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls, const double *width,
               const double *height, const uint8_t *size_status, int32_t n_classes, int32_t nb, uint8_t *out_flag,
               int32_t *out_rows, int64_t *out_cls, int64_t *out_wh, int64_t *out_xy, int64_t *out_bpi, hipStream_t st) {
    const size_t hist_bytes = 8 * (size_t)n_classes * (size_t)nb * (size_t)nb;
    if (n_classes > 0) {
        DYD_HIP(hipMemsetAsync(out_cls, 0, 8 * (size_t)n_classes * K10_CLSC, st));
        DYD_HIP(hipMemsetAsync(out_wh, 0, hist_bytes, st));
        DYD_HIP(hipMemsetAsync(out_xy, 0, hist_bytes, st));
    }
    DYD_HIP(hipMemsetAsync(out_bpi, 0, 8 * (size_t)K10_BPI, st));
    if (n_rows == 0) return DYD_OK;
    const int64_t tiles = ceil_div(n_rows, (int64_t)K10_WROWS);
    const int64_t want = (int64_t)ctx().num_cu * 2;   // two 512-thread workgroups per CU (about 67 KiB of LDS each on the LDS path)
    const int64_t need = ceil_div(tiles, (int64_t)K10_WAVES);
    const unsigned blocks = (unsigned)(need < want ? need : want);
    const bool lds_hist = 2 * (int64_t)n_classes * nb * nb <= K10_HIST_WORDS;
    if (lds_hist)
        hipLaunchKernelGGL(k10_audit_kernel<true>, dim3(blocks), dim3(K10_BLOCK), 0, st, box4, row_off, n_rows, cls, width, height,
                           size_status, n_classes, nb, out_flag, out_rows, out_cls, out_wh, out_xy, out_bpi);
    else
        hipLaunchKernelGGL(k10_audit_kernel<false>, dim3(blocks), dim3(K10_BLOCK), 0, st, box4, row_off, n_rows, cls, width, height,
                           size_status, n_classes, nb, out_flag, out_rows, out_cls, out_wh, out_xy, out_bpi);
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_box_audit_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes, const int32_t *cls,
                      const double *width, const double *height, const uint8_t *size_status, int32_t n_classes, int32_t nbins,
                      uint8_t *out_flag, int32_t *out_row_counts, int64_t *out_class_counts, int64_t *out_hist_wh,
                      int64_t *out_hist_xy, int64_t *out_boxes_per_image, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_boxes >= 0 && n_classes >= 0, "n_rows, n_boxes or n_classes < 0");
    DYD_REQUIRE(nbins >= 1 && nbins <= 64, "nbins must lie in 1..64");
    DYD_REQUIRE(n_boxes < ((int64_t)1 << 31), "n_boxes exceeds int32 offsets");
    DYD_REQUIRE((int64_t)n_classes * nbins * nbins < ((int64_t)1 << 40), "n_classes * nbins^2 too large");
    DYD_REQUIRE(out_boxes_per_image, "null pointer");
    DYD_REQUIRE(n_classes == 0 || (out_class_counts && out_hist_wh && out_hist_xy), "null pointer");
    DYD_REQUIRE(n_rows == 0 || (row_off && width && height && size_status && out_row_counts), "null pointer");
    DYD_REQUIRE(n_boxes == 0 || (box4 && cls && out_flag), "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(box4) & 15) == 0, "box4 must be 16-byte aligned");
    return launch_k10(box4, row_off, n_rows, cls, width, height, size_status, n_classes, nbins, out_flag, out_row_counts,
                      out_class_counts, out_hist_wh, out_hist_xy, out_boxes_per_image, pick_stream(stream));
}

int dyd_box_audit(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls, const double *width,
                  const double *height, const uint8_t *size_status, int32_t n_classes, int32_t nbins, uint8_t *out_flag,
                  int32_t *out_row_counts, int64_t *out_class_counts, int64_t *out_hist_wh, int64_t *out_hist_xy,
                  int64_t *out_boxes_per_image) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_classes >= 0, "n_rows < 0 or n_classes < 0");
    DYD_REQUIRE(nbins >= 1 && nbins <= 64, "nbins must lie in 1..64");
    DYD_REQUIRE(out_boxes_per_image, "null pointer");
    DYD_REQUIRE(n_classes == 0 || (out_class_counts && out_hist_wh && out_hist_xy), "null pointer");
    int64_t nb;
    int rc;
    if ((rc = box_table_check(box4, row_off, n_rows, cls, width, height, size_status, n_classes, out_row_counts != nullptr,
                              out_flag != nullptr, &nb)))
        return rc;
    BoxTableDev d;
    if ((rc = d.upload(box4, row_off, n_rows, cls, width, height, size_status, nb))) return rc;
    const size_t hist_bytes = 8 * (size_t)n_classes * (size_t)nbins * (size_t)nbins;
    DevBuf d_flag, d_rows, d_cc, d_wh, d_xy, d_bpi;
    if ((rc = d_flag.alloc((size_t)nb)) || (rc = d_rows.alloc(4 * K10_ROWC * (size_t)n_rows)) ||
        (rc = d_cc.alloc(8 * K10_CLSC * (size_t)n_classes)) || (rc = d_wh.alloc(hist_bytes)) || (rc = d_xy.alloc(hist_bytes)) ||
        (rc = d_bpi.alloc(8 * K10_BPI)))
        return rc;
    hipStream_t st = ctx().stream;
    KernelTimer t(st);
    rc = launch_k10(d.box.as<double>(), d.off.as<int32_t>(), n_rows, d.cls.as<int32_t>(), d.w.as<double>(), d.h.as<double>(),
                    d.st.as<uint8_t>(), n_classes, nbins, d_flag.as<uint8_t>(), d_rows.as<int32_t>(), d_cc.as<int64_t>(),
                    d_wh.as<int64_t>(), d_xy.as<int64_t>(), d_bpi.as<int64_t>(), st);
    if (rc) return rc;
    t.finish();
    if (nb) DYD_HIP(hipMemcpyAsync(out_flag, d_flag.p, (size_t)nb, hipMemcpyDeviceToHost, st));
    if (n_rows) DYD_HIP(hipMemcpyAsync(out_row_counts, d_rows.p, 4 * K10_ROWC * (size_t)n_rows, hipMemcpyDeviceToHost, st));
    if (n_classes) {
        DYD_HIP(hipMemcpyAsync(out_class_counts, d_cc.p, 8 * K10_CLSC * (size_t)n_classes, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_hist_wh, d_wh.p, hist_bytes, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_hist_xy, d_xy.p, hist_bytes, hipMemcpyDeviceToHost, st));
    }
    DYD_HIP(hipMemcpyAsync(out_boxes_per_image, d_bpi.p, 8 * K10_BPI, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
