// k11_repair.hip — K11: per-box repair decision of an annotation table (the box repair step).
//
// For every box: one action code, the corners it will be written with, and exact integer counts per image row and per class.
// The rules are tested in order, in IEEE f64 with no contraction, on the box audit's boxes (K10's inputs):
//     2 no_size         the row's size_status is not 0                                    -> box untouched
//     3 bad_coords      a corner is not finite                                            -> object removed
//     4 degenerate      max(x2 - x1, 0) <= 0 or max(y2 - y1, 0) <= 0                       -> object removed
//       clip            x1' = 0 if x1 < 0 else x1, y1' likewise, x2' = W if x2 > W else x2, y2' = H if y2 > H else y2,
//                       bw' = max(x2' - x1', 0), bh' likewise, clipped = x1 < 0 or y1 < 0 or x2 > W or y2 > H
//     5 outside         bw' <= 0 or bh' <= 0                                              -> object removed
//     6 low_visibility  bw' * bh' < min_visibility * (bw * bh), bw = x2 - x1, bh = y2 - y1  -> object removed
//     7 small           bw' < min_size or bh' < min_size                                  -> object removed
//     1 clip            clipped                                                           -> ptList replaced by (x1', y1', x2', y2')
//     0 keep            otherwise                                                         -> box untouched
//
// Layout in HBM: box4 = B x (x1, y1, x2, y2) f64 (16-B aligned), row_off = N+1 int32, cls = B int32 (-1 or out of range: the name
// is no str, the box is counted per row only), width / height = N f64, size_status = N u8 (0 ok, 1 missing, 2 invalid).
// Out: action = B u8 (code in bits 0-2, 0x80 for class id -1), box4 = B x 4 f64 (16-B aligned; clipped corners for code 1, the
// input corners otherwise), row_counts = N x 8 int32, class_counts = C x 8 int64 (both indexed by action code).
//
// Mapping: K10's.  A persistent grid; a wave takes tiles of K11_WROWS consecutive rows (lane L holds the offset, size and status
// of row r0 + L) and walks the tile's boxes 64 at a time, one box per lane; a lane finds its row by a 5-step binary search over
// the lane offsets.  Accumulation, Guideline 12 style — reduce on chip, then one atomic per destination:
//   - per-row counts: LDS counters of the wave's tile (a tile's rows belong to one wave), stored once per tile;
//   - per-class counts: eight wave-wide ballots (one per action) per 64 boxes, then a match-any walk over the class ids
//     (leader's class -> ballot of equal lanes -> popcount of its AND with each action ballot, all on the scalar unit) and one add
//     per (class, action) into the block's LDS copy when C <= K11_LDS_CLASSES, else one u64 global atomic.
#include "box_table.h"

namespace dyd {

constexpr int K11_BLOCK = 512;
constexpr int K11_WAVES = K11_BLOCK / kWave;
constexpr int K11_WROWS = 32;               // image rows per wave tile
constexpr int K11_ACT = 8;                  // action codes = counters per row and per class
constexpr int K11_LDS_CLASSES = 256;
constexpr uint8_t K11_UNMATCHABLE = 0x80;

struct K11Shared {
    uint32_t cls_cnt[K11_LDS_CLASSES * K11_ACT];
    uint32_t rowc[K11_WAVES][K11_WROWS * K11_ACT];
};

__global__ __launch_bounds__(K11_BLOCK) void k11_repair_kernel(const double *__restrict__ box4, const int32_t *__restrict__ row_off,
                                                               int64_t n_rows, const int32_t *__restrict__ cls,
                                                               const double *__restrict__ width, const double *__restrict__ height,
                                                               const uint8_t *__restrict__ size_status, int32_t n_classes,
                                                               double min_vis, double min_size, uint8_t *__restrict__ out_action,
                                                               double *__restrict__ out_box4, int32_t *__restrict__ out_rows,
                                                               int64_t *__restrict__ out_cls) {
    __shared__ K11Shared S;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const bool lds_cls = n_classes <= K11_LDS_CLASSES;
    if (lds_cls)
        for (int k = threadIdx.x; k < n_classes * K11_ACT; k += K11_BLOCK) S.cls_cnt[k] = 0u;
    __syncthreads();

    uint32_t *rowc = S.rowc[wave];
    const int64_t n_tiles = (n_rows + K11_WROWS - 1) / K11_WROWS;
    for (int64_t tile = (int64_t)blockIdx.x * K11_WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * K11_WAVES) {
        const int64_t r0 = tile * K11_WROWS;
        const int nr = (n_rows - r0 < K11_WROWS) ? (int)(n_rows - r0) : K11_WROWS;
        const int32_t my_off = (lane <= nr) ? row_off[r0 + lane] : 0;
        double my_w = 0.0, my_h = 0.0;
        int my_st = 1;
        if (lane < nr) {
            my_st = size_status[r0 + lane];
            my_w = width[r0 + lane];
            my_h = height[r0 + lane];
        }
        for (int k = lane; k < K11_WROWS * K11_ACT; k += kWave) rowc[k] = 0u;
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
            const double W = __shfl(my_w, r);
            const double H = __shfl(my_h, r);
            const int st = __shfl(my_st, r);

            int32_t c = -1;
            int act = 0;
            if (valid) {
                c = cls[b];
                if (c < 0 || c >= n_classes) c = -1;
                const double2 *g = reinterpret_cast<const double2 *>(box4 + 4 * (int64_t)b);
                double2 p = g[0], q = g[1];
                const double x1 = p.x, y1 = p.y, x2 = q.x, y2 = q.y;
                if (st != 0) {
                    act = 2;
                } else if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) {
                    act = 3;
                } else {
                    const double bw = x2 - x1, bh = y2 - y1;
                    if (((0.0 > bw) ? 0.0 : bw) <= 0.0 || ((0.0 > bh) ? 0.0 : bh) <= 0.0) {   // max(v, 0.0) <= 0
                        act = 4;
                    } else {
                        const double cx1 = (x1 < 0.0) ? 0.0 : x1, cy1 = (y1 < 0.0) ? 0.0 : y1;
                        const double cx2 = (x2 > W) ? W : x2, cy2 = (y2 > H) ? H : y2;
                        const double dx = cx2 - cx1, dy = cy2 - cy1;
                        const double cw = (0.0 > dx) ? 0.0 : dx, ch = (0.0 > dy) ? 0.0 : dy;
                        const bool clipped = x1 < 0.0 || y1 < 0.0 || x2 > W || y2 > H;
                        if (cw <= 0.0 || ch <= 0.0) act = 5;
                        else if (cw * ch < min_vis * (bw * bh)) act = 6;
                        else if (cw < min_size || ch < min_size) act = 7;
                        else if (clipped) act = 1;
                        else act = 0;
                        if (act == 1) {
                            p.x = cx1; p.y = cy1;
                            q.x = cx2; q.y = cy2;
                        }
                    }
                }
                double2 *o = reinterpret_cast<double2 *>(out_box4 + 4 * (int64_t)b);
                o[0] = p;
                o[1] = q;
                out_action[b] = (uint8_t)(act | (c < 0 ? K11_UNMATCHABLE : 0));
                atomicAdd(&rowc[r * K11_ACT + act], 1u);
            }
            // per-class counts: one group of equal class ids at a time, against the eight per-action ballots
            const bool counted = valid && c >= 0;
            unsigned long long am[K11_ACT];
#pragma unroll
            for (int k = 0; k < K11_ACT; ++k) am[k] = __ballot(counted && act == k);
            unsigned long long pending = __ballot(counted);
            while (pending) {
                const int leader = __ffsll((long long)pending) - 1;
                const int32_t gc = __builtin_amdgcn_readlane(c, leader);
                const unsigned long long grp = __ballot(counted && c == gc);
                pending &= ~grp;
                uint32_t mine = 0u;
#pragma unroll
                for (int k = 0; k < K11_ACT; ++k) {
                    const uint32_t n = (uint32_t)__popcll(am[k] & grp);
                    if (lane == k) mine = n;
                }
                if (lane < K11_ACT && mine) {
                    if (lds_cls) atomicAdd(&S.cls_cnt[gc * K11_ACT + lane], mine);
                    else atomicAdd(reinterpret_cast<unsigned long long *>(out_cls + (int64_t)gc * K11_ACT + lane),
                                   (unsigned long long)mine);
                }
            }
        }
        box_wave_sync();
        for (int k = lane; k < nr * K11_ACT; k += kWave) out_rows[r0 * K11_ACT + k] = (int32_t)rowc[k];
        box_wave_sync();   // the next tile clears rowc
    }

    if (lds_cls) {
        __syncthreads();
        for (int k = threadIdx.x; k < n_classes * K11_ACT; k += K11_BLOCK)
            if (S.cls_cnt[k]) atomicAdd(reinterpret_cast<unsigned long long *>(out_cls + k), (unsigned long long)S.cls_cnt[k]);
    }
}

int launch_k11(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls, const double *width,
               const double *height, const uint8_t *size_status, int32_t n_classes, double min_vis, double min_size,
               uint8_t *out_action, double *out_box4, int32_t *out_rows, int64_t *out_cls, hipStream_t st) {
    if (n_classes > 0) DYD_HIP(hipMemsetAsync(out_cls, 0, 8 * (size_t)n_classes * K11_ACT, st));
    if (n_rows == 0) return DYD_OK;
    const int64_t tiles = ceil_div(n_rows, (int64_t)K11_WROWS);
    const int64_t want = (int64_t)ctx().num_cu * 3;   // 75 VGPRs: 6 waves per SIMD = three resident 512-thread workgroups per CU
    const int64_t need = ceil_div(tiles, (int64_t)K11_WAVES);
    const unsigned blocks = (unsigned)(need < want ? need : want);
    hipLaunchKernelGGL(k11_repair_kernel, dim3(blocks), dim3(K11_BLOCK), 0, st, box4, row_off, n_rows, cls, width, height,
                       size_status, n_classes, min_vis, min_size, out_action, out_box4, out_rows, out_cls);
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_repair_boxes_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes, const int32_t *cls,
                         const double *width, const double *height, const uint8_t *size_status, int32_t n_classes,
                         double min_visibility, double min_size, uint8_t *out_action, double *out_box4, int32_t *out_row_counts,
                         int64_t *out_class_counts, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_boxes >= 0 && n_classes >= 0, "n_rows, n_boxes or n_classes < 0");
    DYD_REQUIRE(min_visibility >= 0.0 && min_visibility <= 1.0, "min_visibility must lie in [0, 1]");
    DYD_REQUIRE(std::isfinite(min_size) && min_size >= 0.0, "min_size must be finite and >= 0");
    DYD_REQUIRE(n_boxes < ((int64_t)1 << 31), "n_boxes exceeds int32 offsets");
    DYD_REQUIRE(n_classes == 0 || out_class_counts, "null pointer");
    DYD_REQUIRE(n_rows == 0 || (row_off && width && height && size_status && out_row_counts), "null pointer");
    DYD_REQUIRE(n_boxes == 0 || (box4 && cls && out_action && out_box4), "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(box4) & 15) == 0 && (reinterpret_cast<uintptr_t>(out_box4) & 15) == 0,
                "box4 and out_box4 must be 16-byte aligned");
    return launch_k11(box4, row_off, n_rows, cls, width, height, size_status, n_classes, min_visibility, min_size, out_action,
                      out_box4, out_row_counts, out_class_counts, pick_stream(stream));
}

int dyd_repair_boxes(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *cls, const double *width,
                     const double *height, const uint8_t *size_status, int32_t n_classes, double min_visibility, double min_size,
                     uint8_t *out_action, double *out_box4, int32_t *out_row_counts, int64_t *out_class_counts) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_classes >= 0, "n_rows < 0 or n_classes < 0");
    DYD_REQUIRE(min_visibility >= 0.0 && min_visibility <= 1.0, "min_visibility must lie in [0, 1]");
    DYD_REQUIRE(std::isfinite(min_size) && min_size >= 0.0, "min_size must be finite and >= 0");
    DYD_REQUIRE(n_classes == 0 || out_class_counts, "null pointer");
    int64_t nb;
    int rc;
    if ((rc = box_table_check(box4, row_off, n_rows, cls, width, height, size_status, n_classes, out_row_counts != nullptr,
                              out_action && out_box4, &nb)))
        return rc;
    BoxTableDev d;
    if ((rc = d.upload(box4, row_off, n_rows, cls, width, height, size_status, nb))) return rc;
    DevBuf d_act, d_obox, d_rows, d_cc;
    if ((rc = d_act.alloc((size_t)nb)) || (rc = d_obox.alloc(32 * (size_t)nb)) || (rc = d_rows.alloc(4 * K11_ACT * (size_t)n_rows)) ||
        (rc = d_cc.alloc(8 * K11_ACT * (size_t)n_classes)))
        return rc;
    hipStream_t st = ctx().stream;
    KernelTimer t(st);
    rc = launch_k11(d.box.as<double>(), d.off.as<int32_t>(), n_rows, d.cls.as<int32_t>(), d.w.as<double>(), d.h.as<double>(),
                    d.st.as<uint8_t>(), n_classes, min_visibility, min_size, d_act.as<uint8_t>(), d_obox.as<double>(),
                    d_rows.as<int32_t>(), d_cc.as<int64_t>(), st);
    if (rc) return rc;
    t.finish();
    if (nb) {
        DYD_HIP(hipMemcpyAsync(out_action, d_act.p, (size_t)nb, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_box4, d_obox.p, 32 * (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    if (n_rows) DYD_HIP(hipMemcpyAsync(out_row_counts, d_rows.p, 4 * K11_ACT * (size_t)n_rows, hipMemcpyDeviceToHost, st));
    if (n_classes) DYD_HIP(hipMemcpyAsync(out_class_counts, d_cc.p, 8 * K11_ACT * (size_t)n_classes, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
