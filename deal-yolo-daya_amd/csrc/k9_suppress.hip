// k9_suppress.hip — K9: greedy duplicate-box suppression inside each image row.
//
// For every box of a row: is there an EARLIER box of the same row, itself kept, whose IoU with this one reaches thr
// (optionally only among boxes with the same name id)?  Such a box is dropped (keep = 0) and `partner` names the first
// (lowest in-row index) kept box that hits it; otherwise keep = 1, partner = -1.  Annotations carry no scores, so annotation
// order decides — NMS with the row order as the ranking.  The pair arithmetic is K2's (k2_wave.h: normalise, pair_hits),
// evaluated as calculate_iou(earlier, later) (reference core/processor.py:328-339), so a NaN corner is handled like the IoU step.
//
// Layout in HBM: box4 = B x (p1x,p1y,p2x,p2y) f64 as scanned (16-B aligned), row_off = N+1 int32, name = B int32 or null;
// out_keep = B u8, out_partner = B int32.  Bytes: 32*B (+4*B with names) + 4*(N+1) in, 5*B out.
//
// Mapping.
//   Rows of at most 64 boxes (k9_tile_kernel): a wave owns K9_WROWS consecutive rows and packs whole rows into 64-lane tiles,
//   one box per lane.  A lane stages its normalised corners in LDS and builds a 64-bit mask of the earlier boxes of its own row
//   that hit it (bits at lane positions).  The rows of a tile sit on disjoint lane ranges, so one wave-wide `kept` mask resolves
//   all of them at once: at step s the lanes whose in-row index is s keep iff (hit & kept) == 0, then kept |= ballot(keep).
//   At most 64 ballot steps per tile, no workgroup barrier.
//   Rows above 64 boxes are pushed onto a list in device scratch (one int32 per row, at most B / 65 of them) and resolved by
//   k9_big_rows_kernel, one workgroup per row, in blocks of 64 boxes: (1) every box of the block is tested against the kept boxes
//   of the earlier blocks, whose decisions are final, spread over the workgroup's waves; (2) the block resolves itself with the
//   same ballot walk.  Exact for any row length, O(1) extra memory per row, never an n x n matrix.
#include "k2_wave.h"
#include "sized_out.h"

namespace dyd {

constexpr int K9_BLOCK = 256;
constexpr int K9_WAVES = K9_BLOCK / kWave;
constexpr int K9_WROWS = 16;   // image rows per wave

struct K9Lds {
    double x1[kWave], y1[kWave], x2[kWave], y2[kWave];
    int32_t name[kWave];
};

__device__ __forceinline__ Corners k9_load(const double *box4, int64_t b) {
    const double2 *g = reinterpret_cast<const double2 *>(box4 + 4 * b);
    return normalise(g[0], g[1]);
}

// calculate_iou(earlier, me) >= thr.  pair_hits' p is the lower-index box, q the higher one.
template <bool NO_NAN>
__device__ __forceinline__ bool k9_hits(const Corners &earlier, const Corners &me, double me_ar, double thr, double thr_lo,
                                        bool zero_hits) {
    double unused = 0.0;
    return pair_hits<false, NO_NAN>(earlier, me, me_ar, earlier, thr, thr_lo, zero_hits, unused);
}

// mask of the earlier boxes at lanes [rs, me_lane) of the LDS tile that hit `me`
template <bool NO_NAN>
__device__ __forceinline__ unsigned long long k9_hit_mask(const K9Lds &S, int rs, int me_lane, const Corners &me, int32_t me_name,
                                                          bool use_name, double thr, double thr_lo, bool zero_hits) {
    const double me_ar = area_of(me);
    unsigned long long hit = 0ull;
    for (int j = rs; j < me_lane; ++j) {
        if (use_name && S.name[j] != me_name) continue;
        const Corners o = {S.x1[j], S.y1[j], S.x2[j], S.y2[j]};
        if (k9_hits<NO_NAN>(o, me, me_ar, thr, thr_lo, zero_hits)) hit |= 1ull << j;
    }
    return hit;
}

__global__ __launch_bounds__(K9_BLOCK) void k9_tile_kernel(const double *__restrict__ box4, const int32_t *__restrict__ row_off,
                                                           int64_t n_rows, const int32_t *__restrict__ name, double thr,
                                                           uint8_t *__restrict__ out_keep, int32_t *__restrict__ out_partner,
                                                           int32_t *__restrict__ bigl, int32_t big_cap) {
    __shared__ K9Lds s_all[K9_WAVES];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    K9Lds &S = s_all[wave];
    const int64_t r0 = ((int64_t)blockIdx.x * K9_WAVES + wave) * K9_WROWS;
    if (r0 >= n_rows) return;
    const int nr = (n_rows - r0 < K9_WROWS) ? (int)(n_rows - r0) : K9_WROWS;
    const int32_t my_off = (lane <= nr) ? row_off[r0 + lane] : 0;   // lane L <= nr: offset of row r0 + L
    const bool zero_hits = (0.0 >= thr);                              // an empty intersection yields IoU 0.0 (:334-335)
    const double thr_lo = (thr > 0.0) ? thr * 0.999 : 0.0;
    const bool use_name = name != nullptr;

    int ra = 0;
    while (ra < nr) {   // wave-uniform
        const int32_t base = __builtin_amdgcn_readlane(my_off, ra);
        const unsigned long long fits = __ballot(lane > ra && lane <= nr && my_off - base <= kWave);
        const int taken = __popcll(fits);
        if (taken == 0) {   // row ra holds more than 64 boxes: k9_big_rows_kernel decides it
            if (lane == 0) {
                const int32_t slot = atomicAdd(&bigl[0], 1);
                if (slot < big_cap) bigl[1 + slot] = (int32_t)(r0 + ra);   // always true when n_boxes is right
            }
            ++ra;
            continue;
        }
        const int rb = ra + taken;
        const int nb = __builtin_amdgcn_readlane(my_off, rb) - base;   // <= 64 boxes in the tile
        // the lane's row: the last r in [ra, rb) with off[r] - base <= lane; rs = its first lane, n = its size
        int lr = ra, maxn = 0;
        for (int r = ra; r < rb; ++r) {
            const int32_t o = __builtin_amdgcn_readlane(my_off, r) - base;
            const int32_t n_r = __builtin_amdgcn_readlane(my_off, r + 1) - base - o;
            if (o <= lane) lr = r;
            maxn = (n_r > maxn) ? n_r : maxn;
        }
        const int rs = __shfl(my_off, lr) - base;
        const int n = __shfl(my_off, lr + 1) - base - rs;
        const bool valid = lane < nb;
        const int i = lane - rs;   // in-row index
        Corners me = {0.0, 0.0, 0.0, 0.0};
        int32_t me_name = 0;
        if (valid) {
            me = k9_load(box4, (int64_t)base + lane);
            S.x1[lane] = me.x1; S.y1[lane] = me.y1; S.x2[lane] = me.x2; S.y2[lane] = me.y2;
            if (use_name) { me_name = name[base + lane]; S.name[lane] = me_name; }
        }
        const unsigned long long nan_lanes = __ballot(valid && has_nan(me));
        wave_sync();
        unsigned long long hit = 0ull;
        if (valid && i > 0) {
            const unsigned long long row_mask = ((n >= 64) ? ~0ull : ((1ull << n) - 1ull)) << rs;
            hit = (nan_lanes & row_mask) ? k9_hit_mask<false>(S, rs, lane, me, me_name, use_name, thr, thr_lo, zero_hits)
                                         : k9_hit_mask<true>(S, rs, lane, me, me_name, use_name, thr, thr_lo, zero_hits);
        }
        // greedy walk: the lanes of in-row index s decide at step s, from the kept bits of their row's earlier lanes
        unsigned long long kept = 0ull;
        for (int s = 0; s < maxn; ++s) kept |= __ballot(valid && i == s && (hit & kept) == 0ull);
        if (valid) {
            const unsigned long long by = hit & kept;
            out_keep[base + lane] = (uint8_t)(by == 0ull);
            out_partner[base + lane] = by ? (__ffsll((long long)by) - 1) - rs : -1;
        }
        wave_sync();   // the next tile overwrites S
        ra = rb;
    }
}

// One workgroup per listed row (rows of more than 64 boxes), blocks of 64 boxes in row order.
__global__ __launch_bounds__(K9_BLOCK) void k9_big_rows_kernel(const double *__restrict__ box4, const int32_t *__restrict__ row_off,
                                                               const int32_t *__restrict__ name, double thr, uint8_t *out_keep,
                                                               int32_t *__restrict__ out_partner, const int32_t *__restrict__ bigl,
                                                               int32_t big_cap) {
    __shared__ K9Lds S;
    __shared__ int32_t first[kWave];   // lowest earlier-block kept box hitting block box l (INT32_MAX: none)
    __shared__ int row_nan;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const bool zero_hits = (0.0 >= thr);
    const double thr_lo = (thr > 0.0) ? thr * 0.999 : 0.0;
    const bool use_name = name != nullptr;
    const int32_t count = (bigl[0] < big_cap) ? bigl[0] : big_cap;
    for (int32_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int32_t r = bigl[1 + q];
        const int64_t base = row_off[r];
        const int32_t n = row_off[r + 1] - (int32_t)base;
        if (threadIdx.x == 0) row_nan = 0;
        __syncthreads();
        bool any_nan = false;
        for (int32_t k = threadIdx.x; k < n; k += K9_BLOCK) any_nan |= has_nan(k9_load(box4, base + k));
        if (any_nan) row_nan = 1;
        __syncthreads();
        const bool no_nan = row_nan == 0;
        for (int32_t b0 = 0; b0 < n; b0 += kWave) {
            const int bn = (n - b0 < kWave) ? n - b0 : kWave;
            const bool valid = lane < bn;
            Corners me = {0.0, 0.0, 0.0, 0.0};
            int32_t me_name = 0;
            if (valid) {
                me = k9_load(box4, base + b0 + lane);
                if (use_name) me_name = name[base + b0 + lane];
            }
            const double me_ar = area_of(me);
            if (wave == 0) first[lane] = INT32_MAX;
            __syncthreads();
            // (1) against the kept boxes of the earlier blocks: wave w takes j = w, w + 4, ...; the first hit is its lowest
            if (valid) {
                for (int32_t j = wave; j < b0; j += K9_WAVES) {
                    if (!out_keep[base + j]) continue;
                    if (use_name && name[base + j] != me_name) continue;
                    const Corners o = k9_load(box4, base + j);
                    if (no_nan ? k9_hits<true>(o, me, me_ar, thr, thr_lo, zero_hits)
                               : k9_hits<false>(o, me, me_ar, thr, thr_lo, zero_hits)) {
                        atomicMin(&first[lane], j);
                        break;
                    }
                }
            }
            __syncthreads();
            // (2) inside the block, wave 0 alone
            if (wave == 0) {
                const int32_t prior = first[lane];
                if (valid) {
                    S.x1[lane] = me.x1; S.y1[lane] = me.y1; S.x2[lane] = me.x2; S.y2[lane] = me.y2;
                    S.name[lane] = me_name;
                }
                wave_sync();
                unsigned long long hit = 0ull;
                if (valid && prior == INT32_MAX && lane > 0)
                    hit = no_nan ? k9_hit_mask<true>(S, 0, lane, me, me_name, use_name, thr, thr_lo, zero_hits)
                                 : k9_hit_mask<false>(S, 0, lane, me, me_name, use_name, thr, thr_lo, zero_hits);
                unsigned long long kept = 0ull;
                for (int s = 0; s < bn; ++s) kept |= __ballot(lane == s && prior == INT32_MAX && (hit & kept) == 0ull);
                if (valid) {
                    const unsigned long long by = hit & kept;
                    const bool keep = prior == INT32_MAX && by == 0ull;
                    out_keep[base + b0 + lane] = (uint8_t)keep;
                    out_partner[base + b0 + lane] = keep ? -1 : (prior != INT32_MAX ? prior : b0 + (__ffsll((long long)by) - 1));
                }
            }
            __syncthreads();   // the block's decisions are visible to every wave before the next block reads them
        }
    }
}

int launch_k9(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes, const int32_t *name, double thr,
              uint8_t *out_keep, int32_t *out_partner, hipStream_t st) {
    if (n_rows == 0) return DYD_OK;
    const int64_t blocks = ceil_div(n_rows, (int64_t)K9_WAVES * K9_WROWS);
    if (blocks > 0x7fffffffLL) {
        set_error("n_rows=%lld exceeds one launch", (long long)n_rows);
        return DYD_ERR_RANGE;
    }
    // rows above 64 boxes: at most n_boxes / 65 of them
    int64_t cap = n_boxes / (kWave + 1);
    cap = (cap < n_rows) ? cap : n_rows;
    ScratchLease lease(st);   // the list of big rows
    void *scratch = nullptr;
    int rc = lease.get(4 * (size_t)(cap + 1), &scratch);
    if (rc) return rc;
    int32_t *bigl = static_cast<int32_t *>(scratch);
    DYD_HIP(hipMemsetAsync(bigl, 0, 4, st));
    hipLaunchKernelGGL(k9_tile_kernel, dim3((unsigned)blocks), dim3(K9_BLOCK), 0, st, box4, row_off, n_rows, name, thr, out_keep,
                       out_partner, bigl, (int32_t)cap);
    DYD_HIP(hipGetLastError());
    if (cap > 0) {
        const int64_t want = (int64_t)ctx().num_cu * 4;
        hipLaunchKernelGGL(k9_big_rows_kernel, dim3((unsigned)(cap < want ? cap : want)), dim3(K9_BLOCK), 0, st, box4, row_off, name,
                           thr, out_keep, out_partner, bigl, (int32_t)cap);
        DYD_HIP(hipGetLastError());
    }
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_suppress_boxes_dev(const double *box4, const int32_t *row_off, int64_t n_rows, int64_t n_boxes, const int32_t *name_or_null,
                           double thr, uint8_t *out_keep, int32_t *out_partner, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_boxes >= 0, "n_rows < 0 or n_boxes < 0");
    DYD_REQUIRE(n_boxes < ((int64_t)1 << 31), "n_boxes exceeds int32 offsets");
    if (n_rows == 0 || n_boxes == 0) return DYD_OK;
    DYD_REQUIRE(row_off && out_keep && out_partner && box4, "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(box4) & 15) == 0, "box4 must be 16-byte aligned");
    return launch_k9(box4, row_off, n_rows, n_boxes, name_or_null, thr, out_keep, out_partner, pick_stream(stream));
}

int dyd_suppress_boxes(const double *box4, const int32_t *row_off, int64_t n_rows, const int32_t *name_or_null, double thr,
                       uint8_t *out_keep, int32_t *out_partner) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0, "n_rows < 0");
    if (n_rows == 0) return DYD_OK;
    DYD_REQUIRE(row_off, "null pointer");
    DYD_REQUIRE(row_off[0] == 0, "row_off[0] != 0");
    for (int64_t i = 0; i < n_rows; ++i) DYD_REQUIRE(row_off[i + 1] >= row_off[i], "row_off not monotone");
    const int64_t nb = row_off[n_rows];
    if (nb == 0) return DYD_OK;
    DYD_REQUIRE(box4 && out_keep && out_partner, "null pointer");
    DevBuf d_box, d_off, d_name, d_keep, d_partner;
    int rc;
    if ((rc = d_box.alloc(32 * (size_t)nb)) || (rc = d_off.alloc(4 * (size_t)(n_rows + 1))) || (rc = d_keep.alloc((size_t)nb)) ||
        (rc = d_partner.alloc(4 * (size_t)nb)))
        return rc;
    if (name_or_null && (rc = d_name.alloc(4 * (size_t)nb))) return rc;
    hipStream_t st = ctx().stream;
    DYD_HIP(hipMemcpyAsync(d_box.p, box4, 32 * (size_t)nb, hipMemcpyHostToDevice, st));
    DYD_HIP(hipMemcpyAsync(d_off.p, row_off, 4 * (size_t)(n_rows + 1), hipMemcpyHostToDevice, st));
    if (name_or_null) DYD_HIP(hipMemcpyAsync(d_name.p, name_or_null, 4 * (size_t)nb, hipMemcpyHostToDevice, st));
    KernelTimer t(st);
    rc = launch_k9(d_box.as<double>(), d_off.as<int32_t>(), n_rows, nb, name_or_null ? d_name.as<int32_t>() : nullptr, thr,
                   d_keep.as<uint8_t>(), d_partner.as<int32_t>(), st);
    if (rc) return rc;
    t.finish();
    DYD_HIP(hipMemcpyAsync(out_keep, d_keep.p, (size_t)nb, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_partner, d_partner.p, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
