// k18_compare.hip — K18: match two box tables of the same image rows (greedy bipartite matching per row).
//
// Tables A ("base") and B ("other") cover the same rows.  Per row the B boxes are taken in annotation order; B box j takes the
// still unmatched A box i (of equal class id when by_label) with the largest calculate_iou(a_i, b_j) >= thr, ties to the lowest
// i, or stays unmatched.  a_best / b_best are the largest IoU of a box with ANY box of the other side (class and matched state
// ignored; folded by `iou > best` from 0.0, so a NaN IoU never raises them).  The pair arithmetic is K2's (k2_wave.h: normalise,
// area_of, reference core/processor.py:328-339 in exact f64, compare/select with a NaN corner about), the A box first.  Full
// semantics: include/dyd.h.
//
// Layout in HBM, per table: box4 = B x (p1x,p1y,p2x,p2y) f64 as scanned (16-B aligned), row_off = N+1 int32, cls = B int32.
// Bytes: 36 per box and 4 per row and table in; 12 per A box, 20 per B box, 16 per row and 8 (C+1)^2 out.
//
// Mapping.
//   k18_tile_kernel: a wave owns K18_WROWS consecutive rows and packs whole rows into tiles of at most 64 A boxes (one per lane)
//   and K18_BCAP B boxes (staged in the wave's LDS slice with their results).  At step s every row of the tile takes its B box s:
//   the rows sit on disjoint lane ranges, so the row's arg-max is a segmented suffix-max over the lanes (shuffles) on the IoU's
//   bit pattern (IoU >= 0 orders like its u64 bits; candidates carry bits + 1, 0 = no candidate) and the lowest lane among the
//   maxima comes from a ballot masked to the row's lanes.  The matched state is the lane's own a_match.  No workgroup barrier
//   in the walk; at most K18_BCAP steps per tile.  The kernel is persistent: the waves stride over the groups of rows.
//   A row that does not fit a tile (more than 64 A boxes or more than K18_BCAP B boxes) is pushed onto a list in device scratch
//   and taken by k18_big_rows_kernel, one workgroup per row: the A boxes strided over the 256 lanes, the B boxes in order, each
//   with a block-wide arg-max through LDS (one barrier per B box).  The matched state lives in out_a_match, which only the
//   lane that owns the A box reads and writes.  Exact for any row length, O(na * nb) IoUs, never an na x nb matrix.
//   Confusion counts: per workgroup in LDS (u32) while (C+1)^2 <= K18_CONF_LDS, flushed with one u64 atomic per non-zero cell;
//   global u64 atomics otherwise and in the big-row kernel.  The counts do not depend on the order.
//   The exact IoU of every candidate is needed, so K2's rejecting bound (thr_lo) is not used here.
#include "k18_pick.h"
#include "sized_out.h"

namespace dyd {

constexpr int K18_BLOCK = 256;
constexpr int K18_WAVES = K18_BLOCK / kWave;
constexpr int K18_WROWS = 16;        // image rows per wave and group
constexpr int K18_BCAP = 128;        // B boxes staged per tile
constexpr int K18_CONF_LDS = 1024;   // (C+1)^2 cells counted in LDS (C <= 31)

struct K18Lds {
    double x1[K18_BCAP], y1[K18_BCAP], x2[K18_BCAP], y2[K18_BCAP];
    double iou[K18_BCAP], best[K18_BCAP];
    int32_t cls[K18_BCAP], match[K18_BCAP];
};

// k18_count in the workgroup's LDS copy of the matrix when there is one
__device__ __forceinline__ void k18_count(unsigned int *lds_conf, unsigned long long *conf, int32_t C, int32_t a, int32_t b) {
    if ((uint32_t)a > (uint32_t)C || (uint32_t)b > (uint32_t)C) return;
    const int64_t cell = (int64_t)a * (C + 1) + b;
    if (lds_conf) atomicAdd(&lds_conf[cell], 1u);
    else atomicAdd(&conf[cell], 1ull);
}
__device__ __forceinline__ int32_t k18_class(int32_t c, int32_t C) { return ((uint32_t)c < (uint32_t)C) ? c : -1; }

__device__ __forceinline__ unsigned long long k18_lane_mask(int first, int width) {   // lanes [first, first + width), width <= 64
    if (width <= 0) return 0ull;
    return ((width >= 64) ? ~0ull : ((1ull << width) - 1ull)) << first;
}

__global__ __launch_bounds__(K18_BLOCK) void k18_tile_kernel(
    const double *__restrict__ a_box4, const int32_t *__restrict__ a_off, const int32_t *__restrict__ a_cls,
    const double *__restrict__ b_box4, const int32_t *__restrict__ b_off, const int32_t *__restrict__ b_cls, int64_t n_rows,
    int32_t C, double thr, int by_label, int32_t *__restrict__ out_a_match, int32_t *__restrict__ out_b_match,
    double *__restrict__ out_b_iou, double *__restrict__ out_a_best, double *__restrict__ out_b_best,
    int32_t *__restrict__ out_rows, unsigned long long *__restrict__ out_conf, int32_t *__restrict__ bigl, int32_t big_cap) {
    __shared__ K18Lds s_all[K18_WAVES];
    __shared__ unsigned int s_conf[K18_CONF_LDS];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    K18Lds &S = s_all[wave];
    const int64_t cells = (int64_t)(C + 1) * (C + 1);
    unsigned int *lds_conf = (cells <= K18_CONF_LDS) ? s_conf : nullptr;
    if (lds_conf) {
        for (int k = threadIdx.x; k < (int)cells; k += K18_BLOCK) s_conf[k] = 0u;
        __syncthreads();
    }

    const int64_t groups = (n_rows + K18_WROWS - 1) / K18_WROWS;
    for (int64_t g = (int64_t)blockIdx.x * K18_WAVES + wave; g < groups; g += (int64_t)gridDim.x * K18_WAVES) {
        const int64_t r0 = g * K18_WROWS;
        const int nr = (n_rows - r0 < K18_WROWS) ? (int)(n_rows - r0) : K18_WROWS;
        const int32_t my_a = (lane <= nr) ? a_off[r0 + lane] : 0;   // lane L <= nr: offsets of row r0 + L
        const int32_t my_b = (lane <= nr) ? b_off[r0 + lane] : 0;

        int ra = 0;
        while (ra < nr) {   // wave-uniform
            const int32_t a_base = __builtin_amdgcn_readlane(my_a, ra);
            const int32_t b_base = __builtin_amdgcn_readlane(my_b, ra);
            const unsigned long long fits =
                __ballot(lane > ra && lane <= nr && my_a - a_base <= kWave && my_b - b_base <= K18_BCAP);
            const int taken = __popcll(fits);
            if (taken == 0) {   // row ra fits no tile: k18_big_rows_kernel takes it
                if (lane == 0) {
                    const int32_t slot = atomicAdd(&bigl[0], 1);
                    if (slot < big_cap) bigl[1 + slot] = (int32_t)(r0 + ra);   // always true when n_a and n_b are right
                }
                ++ra;
                continue;
            }
            const int rb = ra + taken;
            const int tna = __builtin_amdgcn_readlane(my_a, rb) - a_base;   // <= 64 A boxes in the tile
            const int tnb = __builtin_amdgcn_readlane(my_b, rb) - b_base;   // <= K18_BCAP B boxes
            // the lane's row: the last r in [ra, rb) whose first lane is <= lane; maxn / maxnb over the rows holding A boxes
            int lr = ra, maxn = 0, maxnb = 0;
            for (int r = ra; r < rb; ++r) {
                const int32_t o = __builtin_amdgcn_readlane(my_a, r) - a_base;
                const int32_t n_r = __builtin_amdgcn_readlane(my_a, r + 1) - a_base - o;
                const int32_t nb_r = __builtin_amdgcn_readlane(my_b, r + 1) - __builtin_amdgcn_readlane(my_b, r);
                if (o <= lane) lr = r;
                if (n_r > 0) {
                    maxn = (n_r > maxn) ? n_r : maxn;
                    maxnb = (nb_r > maxnb) ? nb_r : maxnb;
                }
            }
            const bool valid = lane < tna;
            const int32_t lr_a0 = __shfl(my_a, lr), lr_a1 = __shfl(my_a, lr + 1);   // every lane takes part in the shuffles
            const int32_t lr_b0 = __shfl(my_b, lr), lr_b1 = __shfl(my_b, lr + 1);
            const int rs = valid ? lr_a0 - a_base : lane;     // first lane of the row
            const int n = valid ? lr_a1 - lr_a0 : 0;          // its A boxes
            const int b_rs = lr_b0 - b_base;                  // its first staged B box
            const int nbr = valid ? lr_b1 - lr_b0 : 0;
            const int rend = rs + n;
            const unsigned long long row_mask = k18_lane_mask(rs, n);

            Corners me = {0.0, 0.0, 0.0, 0.0};
            int32_t me_cls = 0;
            if (valid) {
                me = k18_load(a_box4, (int64_t)a_base + lane);
                me_cls = a_cls[a_base + lane];
            }
            const double me_ar = area_of(me);
            bool nan_here = valid && has_nan(me);
            for (int k = lane; k < tnb; k += kWave) {   // stage the tile's B boxes with the results of an unmatched box
                const Corners v = k18_load(b_box4, (int64_t)b_base + k);
                S.x1[k] = v.x1; S.y1[k] = v.y1; S.x2[k] = v.x2; S.y2[k] = v.y2;
                S.cls[k] = b_cls[b_base + k];
                S.match[k] = -1;
                S.iou[k] = 0.0;
                S.best[k] = 0.0;
                nan_here |= has_nan(v);
            }
            const bool no_nan = __ballot(nan_here) == 0ull;   // a NaN corner anywhere in the tile: the ordered compare/select path
            wave_sync();

            int32_t a_match = -1;
            double best = 0.0;
            for (int s = 0; s < maxnb; ++s) {
                const bool act = valid && s < nbr;   // the same for every lane of a row
                const int k = b_rs + s;
                unsigned long long mine = 0ull, bk = 0ull;
                if (act) {
                    const Corners o = {S.x1[k], S.y1[k], S.x2[k], S.y2[k]};
                    const double iou = no_nan ? k18_iou<true>(me, o, me_ar) : k18_iou<false>(me, o, me_ar);
                    if (iou > best) best = iou;
                    bk = k18_best_key(iou);
                    if (a_match < 0 && (!by_label || S.cls[k] == me_cls) && iou >= thr) mine = k18_cand_key(iou);
                }
                // segmented suffix-max over the lanes of each row; the row's first lane ends with the row's maxima
                unsigned long long ck = mine;
                for (int d = 1; d < maxn; d <<= 1) {
                    const unsigned long long oc = __shfl_down(ck, d);
                    const unsigned long long ob = __shfl_down(bk, d);
                    if (lane + d < rend) {
                        ck = (oc > ck) ? oc : ck;
                        bk = (ob > bk) ? ob : bk;
                    }
                }
                const unsigned long long row_c = __shfl(ck, rs);
                const unsigned long long row_b = __shfl(bk, rs);
                const unsigned long long win = __ballot(act && mine != 0ull && mine == row_c) & row_mask;
                const int first = __ffsll((long long)win) - 1;   // the lowest lane among the row's maxima, -1: no candidate
                if (act && lane == first) a_match = s;
                if (act && lane == rs) {
                    S.match[k] = (first >= 0) ? first - rs : -1;
                    S.iou[k] = (first >= 0) ? k18_value(row_c - 1ull) : 0.0;
                    S.best[k] = k18_value(row_b);
                }
            }
            wave_sync();

            // A side, confusion of the A boxes, per-row counts
            const bool matched = valid && a_match >= 0;
            const int32_t o_cls = matched ? S.cls[b_rs + a_match] : 0;
            const unsigned long long m_all = __ballot(matched);
            const unsigned long long m_same = __ballot(matched && o_cls == me_cls);
            if (valid) {
                out_a_match[a_base + lane] = a_match;
                out_a_best[a_base + lane] = best;
                k18_count(lds_conf, out_conf, C, k18_class(me_cls, C), matched ? k18_class(o_cls, C) : C);
            }
            for (int k = lane; k < tnb; k += kWave) {
                const int32_t m = S.match[k];
                out_b_match[b_base + k] = m;
                out_b_iou[b_base + k] = S.iou[k];
                out_b_best[b_base + k] = S.best[k];
                if (m < 0) k18_count(lds_conf, out_conf, C, C, k18_class(S.cls[k], C));
            }
            {
                const int R = (ra + lane < rb) ? ra + lane : ra;   // lane t < rb - ra writes the counts of row ra + t
                const int o0 = __shfl(my_a, R) - a_base;
                const int na_r = __shfl(my_a, R + 1) - a_base - o0;
                const int nb_r = __shfl(my_b, R + 1) - __shfl(my_b, R);
                const unsigned long long mask = k18_lane_mask(o0, na_r);
                const int same = __popcll(m_same & mask);
                const int all = __popcll(m_all & mask);
                if (ra + lane < rb) {
                    int32_t *o = out_rows + 4 * (r0 + R);
                    o[0] = same;
                    o[1] = all - same;
                    o[2] = na_r - all;
                    o[3] = nb_r - all;
                }
            }
            wave_sync();   // the next tile overwrites S
            ra = rb;
        }
    }

    if (lds_conf) {
        __syncthreads();
        for (int k = threadIdx.x; k < (int)cells; k += K18_BLOCK)
            if (s_conf[k]) atomicAdd(&out_conf[k], (unsigned long long)s_conf[k]);
    }
}

// arg-max of one wave: the largest key, the lowest A index among the lanes holding it, the largest best key
struct K18Pick {
    unsigned long long key;
    unsigned long long best;
    int32_t idx;
};

// One workgroup per listed row.  Lane t owns the A boxes t, t + 256, ...; B boxes in order, one barrier each.
__global__ __launch_bounds__(K18_BLOCK) void k18_big_rows_kernel(
    const double *__restrict__ a_box4, const int32_t *__restrict__ a_off, const int32_t *__restrict__ a_cls,
    const double *__restrict__ b_box4, const int32_t *__restrict__ b_off, const int32_t *__restrict__ b_cls, int32_t C,
    double thr, int by_label, int32_t *out_a_match, int32_t *__restrict__ out_b_match, double *__restrict__ out_b_iou,
    double *out_a_best, double *__restrict__ out_b_best, int32_t *__restrict__ out_rows, unsigned long long *__restrict__ out_conf,
    const int32_t *__restrict__ bigl, int32_t big_cap) {
    __shared__ K18Lds S;                       // K18_BCAP B boxes at a time (iou / best / match unused)
    __shared__ K18Pick pick[2][K18_WAVES];     // per B box, taking turns
    __shared__ int row_nan;
    __shared__ int cnt[2];                     // matched with equal class, matched with different class
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int32_t count = (bigl[0] < big_cap) ? bigl[0] : big_cap;
    for (int32_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int32_t r = bigl[1 + q];
        const int64_t a_base = a_off[r], b_base = b_off[r];
        const int32_t na = a_off[r + 1] - (int32_t)a_base;
        const int32_t nb = b_off[r + 1] - (int32_t)b_base;
        if (threadIdx.x == 0) {
            row_nan = 0;
            cnt[0] = 0;
            cnt[1] = 0;
        }
        __syncthreads();
        bool any_nan = false;
        for (int32_t i = threadIdx.x; i < na; i += K18_BLOCK) {
            any_nan |= has_nan(k18_load(a_box4, a_base + i));
            out_a_match[a_base + i] = -1;
            out_a_best[a_base + i] = 0.0;
        }
        for (int32_t j = threadIdx.x; j < nb; j += K18_BLOCK) any_nan |= has_nan(k18_load(b_box4, b_base + j));
        if (any_nan) row_nan = 1;
        __syncthreads();
        const bool no_nan = row_nan == 0;
        int same = 0, diff = 0;

        for (int32_t j0 = 0; j0 < nb; j0 += K18_BCAP) {
            const int jn = (nb - j0 < K18_BCAP) ? nb - j0 : K18_BCAP;
            __syncthreads();   // the previous piece is done with S
            if ((int)threadIdx.x < jn) {
                const int k = threadIdx.x;
                const Corners v = k18_load(b_box4, b_base + j0 + k);
                S.x1[k] = v.x1; S.y1[k] = v.y1; S.x2[k] = v.x2; S.y2[k] = v.y2;
                S.cls[k] = b_cls[b_base + j0 + k];
            }
            __syncthreads();
            for (int k = 0; k < jn; ++k) {
                const int32_t j = j0 + k;
                const Corners o = {S.x1[k], S.y1[k], S.x2[k], S.y2[k]};
                const int32_t o_cls = S.cls[k];
                unsigned long long key = 0ull, bk = 0ull;
                int32_t idx = INT32_MAX;
                for (int32_t i = threadIdx.x; i < na; i += K18_BLOCK) {   // ascending: the first of equal keys stays
                    const Corners me = k18_load(a_box4, a_base + i);
                    const double me_ar = area_of(me);
                    const double iou = no_nan ? k18_iou<true>(me, o, me_ar) : k18_iou<false>(me, o, me_ar);
                    if (iou > out_a_best[a_base + i]) out_a_best[a_base + i] = iou;
                    const unsigned long long b1 = k18_best_key(iou);
                    bk = (b1 > bk) ? b1 : bk;
                    if (out_a_match[a_base + i] < 0 && (!by_label || a_cls[a_base + i] == o_cls) && iou >= thr) {
                        const unsigned long long c1 = k18_cand_key(iou);
                        if (c1 > key) {
                            key = c1;
                            idx = i;
                        }
                    }
                }
                // the wave's arg-max: largest key, then the lowest A index among its holders
                unsigned long long wk = key, wb = bk;
                for (int d = 32; d >= 1; d >>= 1) {
                    const unsigned long long oc = __shfl_xor(wk, d);
                    const unsigned long long ob = __shfl_xor(wb, d);
                    wk = (oc > wk) ? oc : wk;
                    wb = (ob > wb) ? ob : wb;
                }
                int32_t wi = (key == wk && key != 0ull) ? idx : INT32_MAX;
                for (int d = 32; d >= 1; d >>= 1) {
                    const int32_t oi = __shfl_xor(wi, d);
                    wi = (oi < wi) ? oi : wi;
                }
                K18Pick *slot = pick[j & 1];
                if (lane == 0) {
                    slot[wave].key = wk;
                    slot[wave].best = wb;
                    slot[wave].idx = wi;
                }
                __syncthreads();
                unsigned long long gk = 0ull, gb = 0ull;
                int32_t gi = INT32_MAX;
                for (int w = 0; w < K18_WAVES; ++w) {
                    const K18Pick p = slot[w];
                    gb = (p.best > gb) ? p.best : gb;
                    if (p.key > gk || (p.key == gk && p.key != 0ull && p.idx < gi)) {
                        gk = p.key;
                        gi = p.idx;
                    }
                }
                const bool hit = gk != 0ull;
                if (hit && (gi % K18_BLOCK) == (int32_t)threadIdx.x) {   // the owner of the matched A box
                    out_a_match[a_base + gi] = j;
                    const int32_t mc = a_cls[a_base + gi];
                    if (mc == o_cls) ++same; else ++diff;
                    k18_count(out_conf, C, k18_class(mc, C), k18_class(o_cls, C));
                }
                if (threadIdx.x == 0) {
                    out_b_match[b_base + j] = hit ? gi : -1;
                    out_b_iou[b_base + j] = hit ? k18_value(gk - 1ull) : 0.0;
                    out_b_best[b_base + j] = k18_value(gb);
                    if (!hit) k18_count(out_conf, C, C, k18_class(o_cls, C));
                }
            }
        }
        for (int32_t i = threadIdx.x; i < na; i += K18_BLOCK)
            if (out_a_match[a_base + i] < 0) k18_count(out_conf, C, k18_class(a_cls[a_base + i], C), C);
        if (same) atomicAdd(&cnt[0], same);
        if (diff) atomicAdd(&cnt[1], diff);
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t *o = out_rows + 4 * (int64_t)r;
            o[0] = cnt[0];
            o[1] = cnt[1];
            o[2] = na - cnt[0] - cnt[1];
            o[3] = nb - cnt[0] - cnt[1];
        }
        __syncthreads();   // cnt is cleared for the next row
    }
}

int launch_k18(const double *a_box4, const int32_t *a_off, const int32_t *a_cls, const double *b_box4, const int32_t *b_off,
               const int32_t *b_cls, int64_t n_rows, int64_t n_a, int64_t n_b, int32_t n_classes, double thr, int by_label,
               int32_t *out_a_match, int32_t *out_b_match, double *out_b_iou, double *out_a_best, double *out_b_best,
               int32_t *out_rows, uint64_t *out_conf, hipStream_t st) {
    const size_t cells = (size_t)(n_classes + 1) * (size_t)(n_classes + 1);
    DYD_HIP(hipMemsetAsync(out_conf, 0, 8 * cells, st));
    // rows that fit no tile: more than 64 A boxes or more than K18_BCAP B boxes
    int64_t cap = n_a / (kWave + 1) + n_b / (K18_BCAP + 1);
    cap = (cap < n_rows) ? cap : n_rows;
    ScratchLease lease(st);   // the list of big rows
    void *scratch = nullptr;
    int rc = lease.get(4 * (size_t)(cap + 1), &scratch);
    if (rc) return rc;
    int32_t *bigl = static_cast<int32_t *>(scratch);
    DYD_HIP(hipMemsetAsync(bigl, 0, 4, st));
    const int64_t need = ceil_div(n_rows, (int64_t)K18_WAVES * K18_WROWS);
    const int64_t want = (int64_t)ctx().num_cu * 4;   // 32 KiB of LDS per workgroup: four resident per CU
    unsigned long long *conf = reinterpret_cast<unsigned long long *>(out_conf);
    hipLaunchKernelGGL(k18_tile_kernel, dim3((unsigned)(need < want ? need : want)), dim3(K18_BLOCK), 0, st, a_box4, a_off, a_cls,
                       b_box4, b_off, b_cls, n_rows, n_classes, thr, by_label, out_a_match, out_b_match, out_b_iou, out_a_best,
                       out_b_best, out_rows, conf, bigl, (int32_t)cap);
    DYD_HIP(hipGetLastError());
    if (cap > 0) {
        hipLaunchKernelGGL(k18_big_rows_kernel, dim3((unsigned)(cap < want ? cap : want)), dim3(K18_BLOCK), 0, st, a_box4, a_off,
                           a_cls, b_box4, b_off, b_cls, n_classes, thr, by_label, out_a_match, out_b_match, out_b_iou, out_a_best,
                           out_b_best, out_rows, conf, bigl, (int32_t)cap);
        DYD_HIP(hipGetLastError());
    }
    return DYD_OK;
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_compare_boxes_dev(const double *a_box4, const int32_t *a_row_off, const int32_t *a_cls, const double *b_box4,
                          const int32_t *b_row_off, const int32_t *b_cls, int64_t n_rows, int64_t n_a, int64_t n_b,
                          int32_t n_classes, double thr, int by_label, int32_t *out_a_match, int32_t *out_b_match,
                          double *out_b_iou, double *out_a_best, double *out_b_best, int32_t *out_row_counts,
                          uint64_t *out_confusion, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_a >= 0 && n_b >= 0 && n_classes >= 0, "n_rows, n_a, n_b or n_classes < 0");
    DYD_REQUIRE(n_a < ((int64_t)1 << 31) && n_b < ((int64_t)1 << 31), "n_a or n_b exceeds int32 offsets");
    if (n_rows == 0) return DYD_OK;
    DYD_REQUIRE(a_row_off && b_row_off && out_row_counts && out_confusion, "null pointer");
    DYD_REQUIRE(n_a == 0 || (a_box4 && a_cls && out_a_match && out_a_best), "null pointer");
    DYD_REQUIRE(n_b == 0 || (b_box4 && b_cls && out_b_match && out_b_iou && out_b_best), "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(a_box4) & 15) == 0 && (reinterpret_cast<uintptr_t>(b_box4) & 15) == 0,
                "box4 must be 16-byte aligned");
    DYD_REQUIRE(ceil_div(n_rows, (int64_t)K18_WROWS) < ((int64_t)1 << 40), "n_rows out of range");
    return launch_k18(a_box4, a_row_off, a_cls, b_box4, b_row_off, b_cls, n_rows, n_a, n_b, n_classes, thr, by_label != 0,
                      out_a_match, out_b_match, out_b_iou, out_a_best, out_b_best, out_row_counts, out_confusion,
                      pick_stream(stream));
}

int dyd_compare_boxes(const double *a_box4, const int32_t *a_row_off, const int32_t *a_cls, const double *b_box4,
                      const int32_t *b_row_off, const int32_t *b_cls, int64_t n_rows, int32_t n_classes, double thr,
                      int by_label, int32_t *out_a_match, int32_t *out_b_match, double *out_b_iou, double *out_a_best,
                      double *out_b_best, int32_t *out_row_counts, uint64_t *out_confusion) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_classes >= 0, "n_rows < 0 or n_classes < 0");
    if (n_rows == 0) return DYD_OK;
    DYD_REQUIRE(out_row_counts && out_confusion, "null pointer");
    int64_t na, nb;
    int rc;
    if ((rc = k18_check_side(a_box4, a_row_off, a_cls, n_rows, n_classes, &na)) ||
        (rc = k18_check_side(b_box4, b_row_off, b_cls, n_rows, n_classes, &nb)))
        return rc;
    DYD_REQUIRE(na == 0 || (out_a_match && out_a_best), "null pointer");
    DYD_REQUIRE(nb == 0 || (out_b_match && out_b_iou && out_b_best), "null pointer");
    const size_t cells = (size_t)(n_classes + 1) * (size_t)(n_classes + 1);
    K18Side A, B;
    if ((rc = A.upload(a_box4, a_row_off, a_cls, n_rows, na)) || (rc = B.upload(b_box4, b_row_off, b_cls, n_rows, nb))) return rc;
    DevBuf d_am, d_bm, d_bi, d_ab, d_bb, d_rows, d_conf;
    if ((rc = d_am.alloc(4 * (size_t)na)) || (rc = d_bm.alloc(4 * (size_t)nb)) || (rc = d_bi.alloc(8 * (size_t)nb)) ||
        (rc = d_ab.alloc(8 * (size_t)na)) || (rc = d_bb.alloc(8 * (size_t)nb)) || (rc = d_rows.alloc(16 * (size_t)n_rows)) ||
        (rc = d_conf.alloc(8 * cells)))
        return rc;
    hipStream_t st = ctx().stream;
    KernelTimer t(st);
    rc = launch_k18(A.box.as<double>(), A.off.as<int32_t>(), A.cls.as<int32_t>(), B.box.as<double>(), B.off.as<int32_t>(),
                    B.cls.as<int32_t>(), n_rows, na, nb, n_classes, thr, by_label != 0, d_am.as<int32_t>(), d_bm.as<int32_t>(),
                    d_bi.as<double>(), d_ab.as<double>(), d_bb.as<double>(), d_rows.as<int32_t>(), d_conf.as<uint64_t>(), st);
    if (rc) return rc;
    t.finish();
    if (na) {
        DYD_HIP(hipMemcpyAsync(out_a_match, d_am.p, 4 * (size_t)na, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_a_best, d_ab.p, 8 * (size_t)na, hipMemcpyDeviceToHost, st));
    }
    if (nb) {
        DYD_HIP(hipMemcpyAsync(out_b_match, d_bm.p, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_b_iou, d_bi.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
        DYD_HIP(hipMemcpyAsync(out_b_best, d_bb.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    DYD_HIP(hipMemcpyAsync(out_row_counts, d_rows.p, 16 * (size_t)n_rows, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_confusion, d_conf.p, 8 * cells, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
