// k24_eval.hip — K24: scored box evaluation (COCO-style AP per class): matching in score order at T thresholds, then the
// per-class precision / recall accumulation.  The rule: include/dyd.h (K24) and DESIGN §5v.
//
// Entry 1, dyd_eval_match_boxes.  Table A holds the ground truth (GT), table B the detections with one score each, over the
// same rows.  Per row the finite-scored detections are ranked within their class by score (descending, ties to the earlier
// position); those of rank >= max_dets are cut.  The evaluated ones are walked in score order over the whole row (a valid
// interleaving of the classes: only boxes of equal class can match) and, at every threshold t on its own, take the GT box of
// their class that is still free at t with the largest IoU >= lim[t], ties to the HIGHEST index.
//
// Layout in HBM as K18 (k18_compare.hip) plus score = B f64.  Bytes: 36 per GT box, 44 per detection and 4 per row and table in;
// 12 per GT box and 32 per detection out.
//
// Mapping.
//   k24_rows_kernel<GW>: GW lanes (a group) own one row: lane g holds GT box g in registers with its T-bit `taken` mask (bit t:
//   taken at threshold t, which is also the out_gt_hit bit), the row's detections sit in the group's LDS slice (at most 2 GW)
//   with their results.  Ranks are counted by the lanes over the LDS scores.  At step s the row takes its s-th detection in score
//   order: every lane of equal class computes the pair's IoU once, and each threshold is one ballot of the candidates; only when
//   some group holds two or more candidates at that threshold does the wave run a max-reduction over the IoU keys (k18_pick.h)
//   and a second ballot, whose highest lane wins.  T reductions at the worst, no lane = (GT box, threshold) layout: a detection
//   has zero or one candidate at most thresholds, so the ballot alone decides.  No workgroup barrier.
//   First launch GW = 16 over all rows (16 rows per workgroup); a row of more than 16 GT boxes or 32 detections goes onto a list
//   for the GW = 64 launch (a wave per row, 64 GT boxes, 128 detections); what fits neither goes to k24_big_rows_kernel: a
//   workgroup per row, the GT boxes strided over the 256 lanes, the state in out_gt_hit / out_gt_best (read and written by the
//   owning lane only), the detections' score order in a scratch column (eval_match.h's eval_rank_row, which k25_match_kernel
//   runs too), two or three barriers per evaluated detection whatever T is.  Exact for any row length, O(n_gt * n_dt) IoUs per row (times T in the big-row kernel, which recomputes instead of
//   keeping a row of IoUs), never an n_gt x n_dt matrix.
//
// Entry 2, dyd_eval_accumulate.  The evaluated detections of the whole table are ordered by (class, score descending, index)
// with two stable rocPRIM radix sorts (the score key, then the class id).  k24_curve_kernel: one workgroup per (class, threshold)
// counts the segment's TPs, then walks it BACKWARDS in tiles of 256 with the carried TP count and the carried maximum from the
// right, so that the precision envelope is known at every position without a stored precision column; a detection that raises
// the recall writes the recall points it is the first to reach.  The best-F1 point is folded on the way.
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "eval_match.h"
#include "sized_out.h"

namespace dyd {

constexpr int K24_BLOCK = 256;
constexpr int K24_WAVES = K24_BLOCK / kWave;

template <int DCAP>
struct K24Lds {
    double x1[DCAP], y1[DCAP], x2[DCAP], y2[DCAP];
    double score[DCAP], iou[DCAP], best[DCAP];
    int32_t cls[DCAP], state[DCAP], gt[DCAP];
    uint32_t tp[DCAP];
    unsigned short perm[DCAP];   // score order -> detection, 0xFFFF: none
};

// One group of GW lanes per item; item = row, or list[1 + item] with list[0] entries.  A row that fits no tile is pushed onto next.
template <int GW>
__global__ __launch_bounds__(K24_BLOCK) void k24_rows_kernel(
    const double *__restrict__ a_box4, const int32_t *__restrict__ a_off, const int32_t *__restrict__ a_cls,
    const double *__restrict__ b_box4, const int32_t *__restrict__ b_off, const int32_t *__restrict__ b_cls,
    const double *__restrict__ b_score, int64_t n_rows, const int32_t *__restrict__ list, int32_t list_cap,
    const double *__restrict__ lim, int T, double minlim, int32_t max_dets, EvalOut out, int32_t *__restrict__ next,
    int32_t next_cap) {
    constexpr int DCAP = 2 * GW;
    constexpr int GROUPS = K24_BLOCK / GW;
    __shared__ K24Lds<DCAP> s_all[GROUPS];
    __shared__ double s_lim[EVAL_MAX_T];
    if ((int)threadIdx.x < T) s_lim[threadIdx.x] = lim[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int gl = lane & (GW - 1);
    const int gbase = lane - gl;
    const unsigned long long gmask = (GW == 64) ? ~0ull : (((1ull << (GW & 63)) - 1ull) << gbase);
    K24Lds<DCAP> &S = s_all[threadIdx.x / GW];
    int64_t n_items = n_rows;
    if (list) n_items = (list[0] < list_cap) ? list[0] : list_cap;

    for (int64_t it0 = (int64_t)blockIdx.x * GROUPS; it0 < n_items; it0 += (int64_t)gridDim.x * GROUPS) {   // block-uniform
        const int64_t item = it0 + threadIdx.x / GW;
        const bool have = item < n_items;
        int64_t a_base = 0, b_base = 0;
        int ng = 0, nd = 0;
        if (have) {
            const int64_t r = list ? (int64_t)list[1 + item] : item;
            a_base = a_off[r];
            b_base = b_off[r];
            const int32_t na = a_off[r + 1] - (int32_t)a_base, nb = b_off[r + 1] - (int32_t)b_base;
            if (na <= GW && nb <= DCAP) {
                ng = na;
                nd = nb;
            } else if (gl == 0) {
                const int32_t slot = atomicAdd(&next[0], 1);
                if (slot < next_cap) next[1 + slot] = (int32_t)r;   // always true when the caller's box counts are right
            }
        }
        const bool valid = gl < ng;
        Corners me = {0.0, 0.0, 0.0, 0.0};
        int32_t me_cls = -1;
        if (valid) {
            me = k18_load(a_box4, a_base + gl);
            me_cls = a_cls[a_base + gl];
        }
        const double me_ar = area_of(me);
        bool nan_here = valid && has_nan(me);
        for (int k = gl; k < nd; k += GW) {   // stage the detections with the results of one that takes no part
            const Corners v = k18_load(b_box4, b_base + k);
            const double sc = b_score[b_base + k] + 0.0;   // -0.0 -> 0.0
            S.x1[k] = v.x1; S.y1[k] = v.y1; S.x2[k] = v.x2; S.y2[k] = v.y2;
            S.score[k] = sc;
            S.cls[k] = b_cls[b_base + k];
            S.state[k] = eval_finite(sc) ? EVAL_EVALUATED : EVAL_BAD_SCORE;
            S.gt[k] = -1;
            S.tp[k] = 0u;
            S.iou[k] = 0.0;
            S.best[k] = 0.0;
            S.perm[k] = 0xFFFFu;
            nan_here |= has_nan(v);
        }
        const bool no_nan = __ballot(nan_here) == 0ull;
        wave_sync();
        for (int k = gl; k < nd; k += GW) {   // rank within the class, place in the row's score order
            const double sk = S.score[k];
            if (!eval_finite(sk)) continue;
            const int32_t ck = S.cls[k];
            int rank = 0, ord = 0;
            for (int j = 0; j < nd; ++j) {
                const double sj = S.score[j];
                if (eval_finite(sj) && eval_before(sj, j, sk, k)) {
                    ++ord;
                    rank += (S.cls[j] == ck) ? 1 : 0;
                }
            }
            if (rank >= max_dets) S.state[k] = EVAL_CUT;
            S.perm[ord] = (unsigned short)k;
        }
        int maxnd = nd;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(maxnd, d);
            maxnd = (o > maxnd) ? o : maxnd;
        }
        wave_sync();

        uint32_t taken = 0u;
        double gbest = 0.0;
        for (int s = 0; s < maxnd; ++s) {
            const int k = (s < nd) ? (int)S.perm[s] : 0xFFFF;   // the same in every lane of a group
            const bool act = k != 0xFFFF && S.state[k] == EVAL_EVALUATED;
            if (__ballot(act) == 0ull) continue;                // wave-uniform
            const int kk = act ? k : 0;
            const Corners o = {S.x1[kk], S.y1[kk], S.x2[kk], S.y2[kk]};
            const bool same = act && valid && S.cls[kk] == me_cls;
            double iou = 0.0;
            if (same) iou = no_nan ? k18_iou<true>(me, o, me_ar) : k18_iou<false>(me, o, me_ar);
            if (iou > gbest) gbest = iou;
            const unsigned long long bk = eval_group_max<GW>(same ? k18_best_key(iou) : 0ull);
            const bool near = same && iou >= minlim;
            uint32_t tp = 0u;
            int w0 = -1;
            double w_iou = 0.0;
            if (__ballot(near) != 0ull) {                       // wave-uniform
                for (int t = 0; t < T; ++t) {
                    const bool cand = near && !((taken >> t) & 1u) && iou >= s_lim[t];
                    unsigned long long m = __ballot(cand) & gmask;
                    if (__ballot(__popcll(m) > 1) != 0ull) {    // some group must compare IoUs
                        const unsigned long long key = cand ? k18_cand_key(iou) : 0ull;
                        const unsigned long long top = eval_group_max<GW>(key);
                        m = __ballot(cand && key == top) & gmask;
                    }
                    const int w = m ? 63 - __clzll((long long)m) : -1;   // the highest lane among the group's maxima
                    if (w == lane) taken |= 1u << t;
                    if (w >= 0) tp |= 1u << t;
                    if (t == 0) w0 = w;
                }
                w_iou = __shfl(iou, (w0 >= 0) ? w0 : lane);
            }
            if (act && gl == 0) {
                S.tp[k] = tp;
                S.gt[k] = (w0 >= 0) ? w0 - gbase : -1;
                S.iou[k] = (w0 >= 0) ? w_iou : 0.0;
                S.best[k] = k18_value(bk);
            }
        }
        wave_sync();
        if (valid) {
            out.gt_hit[a_base + gl] = taken;
            out.gt_best[a_base + gl] = gbest;
        }
        for (int k = gl; k < nd; k += GW) {
            out.dt_state[b_base + k] = S.state[k];
            out.dt_tp[b_base + k] = S.tp[k];
            out.dt_gt[b_base + k] = S.gt[k];
            out.dt_iou[b_base + k] = S.iou[k];
            out.dt_best[b_base + k] = S.best[k];
        }
        wave_sync();   // the next item overwrites S
    }
}

struct K24Sum {
    unsigned long long best;
    int32_t near;
};
struct K24Pick {
    unsigned long long key;
    int32_t idx;
};

// One workgroup per listed row.  Lane t owns the GT boxes t, t + 256, ...; `ord` holds the row's score order.
__global__ __launch_bounds__(K24_BLOCK) void k24_big_rows_kernel(
    const double *__restrict__ a_box4, const int32_t *__restrict__ a_off, const int32_t *__restrict__ a_cls,
    const double *__restrict__ b_box4, const int32_t *__restrict__ b_off, const int32_t *__restrict__ b_cls,
    const double *__restrict__ b_score, const int32_t *__restrict__ list, int32_t list_cap, const double *__restrict__ lim, int T,
    double minlim, int32_t max_dets, EvalOut out, int32_t *ord) {
    __shared__ double s_lim[EVAL_MAX_T];
    __shared__ K24Sum sum[2][K24_WAVES];          // per evaluated detection, taking turns
    __shared__ K24Pick pick[K24_WAVES][EVAL_MAX_T];
    if ((int)threadIdx.x < T) s_lim[threadIdx.x] = lim[threadIdx.x];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int32_t count = (list[0] < list_cap) ? list[0] : list_cap;
    for (int32_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int32_t r = list[1 + q];
        const int64_t a_base = a_off[r], b_base = b_off[r];
        const int32_t na = a_off[r + 1] - (int32_t)a_base;
        const int32_t nb = b_off[r + 1] - (int32_t)b_base;
        eval_rank_row<K24_BLOCK>((int)threadIdx.x, a_base, na, b_base, nb, b_score, b_cls, max_dets, [](int64_t) { return true; }, out,
                                 ord);

        int turn = 0;
        for (int32_t s = 0; s < nb; ++s) {
            const int32_t k = ord[b_base + s];
            if (k < 0) break;                                   // the finite-scored ones come first
            if (out.dt_state[b_base + k] != EVAL_EVALUATED) continue;   // block-uniform
            const Corners o = k18_load(b_box4, b_base + k);
            const int32_t o_cls = b_cls[b_base + k];
            // the detection's best IoU, the GT boxes' best IoU, and whether any pair comes near the lowest threshold
            unsigned long long bk = 0ull;
            bool near = false;
            for (int32_t i = threadIdx.x; i < na; i += K24_BLOCK) {
                if (a_cls[a_base + i] != o_cls) continue;
                const Corners me = k18_load(a_box4, a_base + i);
                const double iou = k18_iou<false>(me, o, area_of(me));
                if (iou > out.gt_best[a_base + i]) out.gt_best[a_base + i] = iou;
                const unsigned long long b1 = k18_best_key(iou);
                bk = (b1 > bk) ? b1 : bk;
                near |= iou >= minlim;
            }
            bk = eval_group_max<64>(bk);
            const bool wnear = __ballot(near) != 0ull;
            K24Sum *slot = sum[turn & 1];
            ++turn;
            if (lane == 0) {
                slot[wave].best = bk;
                slot[wave].near = wnear ? 1 : 0;
            }
            __syncthreads();
            unsigned long long gb = 0ull;
            bool any = false;
            for (int w = 0; w < K24_WAVES; ++w) {
                gb = (slot[w].best > gb) ? slot[w].best : gb;
                any |= slot[w].near != 0;
            }
            if (!any) {                                         // block-uniform
                if (threadIdx.x == 0) out.dt_best[b_base + k] = k18_value(gb);
                continue;
            }
            for (int t = 0; t < T; ++t) {
                const double lt = s_lim[t];
                unsigned long long key = 0ull;
                int32_t idx = -1;
                for (int32_t i = threadIdx.x; i < na; i += K24_BLOCK) {   // ascending: the last of equal keys stays
                    if (a_cls[a_base + i] != o_cls || ((out.gt_hit[a_base + i] >> t) & 1u)) continue;
                    const Corners me = k18_load(a_box4, a_base + i);
                    const double iou = k18_iou<false>(me, o, area_of(me));
                    if (iou >= lt) {
                        const unsigned long long c1 = k18_cand_key(iou);
                        if (c1 >= key) {
                            key = c1;
                            idx = i;
                        }
                    }
                }
                const unsigned long long wk = eval_group_max<64>(key);
                int32_t wi = (key == wk && key != 0ull) ? idx : -1;
                for (int d = 32; d >= 1; d >>= 1) {
                    const int32_t oi = __shfl_xor(wi, d);
                    wi = (oi > wi) ? oi : wi;
                }
                if (lane == 0) {
                    pick[wave][t].key = wk;
                    pick[wave][t].idx = wi;
                }
            }
            __syncthreads();
            uint32_t tp = 0u;
            int32_t g0 = -1;
            unsigned long long k0 = 0ull;
            for (int t = 0; t < T; ++t) {
                unsigned long long gk = 0ull;
                int32_t gi = -1;
                for (int w = 0; w < K24_WAVES; ++w) {
                    const K24Pick p = pick[w][t];
                    if (p.key > gk || (p.key == gk && p.key != 0ull && p.idx > gi)) {
                        gk = p.key;
                        gi = p.idx;
                    }
                }
                if (gk == 0ull) continue;
                tp |= 1u << t;
                if ((gi % K24_BLOCK) == (int32_t)threadIdx.x) out.gt_hit[a_base + gi] |= 1u << t;   // the owner of that GT box
                if (t == 0) {
                    g0 = gi;
                    k0 = gk;
                }
            }
            if (threadIdx.x == 0) {
                out.dt_tp[b_base + k] = tp;
                out.dt_gt[b_base + k] = g0;
                out.dt_iou[b_base + k] = (g0 >= 0) ? k18_value(k0 - 1ull) : 0.0;
                out.dt_best[b_base + k] = k18_value(gb);
            }
        }
        __syncthreads();   // the next row reuses sum and pick
    }
}

static int launch_k24_match(const double *a_box4, const int32_t *a_off, const int32_t *a_cls, const double *b_box4,
                            const int32_t *b_off, const int32_t *b_cls, const double *b_score, int64_t n_rows, int64_t n_a,
                            int64_t n_b, const double *lim, int T, double minlim, int32_t max_dets, EvalOut out, hipStream_t st) {
    // rows that leave the 16-lane launch, and those that also leave the 64-lane one
    int64_t cap_mid = n_a / 17 + n_b / 33, cap_big = n_a / 65 + n_b / 129;
    cap_mid = (cap_mid < n_rows) ? cap_mid : n_rows;
    cap_big = (cap_big < n_rows) ? cap_big : n_rows;
    const size_t words = (size_t)(cap_mid + 1) + (size_t)(cap_big + 1) + (size_t)(cap_big > 0 ? n_b : 0);
    ScratchLease lease(st);   // the two row lists and the big rows' score order
    void *scratch = nullptr;
    int rc = lease.get(4 * words, &scratch);
    if (rc) return rc;
    int32_t *mid = static_cast<int32_t *>(scratch);
    int32_t *big = mid + cap_mid + 1;
    int32_t *ord = big + cap_big + 1;
    DYD_HIP(hipMemsetAsync(mid, 0, 4, st));
    DYD_HIP(hipMemsetAsync(big, 0, 4, st));
    const int64_t want = (int64_t)ctx().num_cu * 4;   // 37 KiB of LDS per workgroup: four resident per CU
    int64_t need = ceil_div(n_rows, (int64_t)(K24_BLOCK / 16));
    hipLaunchKernelGGL(k24_rows_kernel<16>, dim3((unsigned)(need < want ? need : want)), dim3(K24_BLOCK), 0, st, a_box4, a_off, a_cls,
                       b_box4, b_off, b_cls, b_score, n_rows, (const int32_t *)nullptr, 0, lim, T, minlim, max_dets, out, mid,
                       (int32_t)cap_mid);
    DYD_HIP(hipGetLastError());
    if (cap_mid > 0) {
        need = ceil_div(cap_mid, (int64_t)K24_WAVES);
        hipLaunchKernelGGL(k24_rows_kernel<64>, dim3((unsigned)(need < want ? need : want)), dim3(K24_BLOCK), 0, st, a_box4, a_off,
                           a_cls, b_box4, b_off, b_cls, b_score, n_rows, (const int32_t *)mid, (int32_t)cap_mid, lim, T, minlim,
                           max_dets, out, big, (int32_t)cap_big);
        DYD_HIP(hipGetLastError());
    }
    if (cap_big > 0) {
        hipLaunchKernelGGL(k24_big_rows_kernel, dim3((unsigned)(cap_big < want ? cap_big : want)), dim3(K24_BLOCK), 0, st, a_box4,
                           a_off, a_cls, b_box4, b_off, b_cls, b_score, (const int32_t *)big, (int32_t)cap_big, lim, T, minlim,
                           max_dets, out, ord);
        DYD_HIP(hipGetLastError());
    }
    return DYD_OK;
}

// ------------------------------------------------------------------------------------------------ accumulation
constexpr double K24_EPS = 0x1p-52;

// descending order of the (finite) scores as ascending u64 keys; -0.0 counts as 0.0
__global__ __launch_bounds__(K24_BLOCK) void k24_score_keys_kernel(const double *__restrict__ score, int32_t n,
                                                                   unsigned long long *__restrict__ key) {
    const int32_t i = blockIdx.x * K24_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = k18_bits(score[i] + 0.0);
    const unsigned long long asc = (b >> 63) ? ~b : (b | (1ull << 63));
    key[i] = ~asc;
}

__global__ __launch_bounds__(K24_BLOCK) void k24_gather_kernel(const int32_t *__restrict__ cls, const uint32_t *__restrict__ perm,
                                                               int32_t n, uint32_t *__restrict__ out) {
    const int32_t i = blockIdx.x * K24_BLOCK + threadIdx.x;
    if (i < n) out[i] = (uint32_t)cls[perm[i]];
}

// first r with rec[r] > v (rec ascending)
__device__ __forceinline__ int k24_upper(const double *__restrict__ rec, int R, double v) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One workgroup per (class, threshold); perm = the detections by (class, score descending, index), seg = class offsets in it.
__global__ __launch_bounds__(K24_BLOCK) void k24_curve_kernel(
    const double *__restrict__ score, const uint32_t *__restrict__ tp, const uint32_t *__restrict__ perm,
    const int32_t *__restrict__ seg, const int64_t *__restrict__ npig, int T, const double *__restrict__ rec, int R,
    double *out_precision, double *out_score_at, double *__restrict__ out_recall, double *__restrict__ out_ap,
    double *__restrict__ out_best_f1, double *__restrict__ out_best_score, int64_t *__restrict__ out_best_tp,
    int64_t *__restrict__ out_best_dets) {
    __shared__ int s_total;
    __shared__ int s_wtot[K24_WAVES];
    __shared__ double s_wmax[K24_WAVES];
    __shared__ double s_f1[K24_BLOCK];
    __shared__ int32_t s_k[K24_BLOCK], s_tp[K24_BLOCK];
    const int ct = blockIdx.x;
    const int c = ct / T, t = ct % T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t s0 = seg[c], s1 = seg[c + 1], m = s1 - s0;
    const int64_t np = npig[c];
    double *P = out_precision + (int64_t)ct * R, *SA = out_score_at + (int64_t)ct * R;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (np <= 0 || m == 0) {   // no ground truth: undefined; no detection: an empty curve
        const double v = (np <= 0) ? nan : 0.0;
        for (int r = threadIdx.x; r < R; r += K24_BLOCK) {
            P[r] = v;
            SA[r] = v;
        }
        if (threadIdx.x == 0) {
            out_recall[ct] = v;
            out_ap[ct] = v;
            out_best_f1[ct] = nan;
            out_best_score[ct] = nan;
            out_best_tp[ct] = 0;
            out_best_dets[ct] = 0;
        }
        return;
    }
    for (int r = threadIdx.x; r < R; r += K24_BLOCK) {
        P[r] = 0.0;
        SA[r] = 0.0;
    }
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    int cnt = 0;
    for (int32_t k = s0 + threadIdx.x; k < s1; k += K24_BLOCK) cnt += (tp[perm[k]] >> t) & 1u;
    if (cnt) atomicAdd(&s_total, cnt);
    __syncthreads();   // also: the zeros above are written before any recall point
    const int total = s_total;
    const double dnp = (double)np;

    int carry = total;         // TPs up to the end of the current tile
    double right = 0.0;        // the largest precision to the right of the current tile
    double bf1 = -1.0;
    int32_t bk = 0, btp = 0;
    for (int32_t tile = (m - 1) / K24_BLOCK; tile >= 0; --tile) {
        const int32_t kk = tile * K24_BLOCK + threadIdx.x;   // position in the segment
        const bool in = kk < m;
        const uint32_t p = in ? perm[s0 + kk] : 0u;
        const int bit = in ? (int)((tp[p] >> t) & 1u) : 0;
        const unsigned long long bal = __ballot(bit != 0);
        const int incl = __popcll(bal & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull)));
        if (lane == 0) s_wtot[wave] = __popcll(bal);
        __syncthreads();
        int tile_sum = 0, before = 0;
        for (int w = 0; w < K24_WAVES; ++w) {
            tile_sum += s_wtot[w];
            before += (w < wave) ? s_wtot[w] : 0;
        }
        const int tpk = carry - tile_sum + before + incl;    // TPs among the positions 0..kk
        const double pr = in ? (double)tpk / ((double)(kk + 1) + K24_EPS) : 0.0;
        double env = pr;                                     // the running maximum from the right
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_down(env, d);
            if (lane + d < 64 && o > env) env = o;
        }
        if (lane == 0) s_wmax[wave] = env;
        __syncthreads();
        double tile_max = right;
        for (int w = 0; w < K24_WAVES; ++w) {
            const double v = s_wmax[w];
            if (w > wave && v > env) env = v;
            if (v > tile_max) tile_max = v;
        }
        if (right > env) env = right;
        if (in) {
            const double sc = score[p] + 0.0;
            if (bit || kk == 0) {   // the first position to reach the recall points in (rc of kk - 1, rc of kk]
                const int lo = (kk == 0) ? 0 : k24_upper(rec, R, (double)(tpk - bit) / dnp);
                const int hi = k24_upper(rec, R, (double)tpk / dnp);
                for (int r = lo; r < hi; ++r) {
                    P[r] = env;
                    SA[r] = sc;
                }
            }
            const bool run_end = kk == m - 1 || (score[perm[s0 + kk + 1]] + 0.0) != sc;
            if (run_end) {
                const double f1 = (double)(2 * (int64_t)tpk) / (double)((int64_t)(kk + 1) + np);
                if (f1 >= bf1) {   // kk descends: the smallest position of equal values stays
                    bf1 = f1;
                    bk = kk;
                    btp = tpk;
                }
            }
        }
        right = tile_max;
        carry -= tile_sum;
        __syncthreads();   // s_wtot and s_wmax are rewritten
    }
    s_f1[threadIdx.x] = bf1;
    s_k[threadIdx.x] = bk;
    s_tp[threadIdx.x] = btp;
    __syncthreads();       // and the recall points are written
    if (threadIdx.x == 0) {
        for (int i = 1; i < K24_BLOCK; ++i)
            if (s_f1[i] > bf1 || (s_f1[i] == bf1 && s_f1[i] >= 0.0 && s_k[i] < bk)) {
                bf1 = s_f1[i];
                bk = s_k[i];
                btp = s_tp[i];
            }
        out_recall[ct] = (double)total / dnp;
        double sum = 0.0;
        for (int r = 0; r < R; ++r) sum += P[r];
        out_ap[ct] = sum / (double)R;
        out_best_f1[ct] = bf1;
        out_best_score[ct] = score[perm[s0 + bk]] + 0.0;
        out_best_tp[ct] = btp;
        out_best_dets[ct] = (int64_t)bk + 1;
    }
}

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_eval_match_boxes(const double *gt_box4, const int32_t *gt_row_off, const int32_t *gt_cls, const double *dt_box4,
                         const int32_t *dt_row_off, const int32_t *dt_cls, const double *dt_score, int64_t n_rows,
                         int32_t n_classes, const double *iou_thr, int32_t T, int32_t max_dets, int32_t *out_dt_state,
                         uint32_t *out_dt_tp, int32_t *out_dt_gt, double *out_dt_iou, double *out_dt_best, uint32_t *out_gt_hit,
                         double *out_gt_best) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_rows >= 0 && n_classes >= 0, "n_rows < 0 or n_classes < 0");
    EvalLimits L;
    int rc = L.set(iou_thr, T, max_dets);
    if (rc) return rc;
    if (n_rows == 0) return DYD_OK;
    int64_t na, nb;
    if ((rc = k18_check_side(gt_box4, gt_row_off, gt_cls, n_rows, n_classes, &na)) ||
        (rc = k18_check_side(dt_box4, dt_row_off, dt_cls, n_rows, n_classes, &nb)))
        return rc;
    DYD_REQUIRE(na == 0 || (out_gt_hit && out_gt_best), "null pointer");
    DYD_REQUIRE(nb == 0 || (dt_score && out_dt_state && out_dt_tp && out_dt_gt && out_dt_iou && out_dt_best), "null pointer");
    K18Side A, B;
    if ((rc = A.upload(gt_box4, gt_row_off, gt_cls, n_rows, na)) || (rc = B.upload(dt_box4, dt_row_off, dt_cls, n_rows, nb))) return rc;
    DevBuf d_sc, d_lim;
    EvalOutDev res;
    if ((rc = d_sc.alloc(8 * (size_t)nb)) || (rc = d_lim.alloc(8 * (size_t)T)) || (rc = res.alloc(na, nb))) return rc;
    hipStream_t st = ctx().stream;
    if (nb) DYD_HIP(hipMemcpyAsync(d_sc.p, dt_score, 8 * (size_t)nb, hipMemcpyHostToDevice, st));
    DYD_HIP(hipMemcpyAsync(d_lim.p, L.lim, 8 * (size_t)T, hipMemcpyHostToDevice, st));
    DYD_HIP(hipStreamSynchronize(st));   // L lives on this frame
    KernelTimer timer(st);
    rc = launch_k24_match(A.box.as<double>(), A.off.as<int32_t>(), A.cls.as<int32_t>(), B.box.as<double>(), B.off.as<int32_t>(),
                          B.cls.as<int32_t>(), d_sc.as<double>(), n_rows, na, nb, d_lim.as<double>(), T, L.minlim, max_dets, res.out(),
                          st);
    if (rc) return rc;
    timer.finish();
    if ((rc = res.copy_back({out_dt_state, out_dt_tp, out_dt_gt, out_dt_iou, out_dt_best, out_gt_hit, out_gt_best}, st))) return rc;
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

int dyd_eval_accumulate(const int32_t *cls, const double *score, const uint32_t *tp, int64_t n, int32_t n_classes, int32_t T,
                        const int64_t *npig, const double *rec, int32_t R, double *out_precision, double *out_score_at,
                        double *out_recall, double *out_ap, double *out_best_f1, double *out_best_score, int64_t *out_best_tp,
                        int64_t *out_best_dets) {
    DYD_API_ENTER();
    DYD_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n outside 0..2^31-1");
    DYD_REQUIRE(n_classes >= 0 && R >= 1, "n_classes < 0 or R < 1");
    DYD_REQUIRE(T >= 1 && T <= EVAL_MAX_T, "T outside 1..32");
    DYD_REQUIRE((int64_t)n_classes * T < ((int64_t)1 << 31), "n_classes * T out of range");
    if (n_classes == 0) return DYD_OK;
    DYD_REQUIRE(npig && out_recall && out_ap && out_best_f1 && out_best_score && out_best_tp && out_best_dets, "null pointer");
    DYD_REQUIRE(rec && out_precision && out_score_at, "null pointer");
    DYD_REQUIRE(n == 0 || (cls && score && tp), "null pointer");
    for (int32_t r = 0; r < R; ++r) DYD_REQUIRE(rec[r] == rec[r] && (r == 0 || rec[r] >= rec[r - 1]), "rec not ascending");
    for (int32_t c = 0; c < n_classes; ++c) DYD_REQUIRE(npig[c] >= 0, "npig < 0");
    std::vector<int32_t> seg((size_t)n_classes + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        DYD_REQUIRE(cls[i] >= 0 && cls[i] < n_classes, "class id outside 0..n_classes-1");
        DYD_REQUIRE(score[i] - score[i] == 0.0, "score not finite");
        ++seg[(size_t)cls[i] + 1];
    }
    for (int32_t c = 0; c < n_classes; ++c) seg[c + 1] += seg[c];
    int cbits = 1;
    while (cbits < 31 && ((int64_t)1 << cbits) < n_classes) ++cbits;

    const size_t CT = (size_t)n_classes * (size_t)T, N = (size_t)n;
    hipStream_t st = ctx().stream;
    size_t tmp_a = 0, tmp_b = 0;
    DYD_HIP(rocprim::radix_sort_pairs(nullptr, tmp_a, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                      rocprim::make_counting_iterator<uint32_t>(0u), (uint32_t *)nullptr, N, 0u, 64u, st));
    DYD_HIP(rocprim::radix_sort_pairs(nullptr, tmp_b, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, N, 0u, (unsigned)cbits, st));
    const size_t tmp_bytes = (tmp_a > tmp_b) ? tmp_a : tmp_b;
    DevBuf d_cls, d_score, d_tp, d_seg, d_npig, d_rec, d_key, d_key2, d_p1, d_ck, d_ck2, d_perm, d_tmp;
    DevBuf d_prec, d_sat, d_rc, d_ap, d_f1, d_bs, d_btp, d_bd;
    int rc;
    if ((rc = d_cls.alloc(4 * N)) || (rc = d_score.alloc(8 * N)) || (rc = d_tp.alloc(4 * N)) ||
        (rc = d_seg.alloc(4 * seg.size())) || (rc = d_npig.alloc(8 * (size_t)n_classes)) || (rc = d_rec.alloc(8 * (size_t)R)) ||
        (rc = d_key.alloc(8 * N)) || (rc = d_key2.alloc(8 * N)) || (rc = d_p1.alloc(4 * N)) || (rc = d_ck.alloc(4 * N)) ||
        (rc = d_ck2.alloc(4 * N)) || (rc = d_perm.alloc(4 * N)) || (rc = d_tmp.alloc(tmp_bytes)) ||
        (rc = d_prec.alloc(8 * CT * (size_t)R)) || (rc = d_sat.alloc(8 * CT * (size_t)R)) || (rc = d_rc.alloc(8 * CT)) ||
        (rc = d_ap.alloc(8 * CT)) || (rc = d_f1.alloc(8 * CT)) || (rc = d_bs.alloc(8 * CT)) || (rc = d_btp.alloc(8 * CT)) ||
        (rc = d_bd.alloc(8 * CT)))
        return rc;
    if (n) {
        DYD_HIP(hipMemcpyAsync(d_cls.p, cls, 4 * N, hipMemcpyHostToDevice, st));
        DYD_HIP(hipMemcpyAsync(d_score.p, score, 8 * N, hipMemcpyHostToDevice, st));
        DYD_HIP(hipMemcpyAsync(d_tp.p, tp, 4 * N, hipMemcpyHostToDevice, st));
    }
    DYD_HIP(hipMemcpyAsync(d_seg.p, seg.data(), 4 * seg.size(), hipMemcpyHostToDevice, st));
    DYD_HIP(hipMemcpyAsync(d_npig.p, npig, 8 * (size_t)n_classes, hipMemcpyHostToDevice, st));
    DYD_HIP(hipMemcpyAsync(d_rec.p, rec, 8 * (size_t)R, hipMemcpyHostToDevice, st));
    DYD_HIP(hipStreamSynchronize(st));   // seg lives on this frame
    KernelTimer timer(st);
    if (n) {
        const unsigned blocks = (unsigned)ceil_div(n, K24_BLOCK);
        hipLaunchKernelGGL(k24_score_keys_kernel, dim3(blocks), dim3(K24_BLOCK), 0, st, d_score.as<double>(), (int32_t)n,
                           d_key.as<unsigned long long>());
        DYD_HIP(hipGetLastError());
        size_t tb = tmp_bytes;
        DYD_HIP(rocprim::radix_sort_pairs(d_tmp.p, tb, d_key.as<unsigned long long>(), d_key2.as<unsigned long long>(),
                                          rocprim::make_counting_iterator<uint32_t>(0u), d_p1.as<uint32_t>(), N, 0u, 64u, st));
        hipLaunchKernelGGL(k24_gather_kernel, dim3(blocks), dim3(K24_BLOCK), 0, st, d_cls.as<int32_t>(), d_p1.as<uint32_t>(),
                           (int32_t)n, d_ck.as<uint32_t>());
        DYD_HIP(hipGetLastError());
        tb = tmp_bytes;
        DYD_HIP(rocprim::radix_sort_pairs(d_tmp.p, tb, d_ck.as<uint32_t>(), d_ck2.as<uint32_t>(), d_p1.as<uint32_t>(),
                                          d_perm.as<uint32_t>(), N, 0u, (unsigned)cbits, st));
    }
    hipLaunchKernelGGL(k24_curve_kernel, dim3((unsigned)CT), dim3(K24_BLOCK), 0, st, d_score.as<double>(), d_tp.as<uint32_t>(),
                       d_perm.as<uint32_t>(), d_seg.as<int32_t>(), d_npig.as<int64_t>(), (int)T, d_rec.as<double>(), (int)R,
                       d_prec.as<double>(), d_sat.as<double>(), d_rc.as<double>(), d_ap.as<double>(), d_f1.as<double>(),
                       d_bs.as<double>(), d_btp.as<int64_t>(), d_bd.as<int64_t>());
    DYD_HIP(hipGetLastError());
    timer.finish();
    DYD_HIP(hipMemcpyAsync(out_precision, d_prec.p, 8 * CT * (size_t)R, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_score_at, d_sat.p, 8 * CT * (size_t)R, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_recall, d_rc.p, 8 * CT, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_ap, d_ap.p, 8 * CT, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_best_f1, d_f1.p, 8 * CT, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_best_score, d_bs.p, 8 * CT, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_best_tp, d_btp.p, 8 * CT, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_best_dets, d_bd.p, 8 * CT, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
