// eval_match.h — what the two scored matchers share: K24 (k24_eval.hip, boxes by K18's IoU) and K25 (k25_poly_eval.hip,
// polygons by K22's mask IoU).  The rule: include/dyd.h (K24, K25) and DESIGN §5v, §5w.
//   Device: the seven result columns (EvalOut) and the detection states, the score predicates, the maximum over a group of
//   lanes, and the rank pass of a row whose state lives in memory (eval_rank_row: k24_big_rows_kernel with 256 lanes,
//   k25_match_kernel with 64; k24_rows_kernel ranks over its LDS slice with the same predicates).
//   Host: the clamped limits (EvalLimits) and the result columns in device memory (EvalOutDev).
// One threshold's arg-max (a lane's ascending walk that keeps the last of equal k18_pick.h keys, then the wave's largest key and
// the HIGHEST index among its holders) stays written out in k24_big_rows_kernel and k25_match_kernel: as functions over the
// caller's IoU functor, in five spellings, the walk moved both kernels' registers (K24 68 -> 81..87 VGPRs and 7 -> 5 waves per
// SIMD, K25 79 -> 81 and 6 -> 5), and the wave step alone, in five, moved K24's (80 VGPRs, 6 waves): DESIGN §7.  The rank pass
// holds the parent's remarks only with takes_part over the detection's place in the table, captured by value.
#pragma once

#include <cmath>

#include "k18_pick.h"

namespace dyd {

constexpr int EVAL_MAX_T = 32;   // thresholds per call: one bit each in dt_tp and gt_hit
// dt_state.  CUT: rank within (row, class) >= max_dets; BAD_SCORE: not finite; SKIPPED: takes no part (K25: action is not 0)
enum : int32_t { EVAL_EVALUATED = 0, EVAL_CUT = 1, EVAL_BAD_SCORE = 2, EVAL_SKIPPED = 3 };

struct EvalOut {
    int32_t *dt_state;
    uint32_t *dt_tp;
    int32_t *dt_gt;
    double *dt_iou, *dt_best;
    uint32_t *gt_hit;
    double *gt_best;
};

__device__ __forceinline__ bool eval_finite(double s) { return (s - s) == 0.0; }
// detection j goes before detection k (both finite scores)
template <class N>
__device__ __forceinline__ bool eval_before(double sj, N j, double sk, N k) { return sj > sk || (sj == sk && j < k); }

template <int GW>
__device__ __forceinline__ unsigned long long eval_group_max(unsigned long long v) {
#pragma unroll
    for (int d = GW / 2; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = (o > v) ? o : v;
    }
    return v;
}

// State and rank of every detection of one row and the row's score order, by STRIDE lanes (tid = 0..STRIDE-1, the whole
// workgroup).  Clears gt_hit / gt_best of the row's na GT objects and writes the five detection outputs at their defaults;
// ord[b_base + s] = the s-th detection in score order, -1 behind the last finite-scored one.  takes_part(b_base + k): a detection for
// which it is false is EVAL_SKIPPED and is left out of every other detection's rank and order.  Both barriers are inside.
// N: the kernel's index type (int32_t in K24, int64_t in K25).
template <int STRIDE, class N, class F>
__device__ __forceinline__ void eval_rank_row(int tid, int64_t a_base, N na, int64_t b_base, N nb, const double *__restrict__ b_score,
                                              const int32_t *__restrict__ b_cls, int32_t max_dets, F takes_part, const EvalOut &out,
                                              int32_t *ord) {
    for (N i = tid; i < na; i += STRIDE) {
        out.gt_hit[a_base + i] = 0u;
        out.gt_best[a_base + i] = 0.0;
    }
    for (N k = tid; k < nb; k += STRIDE) ord[b_base + k] = -1;
    __syncthreads();
    for (N k = tid; k < nb; k += STRIDE) {
        int32_t state = EVAL_SKIPPED;
        if (takes_part(b_base + k)) {
            const double sk = b_score[b_base + k] + 0.0;   // -0.0 -> 0.0
            state = EVAL_BAD_SCORE;
            if (eval_finite(sk)) {
                const int32_t ck = b_cls[b_base + k];
                N rank = 0, o = 0;
                for (N j = 0; j < nb; ++j) {
                    if (!takes_part(b_base + j)) continue;
                    const double sj = b_score[b_base + j] + 0.0;
                    if (eval_finite(sj) && eval_before(sj, j, sk, k)) {
                        ++o;
                        rank += (b_cls[b_base + j] == ck) ? 1 : 0;
                    }
                }
                state = (rank >= max_dets) ? EVAL_CUT : EVAL_EVALUATED;
                ord[b_base + o] = (int32_t)k;
            }
        }
        out.dt_state[b_base + k] = state;
        out.dt_tp[b_base + k] = 0u;
        out.dt_gt[b_base + k] = -1;
        out.dt_iou[b_base + k] = 0.0;
        out.dt_best[b_base + k] = 0.0;
    }
    __syncthreads();
}

// The thresholds of one call as the kernels take them: lim[t] = min(iou_thr[t], 1 - 1e-10), and the lowest of them.
struct EvalLimits {
    double lim[EVAL_MAX_T], minlim;
    int set(const double *iou_thr, int32_t T, int32_t max_dets) {
        DYD_REQUIRE(T >= 1 && T <= EVAL_MAX_T, "T outside 1..32");
        DYD_REQUIRE(max_dets >= 1, "max_dets < 1");
        DYD_REQUIRE(iou_thr, "null pointer");
        const double cap = 1.0 - 1e-10;
        minlim = HUGE_VAL;
        for (int t = 0; t < T; ++t) {
            lim[t] = (cap < iou_thr[t]) ? cap : iou_thr[t];   // NaN stays and matches nothing
            if (lim[t] < minlim) minlim = lim[t];
        }
        return DYD_OK;
    }
};

// The seven result columns in device memory: five per detection (nb), two per GT object (na).
struct EvalOutDev {
    DevBuf st, tp, gt, iou, best, hit, gbest;
    size_t na = 0, nb = 0;
    int alloc(int64_t n_a, int64_t n_b) {
        na = (size_t)n_a;
        nb = (size_t)n_b;
        int rc;
        if ((rc = st.alloc(4 * nb)) || (rc = tp.alloc(4 * nb)) || (rc = gt.alloc(4 * nb)) || (rc = iou.alloc(8 * nb)) ||
            (rc = best.alloc(8 * nb)) || (rc = hit.alloc(4 * na)) || (rc = gbest.alloc(8 * na)))
            return rc;
        return DYD_OK;
    }
    EvalOut out() {
        return {st.as<int32_t>(), tp.as<uint32_t>(), gt.as<int32_t>(), iou.as<double>(), best.as<double>(), hit.as<uint32_t>(),
                gbest.as<double>()};
    }
    // queues the copies to the caller's arrays (an empty column's pointer may be NULL); the caller waits for s
    int copy_back(const EvalOut &host, hipStream_t s) {
        const CopyBack back[] = {{host.dt_state, st.p, 4 * nb}, {host.dt_tp, tp.p, 4 * nb},   {host.dt_gt, gt.p, 4 * nb},
                                 {host.dt_iou, iou.p, 8 * nb},  {host.dt_best, best.p, 8 * nb}, {host.gt_hit, hit.p, 4 * na},
                                 {host.gt_best, gbest.p, 8 * na}};
        for (const CopyBack &c : back)
            if (c.bytes) DYD_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s));
        return DYD_OK;
    }
};

}  // namespace dyd
