// k25_poly_eval.hip — K25: scored polygon evaluation (COCO-style mask AP per class): K24's selection and matching rule on
// K22's mask IoU.  The rule: include/dyd.h (K25) and DESIGN §5w.  The accumulation is K24's dyd_eval_accumulate, unchanged.
//
// Table A holds the ground truth (GT), table B the detections with one score each, both in K22's layout over the same rows.
// The pair step is K22's (k22_pairs.h: rows, polygons, paint into the pair table, pixel counts) in the paint kernel's evaluation
// flavour, which keeps no owners, runs no class-pair pass and leaves the cells of pairs of different classes alone: only
// polygons of equal class can match, so those cells are never read here.
//
// Mapping of k25_match_kernel: a wave (one workgroup) per row, rows taken grid-stride.  Both existing matchers were read for it.
// k24_big_rows_kernel gives a row to 256 lanes because a candidate there costs a box load and K2's IoU arithmetic, recomputed
// per threshold, and pays two or three workgroup barriers per evaluated detection for it.  Here a candidate costs one u32 load
// from the pair cell and one division, the same as in k22_match_kernel, and the rows are those of K22: a few polygons each in
// most tables, at most max_pairs_per_row pairs.  So K22's scheme is kept: lanes stride over the GT polygons, the detections are
// taken in score order, and every reduction is a wave's own (shuffles and ballots), never a workgroup barrier between waves.
// What K22 lacks is eval_match.h's, shared with k24_big_rows_kernel: the result columns and states, and eval_rank_row, the state
// and rank of every detection counted by the lanes over the row's scores with the row's score order in a scratch column (ord,
// one i32 per detection).  The arg-max is the big-row kernel's too, written out in both.  The GT state is the T-bit
// mask in out_gt_hit, read and written by the owning lane (index % 64) only, as out_gt_best is.  A row of at most 64 GT
// polygons keeps the detection's IoU in a register across the thresholds; a longer one recomputes it from the cell.  The
// arg-max is over k18_pick.h's keys: the largest key, then the highest index (the last of equal keys stays in a lane's
// ascending walk, then the maximum over the holders).  A detection without a same-class pair at or above the lowest limit
// skips the T loop.  Exact for any row length; no atomics, no result depends on the schedule.
#include "eval_match.h"
#include "k21_cover.h"
#include "k22_pairs.h"
#include "poly_table.h"

namespace dyd {

// inter > 0: one correctly rounded division of two exact integers
__device__ __forceinline__ double k25_iou(uint32_t inter, unsigned long long pg, unsigned long long pd) {
    return (double)inter / (double)(pg + pd - inter);
}

__global__ __launch_bounds__(kWave) void k25_match_kernel(
    const int32_t *__restrict__ a_row_off, const int32_t *__restrict__ a_cls, const uint8_t *__restrict__ a_action,
    const unsigned long long *__restrict__ a_pixels, const int32_t *__restrict__ b_row_off, const int32_t *__restrict__ b_cls,
    const uint8_t *__restrict__ b_action, const unsigned long long *__restrict__ b_pixels, const double *__restrict__ b_score,
    int64_t n_rows, int64_t n_a, int64_t n_b, const double *__restrict__ lim, int T, double minlim, int32_t max_dets,
    const uint8_t *__restrict__ row_status, const int64_t *__restrict__ pair_off, const uint32_t *__restrict__ pairs, EvalOut out,
    int32_t *ord) {
    __shared__ double s_lim[EVAL_MAX_T];
    const int lane = threadIdx.x;
    if (lane < T) s_lim[lane] = lim[lane];
    __syncthreads();
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        int64_t a0, a1, b0, b1;
        k21_row_polys(a_row_off, r, n_a, &a0, &a1);
        k21_row_polys(b_row_off, r, n_b, &b0, &b1);
        const int64_t na = a1 - a0, nb = b1 - b0, cell0 = pair_off[r];
        const bool one = na <= kWave;   // every GT polygon of the row has a lane of its own
        // a row that is not evaluated has no polygon of action 0
        eval_rank_row<kWave>(lane, a0, na, b0, nb, b_score, b_cls, max_dets, [=](int64_t p) { return b_action[p] == COVER_DONE; },
                             out, ord);

        for (int64_t s = 0; s < nb; ++s) {   // wave-uniform
            const int32_t k = ord[b0 + s];
            if (k < 0) break;                                   // the ranked ones come first
            if (out.dt_state[b0 + k] != EVAL_EVALUATED) continue;
            const int32_t cd = b_cls[b0 + k];
            const unsigned long long pd = b_pixels[b0 + k];
            // the detection's best IoU, the GT polygons' best IoU, and whether any pair comes near the lowest limit
            unsigned long long bk = 0ull;
            bool near = false;
            double iou1 = 0.0;                                  // with `one`: the IoU with the lane's GT polygon, 0.0 = no pair
            for (int64_t i = lane; i < na; i += kWave) {
                if (a_action[a0 + i] != COVER_DONE || a_cls[a0 + i] != cd) continue;
                const uint32_t inter = pairs[cell0 + i * nb + k];
                if (inter == 0) continue;
                const double iou = k25_iou(inter, a_pixels[a0 + i], pd);
                if (iou > out.gt_best[a0 + i]) out.gt_best[a0 + i] = iou;
                const unsigned long long b1k = k18_bits(iou);   // iou > 0: ordered like its bits
                bk = (b1k > bk) ? b1k : bk;
                near |= iou >= minlim;
                iou1 = iou;
            }
            bk = eval_group_max<64>(bk);
            uint32_t tp = 0u;
            int64_t g0 = -1;
            unsigned long long k0 = 0ull;
            if (__ballot(near) != 0ull) {                       // wave-uniform
                for (int t = 0; t < T; ++t) {
                    const double lt = s_lim[t];
                    unsigned long long key = 0ull;
                    int64_t idx = -1;
                    if (one) {
                        if (iou1 >= lt && iou1 > 0.0 && !((out.gt_hit[a0 + lane] >> t) & 1u)) {
                            key = k18_cand_key(iou1);
                            idx = lane;
                        }
                    } else {
                        for (int64_t i = lane; i < na; i += kWave) {   // ascending: the last of equal keys stays
                            if (a_action[a0 + i] != COVER_DONE || a_cls[a0 + i] != cd || ((out.gt_hit[a0 + i] >> t) & 1u)) continue;
                            const uint32_t inter = pairs[cell0 + i * nb + k];
                            if (inter == 0) continue;
                            const double iou = k25_iou(inter, a_pixels[a0 + i], pd);
                            if (iou >= lt) {
                                const unsigned long long c1 = k18_cand_key(iou);
                                if (c1 >= key) {
                                    key = c1;
                                    idx = i;
                                }
                            }
                        }
                    }
                    const unsigned long long wk = eval_group_max<64>(key);
                    if (wk == 0ull) continue;                   // wave-uniform
                    int64_t wi = (key == wk) ? idx : -1;
                    for (int d = 32; d >= 1; d >>= 1) {
                        const int64_t oi = __shfl_xor(wi, d);
                        wi = (oi > wi) ? oi : wi;
                    }
                    tp |= 1u << t;
                    if (wi % kWave == lane) out.gt_hit[a0 + wi] |= 1u << t;   // the owner of that GT polygon
                    if (t == 0) {
                        g0 = wi;
                        k0 = wk;
                    }
                }
            }
            if (lane == 0) {
                out.dt_tp[b0 + k] = tp;
                out.dt_gt[b0 + k] = (int32_t)g0;
                out.dt_iou[b0 + k] = (g0 >= 0) ? k18_value(k0 - 1ull) : 0.0;
                out.dt_best[b0 + k] = k18_value(bk);
            }
        }
        __syncthreads();   // ord and the states of the next row are written behind every read of this one
    }
}

constexpr SizedName K25_PAIRS{"K25", "pair", "elements", 4};

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_eval_match_polygons(const double *gt_xy, const int32_t *gt_pt_off, const int32_t *gt_row_off, const int32_t *gt_cls,
                            const double *dt_xy, const int32_t *dt_pt_off, const int32_t *dt_row_off, const int32_t *dt_cls,
                            const double *dt_score, const double *width, const double *height, int64_t n_rows, int32_t n_classes,
                            const double *iou_thr, int32_t T, int32_t max_dets, int64_t max_pixels_per_row,
                            int64_t max_pairs_per_row, uint8_t *out_row_status, int64_t *out_pair_off, uint8_t *out_gt_action,
                            uint8_t *out_dt_action, int64_t *out_gt_pixels, int64_t *out_dt_pixels, int32_t *out_dt_state,
                            uint32_t *out_dt_tp, int32_t *out_dt_gt, double *out_dt_iou, double *out_dt_best, uint32_t *out_gt_hit,
                            double *out_gt_best) {
    DYD_API_ENTER();
    EvalLimits L;
    int rc = compare_params(n_classes, max_pixels_per_row, max_pairs_per_row);
    if (rc || (rc = L.set(iou_thr, T, max_dets))) return rc;
    DYD_REQUIRE(n_rows >= 0, "negative size");
    DYD_REQUIRE(n_rows < (1LL << 31), "size too large");
    if (n_rows == 0) return DYD_OK;
    DYD_REQUIRE(out_pair_off, "null pointer");
    int64_t na = 0, npa = 0, nb = 0, npb = 0;
    if ((rc = poly_table_check(gt_xy, gt_pt_off, gt_row_off, n_rows, width, height, out_row_status != nullptr,
                               gt_cls && out_gt_action && out_gt_pixels && out_gt_hit && out_gt_best, nullptr, 0, &na, &npa)) ||
        (rc = poly_table_check(dt_xy, dt_pt_off, dt_row_off, n_rows, width, height, out_row_status != nullptr,
                               dt_cls && dt_score && out_dt_action && out_dt_pixels && out_dt_state && out_dt_tp && out_dt_gt &&
                                   out_dt_iou && out_dt_best,
                               nullptr, 0, &nb, &npb)))
        return rc;
    for (int64_t p = 0; p < na; ++p) DYD_REQUIRE(gt_cls[p] < n_classes, "class id outside the list");
    for (int64_t p = 0; p < nb; ++p) DYD_REQUIRE(dt_cls[p] < n_classes, "class id outside the list");
    hipStream_t st = ctx().stream;
    PolyTableDev ta;
    DevBuf b_xyd, b_pt, b_row, d_ca, d_cb, d_sc, d_lim, d_status, d_poff, d_aact, d_bact, d_apix, d_bpix;
    EvalOutDev res;
    if ((rc = ta.upload(gt_xy, gt_pt_off, gt_row_off, width, height, n_rows, na, npa)) ||
        (rc = poly_column(b_xyd, npb ? dt_xy : nullptr, 16 * (size_t)npb)) ||
        (rc = poly_column(b_pt, nb ? dt_pt_off : nullptr, nb ? 4 * (size_t)(nb + 1) : 0)) ||
        (rc = poly_column(b_row, dt_row_off, 4 * (size_t)(n_rows + 1))) || (rc = poly_column(d_ca, gt_cls, 4 * (size_t)na)) ||
        (rc = poly_column(d_cb, dt_cls, 4 * (size_t)nb)) || (rc = poly_column(d_sc, dt_score, 8 * (size_t)nb)) ||
        (rc = poly_column(d_lim, L.lim, 8 * (size_t)T)) || (rc = d_status.alloc((size_t)n_rows)) ||
        (rc = d_poff.alloc(8 * (size_t)(n_rows + 1))) || (rc = d_aact.alloc((size_t)na)) || (rc = d_bact.alloc((size_t)nb)) ||
        (rc = d_apix.alloc(8 * (size_t)na)) || (rc = d_bpix.alloc(8 * (size_t)nb)) ||
        (rc = res.alloc(na, nb)))
        return rc;
    DYD_HIP(hipStreamSynchronize(st));   // L lives on this frame
    const K22Table a{ta.xy.as<double>(), ta.pt.as<int32_t>(), ta.row.as<int32_t>(), d_ca.as<int32_t>(), na, npa,
                     d_aact.as<uint8_t>(), d_apix.as<int64_t>(), nullptr, nullptr};
    const K22Table b{b_xyd.as<double>(), b_pt.as<int32_t>(), b_row.as<int32_t>(), d_cb.as<int32_t>(), nb, npb,
                     d_bact.as<uint8_t>(), d_bpix.as<int64_t>(), nullptr, nullptr};
    const K22Out o{d_status.as<uint8_t>(), d_poff.as<int64_t>(), nullptr, nullptr, nullptr, nullptr, nullptr};
    SizedOut pairs(K25_PAIRS, st);
    KernelTimer timer(st);
    rc = compare_pairs_launch(a, b, ta.w.as<double>(), ta.h.as<double>(), n_rows, n_classes, max_pixels_per_row, max_pairs_per_row,
                              o, true, pairs, st);
    if (rc) return rc;
    {
        ScratchLease lease(st);   // the score order, one i32 per detection
        void *scr = nullptr;
        if ((rc = lease.get(4 * (size_t)(nb > 0 ? nb : 1), &scr))) return rc;
        const int64_t want = (int64_t)ctx().num_cu * 32;
        hipLaunchKernelGGL(k25_match_kernel, dim3((unsigned)(n_rows < want ? n_rows : want)), dim3(kWave), 0, st, a.row_off, a.cls,
                           a.action, reinterpret_cast<const unsigned long long *>(a.pixels), b.row_off, b.cls, b.action,
                           reinterpret_cast<const unsigned long long *>(b.pixels), d_sc.as<double>(), n_rows, na, nb,
                           d_lim.as<double>(), (int)T, L.minlim, max_dets, o.row_status, o.pair_off, pairs.as<uint32_t>(), res.out(),
                           static_cast<int32_t *>(scr));
        DYD_HIP(hipGetLastError());
    }
    timer.finish();
    const CopyBack back[] = {{out_row_status, d_status.p, (size_t)n_rows}, {out_pair_off, d_poff.p, 8 * (size_t)(n_rows + 1)},
                             {out_gt_action, d_aact.p, (size_t)na}, {out_dt_action, d_bact.p, (size_t)nb},
                             {out_gt_pixels, d_apix.p, 8 * (size_t)na}, {out_dt_pixels, d_bpix.p, 8 * (size_t)nb}};
    for (const CopyBack &c : back)
        if (c.bytes) DYD_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st));
    if ((rc = res.copy_back({out_dt_state, out_dt_tp, out_dt_gt, out_dt_iou, out_dt_best, out_gt_hit, out_gt_best}, st))) return rc;
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
