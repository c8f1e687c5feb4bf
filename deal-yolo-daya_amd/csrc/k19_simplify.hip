// k19_simplify.hip — K19: Douglas-Peucker simplification of every annotation polygon of a table (the polygon simplify step).
//
// Per polygon (K14's polygons: V = the ptList points, m = len(V)) which vertices stay, by the rule of include/dyd.h and DESIGN
// §5q: vertex 0 and the vertex b farthest from it are anchors, the root segments are (0, b) and (b, m) (index m = vertex 0), a
// segment (i, j) splits at its interior vertex k* of largest squared segment distance s* when s* > tolerance^2, and when neither
// root splits the one with the larger s* splits anyway.  Every test is IEEE f64 without contraction, the division the correctly
// rounded one.  A split depends on its segment alone, so the kernels below evaluate the segments in rounds, not recursively, and
// give the bits the recursive form gives.
//
// Layout in HBM: xy = P x (x, y) f64 (16-B aligned), pt_off = B+1 int32.  Out: keep = P u8 (1 = the vertex stays), action = B u8
// (0 kept, 1 simplified, 2 bad_coords, 3 too_few_points), kept = B int32, dev2 = B f64.  The outputs have a fixed size: no scan.
//
// Mapping, tiered by m so that short polygons never wait behind a long one.
//   1. k19_lane_kernel, a lane per polygon over a persistent grid.  m <= lane_points (default 32, at most 64): the lane runs the
//      whole rule with the kept set as a 64-bit mask in registers and the vertices from L1 / L2; each round walks the kept bits
//      and evaluates every segment that still has interior vertices.  A longer polygon only goes on one of two work lists.
//   2. k19_block_kernel<true>, a workgroup per listed polygon of m <= lds_points (default and at most 1024): the points staged in
//      LDS, the current segments of a round in an LDS queue.  Each wave takes segments from the queue, its lanes stride over the
//      interior vertices, a shuffle arg-max gives (s*, k*), lane 0 marks k* and queues the two halves for the next round.  One
//      barrier per round; the rounds go on until the queue is empty, so no depth is fixed (a comb takes ~m rounds).
//   3. k19_block_kernel<false>, the same code for any larger m: the points read from HBM / L2, the two queues in a scratch buffer
//      of 8 bytes per point of the table (a round never holds more than m / 2 segments with interior vertices).
// Work is O(m * depth) distance evaluations per polygon: O(m log m) for a round outline, O(m^2) for a comb, like K14's pair test.
// No kernel indexes a per-lane array at run time: no scratch registers.
#include "k13_poly.h"
#include "poly_table.h"

namespace dyd {

constexpr int K19_BLOCK = 256;
constexpr int K19_WAVES = K19_BLOCK / kWave;
constexpr int K19_LANE_POINTS = 32;          // default: polygons up to this many points run in one lane (at most 64: the mask)
constexpr int K19_LANE_MAX = 64;
constexpr int K19_LDS_POINTS = 1024;         // default and largest polygon whose points a workgroup stages in LDS

enum : uint8_t { SIMP_KEPT = 0, SIMP_SIMPLIFIED = 1, SIMP_BAD_COORDS = 2, SIMP_TOO_FEW = 3 };

__device__ __forceinline__ double2 k19_v(const double2 *p, int k) { return p[k]; }

__device__ __forceinline__ bool k19_bad(double2 v) { return !(fabs(v.x) < K13_LIMIT) || !(fabs(v.y) < K13_LIMIT); }

// s(k; i, j) of the definition: the squared distance of v from the segment (P, Q)
__device__ __forceinline__ double k19_dist2(double2 P, double2 Q, double2 v) {
    const double dx = Q.x - P.x, dy = Q.y - P.y, ex = v.x - P.x, ey = v.y - P.y;
    const double L2 = dx * dx + dy * dy;
    const double t = dx * ex + dy * ey;
    if (L2 == 0.0 || t <= 0.0) return ex * ex + ey * ey;
    if (t >= L2) {
        const double fx = v.x - Q.x, fy = v.y - Q.y;
        return fx * fx + fy * fy;
    }
    const double c = dx * ey - dy * ex;
    return (c * c) / L2;
}

// (s, k) beats (bs, bk): the larger s, ties to the lower k
__device__ __forceinline__ bool k19_better(double s, int k, double bs, int bk) { return s > bs || (s == bs && k < bk); }

// ---- 1. the lane tier ---------------------------------------------------------------------------------------------------
// the interior vertex of (i, j) with the largest s, one lane, the points from memory; j == m stands for vertex 0
__device__ __forceinline__ void k19_lane_seg(const double2 *p, int m, int i, int j, double &s_best, int &k_best) {
    const double2 P = k19_v(p, i), Q = k19_v(p, j == m ? 0 : j);
    s_best = -1.0;
    k_best = -1;
    for (int k = i + 1; k < j; ++k) {
        const double s = k19_dist2(P, Q, k19_v(p, k));
        if (s > s_best) { s_best = s; k_best = k; }
    }
}

__global__ __launch_bounds__(K19_BLOCK) void k19_lane_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                             int64_t n_polys, int64_t n_points, double e2, int32_t lane_points,
                                                             int32_t lds_points, uint8_t *__restrict__ out_keep,
                                                             uint8_t *__restrict__ out_action, int32_t *__restrict__ out_kept,
                                                             double *__restrict__ out_dev2, int32_t *__restrict__ work_lds,
                                                             int32_t *__restrict__ work_big, uint32_t *__restrict__ n_work) {
    const int64_t stride = (int64_t)gridDim.x * K19_BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * K19_BLOCK + threadIdx.x; p < n_polys; p += stride) {
        const int32_t a = max(pt_off[p], 0), b_end = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);   // as K13
        const int m = b_end - a;
        if (m >= 4 && m > lane_points) {       // the block tiers decide everything, bad_coords included
            if (m <= lds_points) work_lds[atomicAdd(n_work, 1u)] = (int32_t)p;
            else work_big[atomicAdd(n_work + 1, 1u)] = (int32_t)p;
            continue;
        }
        const double2 *v = reinterpret_cast<const double2 *>(xy) + a;
        uint8_t *keep = out_keep + a;
        bool bad = false;
        double d_best = 0.0;
        int b = 0;
        if (m > 0) {
            const double2 v0 = k19_v(v, 0);
            for (int k = 0; k < m; ++k) {
                const double2 c = k19_v(v, k);
                bad |= k19_bad(c);
                const double ux = c.x - v0.x, uy = c.y - v0.y, d = ux * ux + uy * uy;
                if (d > d_best) { d_best = d; b = k; }
            }
        }
        uint8_t action = bad ? SIMP_BAD_COORDS : (m < 4 ? SIMP_TOO_FEW : SIMP_KEPT);
        unsigned long long mask = ~0ull;       // bit k: vertex k stays (bits >= m unused)
        double dev2 = 0.0;
        int kept = m;
        if (!bad && m >= 4 && d_best != 0.0) {  // m <= lane_points <= 64
            mask = 1ull | (1ull << b);
            kept = 2;
            // the roots, with the forced split
            double s0, s1;
            int k0, k1;
            k19_lane_seg(v, m, 0, b, s0, k0);
            k19_lane_seg(v, m, b, m, s1, k1);
            bool split0 = k0 >= 0 && s0 > e2, split1 = k1 >= 0 && s1 > e2;
            if (!split0 && !split1) {
                if (k0 >= 0 && (k1 < 0 || s0 >= s1)) split0 = true;
                else split1 = true;
            }
            if (split0) { mask |= 1ull << k0; ++kept; }
            if (split1) { mask |= 1ull << k1; ++kept; }
            // rounds: every segment between two kept vertices that has interior vertices, until none splits
            bool changed = true;
            while (changed) {
                changed = false;
                dev2 = 0.0;
                unsigned long long now = mask;
                int i = 0;
                while (i < m) {
                    const unsigned long long rest = (i + 1 < 64) ? (mask >> (i + 1)) << (i + 1) : 0ull;
                    const int j = rest ? min(__ffsll((long long)rest) - 1, m) : m;
                    if (j - i >= 2) {
                        double s;
                        int k;
                        k19_lane_seg(v, m, i, j, s, k);
                        if (s > e2) { now |= 1ull << k; ++kept; changed = true; }
                        else dev2 = fmax(dev2, s);
                    }
                    i = j;
                }
                mask = now;
            }
            action = kept < m ? SIMP_SIMPLIFIED : SIMP_KEPT;
        }
        for (int k = 0; k < m; ++k) keep[k] = (uint8_t)((mask >> (k & 63)) & 1ull);
        out_action[p] = action;
        out_kept[p] = kept;
        out_dev2[p] = dev2;
    }
}

// ---- 2. / 3. the block tiers --------------------------------------------------------------------------------------------
template <bool LDS>
struct K19Stage {                              // the points and the two segment queues of one polygon in LDS
    double2 xy[K19_LDS_POINTS];
    int2 q[2][K19_LDS_POINTS / 2];
};
template <>
struct K19Stage<false> {};

struct K19Ctl {
    double red_s[K19_WAVES];
    int red_k[K19_WAVES];
    double root_s[2];
    int root_k[2];
    int n[3];                                  // segments queued for round r in n[r % 3]
    int kept;
    unsigned long long dev2;                   // bits of the largest s* of a segment that ended without a split
    int go;
};

// arg-max over the wave: every lane ends with the best (s, k) of the 64
__device__ __forceinline__ void k19_wave_best(double &s, int &k) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double os = __shfl_xor(s, d);
        const int ok = __shfl_xor(k, d);
        if (k19_better(os, ok, s, k)) { s = os; k = ok; }
    }
}

template <bool LDS>
__global__ __launch_bounds__(K19_BLOCK) void k19_block_kernel(const double *__restrict__ xy, const int32_t *__restrict__ pt_off,
                                                              int64_t n_points, double e2, const int32_t *__restrict__ work,
                                                              const uint32_t *__restrict__ n_work, int2 *__restrict__ queues,
                                                              uint8_t *__restrict__ out_keep, uint8_t *__restrict__ out_action,
                                                              int32_t *__restrict__ out_kept, double *__restrict__ out_dev2) {
    __shared__ K19Stage<LDS> T;
    __shared__ K19Ctl S;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t total = *n_work;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int32_t p = work[w];
        const int32_t a = max(pt_off[p], 0), b_end = (int32_t)min((int64_t)max(pt_off[p + 1], a), n_points);
        const int m = b_end - a;               // 4 <= m, and m <= K19_LDS_POINTS when LDS
        const double2 *v = reinterpret_cast<const double2 *>(xy) + a;
        uint8_t *keep = out_keep + a;
        int2 *q0, *q1;
        if constexpr (LDS) { q0 = T.q[0]; q1 = T.q[1]; }
        else { q0 = queues + a; q1 = queues + a + m / 2; }
        auto pt = [&](int k) -> double2 {
            if constexpr (LDS) return T.xy[k];
            else return v[k];
        };
        __syncthreads();                       // the previous polygon is done with T and S
        // bad_coords, the stage, and b = the vertex farthest from vertex 0
        const double2 v0 = v[0];
        bool bad = false;
        double bs = 0.0;
        int bk = 0;
        for (int k = tid; k < m; k += K19_BLOCK) {
            const double2 c = v[k];
            if constexpr (LDS) T.xy[k] = c;
            bad |= k19_bad(c);
            const double ux = c.x - v0.x, uy = c.y - v0.y, d = ux * ux + uy * uy;
            if (d > bs) { bs = d; bk = k; }
        }
        k19_wave_best(bs, bk);
        if (lane == 0) { S.red_s[wave] = bs; S.red_k[wave] = bk; }
        bad = __syncthreads_or(bad);           // also: the stage and the partial results are visible
#pragma unroll
        for (int x = 0; x < K19_WAVES; ++x)
            if (k19_better(S.red_s[x], S.red_k[x], bs, bk)) { bs = S.red_s[x]; bk = S.red_k[x]; }
        const int b = bk;
        if (bad || bs == 0.0) {                // untouched
            for (int k = tid; k < m; k += K19_BLOCK) keep[k] = 1;
            if (tid == 0) {
                out_action[p] = bad ? SIMP_BAD_COORDS : SIMP_KEPT;
                out_kept[p] = m;
                out_dev2[p] = 0.0;
            }
            continue;
        }
        for (int k = tid; k < m; k += K19_BLOCK) keep[k] = (uint8_t)(k == 0 || k == b);
        // the interior vertex of (i, j) with the largest s, by one wave; j == m stands for vertex 0
        auto wave_seg = [&](int i, int j, double &s, int &k_best) {
            const double2 P = pt(i), Q = pt(j == m ? 0 : j);
            s = -1.0;
            k_best = 0x7fffffff;
            for (int k = i + 1 + lane; k < j; k += kWave) {
                const double sk = k19_dist2(P, Q, pt(k));
                if (sk > s) { s = sk; k_best = k; }
            }
            k19_wave_best(s, k_best);
        };
        // the roots (waves 0 and 1), then thread 0 decides them with the forced split and fills the first queue
        if (wave < 2) {
            double s;
            int k;
            wave_seg(wave == 0 ? 0 : b, wave == 0 ? b : m, s, k);
            if (lane == 0) { S.root_s[wave] = s; S.root_k[wave] = k; }
        }
        __syncthreads();                       // the roots' results; every keep[] byte is written before any is set below
        if (tid == 0) {
            const double s0 = S.root_s[0], s1 = S.root_s[1];
            const int k0 = S.root_k[0], k1 = S.root_k[1];
            const bool has0 = b >= 2, has1 = m - b >= 2;
            bool split0 = has0 && s0 > e2, split1 = has1 && s1 > e2;
            if (!split0 && !split1) {
                if (has0 && (!has1 || s0 >= s1)) split0 = true;
                else split1 = true;
            }
            int n = 0, kept = 2;
            double dev2 = 0.0;
            if (split0) {
                keep[k0] = 1;
                ++kept;
                if (k0 >= 2) q0[n++] = make_int2(0, k0);
                if (b - k0 >= 2) q0[n++] = make_int2(k0, b);
            } else if (has0) {
                dev2 = fmax(dev2, s0);
            }
            if (split1) {
                keep[k1] = 1;
                ++kept;
                if (k1 - b >= 2) q0[n++] = make_int2(b, k1);
                if (m - k1 >= 2) q0[n++] = make_int2(k1, m);
            } else if (has1) {
                dev2 = fmax(dev2, s1);
            }
            S.n[0] = n;
            S.n[1] = 0;
            S.n[2] = 0;
            S.kept = kept;
            S.dev2 = (unsigned long long)__double_as_longlong(dev2);
        }
        // rounds: round r takes its segments from queue r & 1 and queues their halves for round r + 1
        for (int r = 0;; ++r) {
            __syncthreads();                   // round r's queue and count are complete
            const int n = S.n[r % 3];
            if (n == 0) break;
            if (tid == 0) S.n[(r + 2) % 3] = 0;    // last read at the top of round r - 1, next used in round r + 1
            const int2 *cur = (r & 1) ? q1 : q0;
            int2 *nxt = (r & 1) ? q0 : q1;
            for (int x = wave; x < n; x += K19_WAVES) {
                const int2 sg = cur[x];
                double s;
                int k;
                wave_seg(sg.x, sg.y, s, k);
                if (lane == 0) {
                    if (s > e2) {
                        keep[k] = 1;
                        atomicAdd(&S.kept, 1);
                        const int c = (k - sg.x >= 2) + (sg.y - k >= 2);
                        if (c) {
                            int at = atomicAdd(&S.n[(r + 1) % 3], c);
                            if (k - sg.x >= 2) nxt[at++] = make_int2(sg.x, k);
                            if (sg.y - k >= 2) nxt[at] = make_int2(k, sg.y);
                        }
                    } else {
                        atomicMax(&S.dev2, (unsigned long long)__double_as_longlong(s));   // s >= 0: the bits order like s
                    }
                }
            }
        }
        if (tid == 0) {
            const int kept = S.kept;
            out_action[p] = kept < m ? SIMP_SIMPLIFIED : SIMP_KEPT;
            out_kept[p] = kept;
            out_dev2[p] = __longlong_as_double((long long)S.dev2);
        }
    }
}

// dyd_set_option("k19_lane_points" / "k19_lds_points", n): the tier limits; <= 0 restores the default, larger values are capped
static int g_k19_lane_points = K19_LANE_POINTS, g_k19_lds_points = K19_LDS_POINTS;

void set_k19_lane_points(int v) { g_k19_lane_points = v > 0 ? (v < K19_LANE_MAX ? v : K19_LANE_MAX) : K19_LANE_POINTS; }
void set_k19_lds_points(int v) { g_k19_lds_points = v > 0 ? (v < K19_LDS_POINTS ? v : K19_LDS_POINTS) : K19_LDS_POINTS; }

static int k19_launch(const double *xy, const int32_t *pt_off, int64_t n_polys, int64_t n_points, double tolerance,
                      uint8_t *out_keep, uint8_t *out_action, int32_t *out_kept, double *out_dev2, hipStream_t st) {
    if (n_polys == 0) return DYD_OK;
    DevBuf d_work, d_queues;
    int rc;
    if ((rc = d_work.alloc(8 * (size_t)n_polys + 16, st)) || (rc = d_queues.alloc(8 * (size_t)n_points, st))) return rc;
    int32_t *work_lds = d_work.as<int32_t>(), *work_big = work_lds + n_polys;
    uint32_t *n_work = reinterpret_cast<uint32_t *>(work_big + n_polys);
    DYD_HIP(hipMemsetAsync(n_work, 0, 8, st));
    const double e2 = tolerance * tolerance;
    const int64_t tiles = ceil_div(n_polys, (int64_t)K19_BLOCK);
    const int64_t want = (int64_t)ctx().num_cu * 8;
    hipLaunchKernelGGL(k19_lane_kernel, dim3((unsigned)(tiles < want ? tiles : want)), dim3(K19_BLOCK), 0, st, xy, pt_off, n_polys,
                       n_points, e2, g_k19_lane_points, g_k19_lds_points, out_keep, out_action, out_kept, out_dev2, work_lds,
                       work_big, n_work);
    const unsigned blocks = (unsigned)(n_polys < want ? n_polys : want);
    hipLaunchKernelGGL(k19_block_kernel<true>, dim3(blocks), dim3(K19_BLOCK), 0, st, xy, pt_off, n_points, e2, work_lds, n_work,
                       (int2 *)nullptr, out_keep, out_action, out_kept, out_dev2);
    hipLaunchKernelGGL(k19_block_kernel<false>, dim3(blocks), dim3(K19_BLOCK), 0, st, xy, pt_off, n_points, e2, work_big, n_work + 1,
                       d_queues.as<int2>(), out_keep, out_action, out_kept, out_dev2);
    DYD_HIP(hipGetLastError());
    return DYD_OK;
}

static bool k19_tolerance_ok(double t) { return std::isfinite(t) && t >= 0.0 && t < K13_LIMIT; }

}  // namespace dyd

using namespace dyd;

extern "C" {

int dyd_simplify_polygons_dev(const double *xy, const int32_t *pt_off, int64_t n_polys, int64_t n_points, double tolerance,
                              uint8_t *out_keep, uint8_t *out_action, int32_t *out_kept, double *out_dev2, void *stream) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_polys >= 0 && n_points >= 0, "negative size");
    DYD_REQUIRE(n_polys < (1LL << 31) && n_points < (1LL << 31), "n_polys or n_points exceeds int32 offsets");
    DYD_REQUIRE(k19_tolerance_ok(tolerance), "tolerance must be finite, >= 0 and < 2^43");
    DYD_REQUIRE(n_polys == 0 || (pt_off && out_action && out_kept && out_dev2), "null pointer");
    DYD_REQUIRE(n_points == 0 || (xy && out_keep), "null pointer");
    DYD_REQUIRE((reinterpret_cast<uintptr_t>(xy) & 15) == 0, "xy must be 16-byte aligned");
    return k19_launch(xy, pt_off, n_polys, n_points, tolerance, out_keep, out_action, out_kept, out_dev2, pick_stream(stream));
}

int dyd_simplify_polygons(const double *xy, const int32_t *pt_off, int64_t n_polys, double tolerance, uint8_t *out_keep,
                          uint8_t *out_action, int32_t *out_kept, double *out_dev2) {
    DYD_API_ENTER();
    DYD_REQUIRE(n_polys >= 0 && n_polys < (1LL << 31), "n_polys negative or beyond int32 offsets");
    DYD_REQUIRE(k19_tolerance_ok(tolerance), "tolerance must be finite, >= 0 and < 2^43");
    // the table checks of the polygon steps, on one row that holds every polygon
    const int32_t row_off[2] = {0, (int32_t)n_polys};
    const double size = 1.0;
    int64_t nb = 0, np = 0;
    int rc = poly_table_check(xy, pt_off, row_off, 1, &size, &size, true, out_action && out_kept && out_dev2, nullptr, 0, &nb, &np);
    if (rc) return rc;
    DYD_REQUIRE(np == 0 || out_keep, "null pointer");
    if (nb == 0) return DYD_OK;
    hipStream_t st = ctx().stream;
    DevBuf d_xy, d_pt, d_keep, d_act, d_kept, d_dev2;
    if ((rc = poly_column(d_xy, xy, 16 * (size_t)np)) || (rc = poly_column(d_pt, pt_off, 4 * (size_t)(nb + 1))) ||
        (rc = d_keep.alloc((size_t)np)) || (rc = d_act.alloc((size_t)nb)) || (rc = d_kept.alloc(4 * (size_t)nb)) ||
        (rc = d_dev2.alloc(8 * (size_t)nb)))
        return rc;
    KernelTimer timer(st);
    rc = k19_launch(d_xy.as<double>(), d_pt.as<int32_t>(), nb, np, tolerance, d_keep.as<uint8_t>(), d_act.as<uint8_t>(),
                    d_kept.as<int32_t>(), d_dev2.as<double>(), st);
    if (rc) return rc;
    timer.finish();
    if (np) DYD_HIP(hipMemcpyAsync(out_keep, d_keep.p, (size_t)np, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_action, d_act.p, (size_t)nb, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_kept, d_kept.p, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipMemcpyAsync(out_dev2, d_dev2.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    DYD_HIP(hipStreamSynchronize(st));
    return DYD_OK;
}

}  // extern "C"
