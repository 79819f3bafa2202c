/*
 * k_rate_profile.hip -- the whole-grid rate profile of a rate curve (pacx_rate_profile, pacx_rate_profile_segments,
 * include/pacx.h): total(t / 64) of pacx_rate_solve at every target t of the range in one pass, a row per uniform
 * segment of the piece.  What k_profile.hip / k_seg_profile.hip do for a band curve, on the other curve: per unit the
 * look-ups of solve_frame (k_rate.hip) are step functions of the target.
 *
 *   k_rate_profile<LDS>  worst[j] <= t / 64 is 64 worst[j] <= t (both scalings exact), so entry j passes from the grid
 *                        index e_j = ceil(64 worst[j]) - t_lo on: 0 where that is at or below t_lo, never where the
 *                        entry is NaN, +inf or above t_hi -- decided by comparisons in double before any cast, the
 *                        rule of k_profile.hip.  Per frame the workgroup's 1024 threads turn the frame's row of worst
 *                        into 16-bit e_j in LDS (G < 65536) with the row of bits beside them; then every thread runs
 *                        solve_frame's bisection with ok(j) := e_j <= g for each grid entry g it owns (PROF_TILES at
 *                        most) and each unit: the cap test on entry J first, at most SOLVE_MAX_LOOKUP halvings, a J
 *                        that would leave its row cut to the row, a unit with steps < 0 does not exist, a frame
 *                        without units adds nothing, a short frame's eight units summed BEFORE (sum + 4 + 7) >> 3.
 *                        Neighbouring g take the same path through a unit, so the LDS reads mostly broadcast.
 *                        A workgroup walks a CONTIGUOUS run of frames, as k_band_profile_seg does, keeps its bytes at
 *                        the entries a thread owns in registers and adds them to the row of the segment it is in when
 *                        that changes and at its end: one 64-bit atomicAdd per entry.  Integer sums; every trip count
 *                        is an argument's or a constant's.
 *                        <false>: a row beyond RATE_ROW_LDS entries (no layout of pacx_rate_curve_layout has one)
 *                        does not go through LDS: every look-up reads the curve and compares 64 worst[j] <= t_lo + g
 *                        in double, the definition itself.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"

using namespace pacx_k;

namespace {

constexpr int PROF_THREADS = 1024;
constexpr int PROF_TILES = (PACX_PROFILE_MAX + PROF_THREADS - 1) / PROF_THREADS;      /* entries a thread owns, at most */
constexpr int PROF_GROUPS = 512;                   /* workgroups at most: two per CU */
constexpr int RATE_ROW_LDS = PACX_SUB * 513;       /* entries of a row kept in LDS: eight units of J <= 512 */
constexpr int SOLVE_MAX_LOOKUP = 12;               /* k_rate.hip's: 1 + ceil(log2(J + 1)) for J < 2048 */
constexpr unsigned E_NEVER = 0xffffu;              /* above every g a thread owns */

static_assert(PROF_TILES * PROF_THREADS < (int)E_NEVER, "grid indices are kept in 16 bits");

/* the workgroup's bytes into one row, and cleared: entry g of thread (w, lane) is base + 64 t.  `base` goes through an
   empty asm so that the entries' addresses and bounds are worked out here and not hoisted out of the frame loop, where
   they would stay in 18 vector registers across every frame and spill (k_seg_profile.hip, flush_row) */
__device__ __forceinline__ void flush_row(long long (&bytes)[PROF_TILES], int base, int n_tiles, int G,
                                          unsigned long long *__restrict__ row)
{
    asm volatile("" : "+v"(base));
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        const int g = base + 64 * t;
        if (t < n_tiles && g < G && bytes[t])
            atomicAdd(&row[g], (unsigned long long)bytes[t]);
        bytes[t] = 0;
    }
}

/* Workgroup b walks the frames [b run, min((b + 1) run, n_cf)); profile: [n_seg][G], row (first_off + cf) / seg_cf
   for frame cf.  row_trips = ceil(row / PROF_THREADS) */
template <bool LDS>
__global__ __launch_bounds__(PROF_THREADS) void k_rate_profile(long long n_cf, int run, long long seg_cf,
                                                              long long first_off, int t_lo, int t_hi, int n_tiles,
                                                              int row, int sub_stride, int row_trips,
                                                              const double *__restrict__ worst,
                                                              const int32_t *__restrict__ bits,
                                                              const int32_t *__restrict__ steps,
                                                              unsigned long long *__restrict__ profile)
{
    __shared__ unsigned short es[LDS ? RATE_ROW_LDS : 1];
    __shared__ int bs[LDS ? RATE_ROW_LDS : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int G = t_hi - t_lo + 1;
    const int base = w * (n_tiles * 64) + lane;

    /* the run, and the segment its first frame lies in: the one division, before anything is held in registers.  What
       the loop carries is 32 bits wide (n_cf < 2^28): the frame, the run's end, the frames left in the segment */
    const int cf0 = blockIdx.x * run;
    const int cf1 = cf0 + run < (int)n_cf ? cf0 + run : (int)n_cf;
    const long long seg0 = (first_off + cf0) / seg_cf;
    const long long left0 = (seg0 + 1) * seg_cf - first_off - cf0;     /* >= 1: frames of segment seg0 from cf0 on */
    const int seg_len = seg_cf < run ? (int)seg_cf : run;              /* beyond the run's length no boundary matters */
    int left = left0 < run ? (int)left0 : run;
    unsigned long long *__restrict__ out = profile + seg0 * G;         /* the row the bytes in registers belong to */

    long long bytes[PROF_TILES];
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t)
        bytes[t] = 0;

    /* segment by segment of the run: the frames of one, then its bytes into its row */
#pragma unroll 1
    for (int cf = cf0; cf < cf1; left = seg_len, out += G) {
        const int end = cf + left < cf1 ? cf + left : cf1;
#pragma unroll 1
        for (; cf < end; ++cf) {
            const int32_t *__restrict__ sp = steps + (long long)cf * PACX_SUB;
            int units = 0;
            for (int sb = 0; sb < PACX_SUB; ++sb)
                units += sp[sb] >= 0 ? 1 : 0;
            if (!units)                            /* a dropped hop: no bytes.  Workgroup-uniform, as all of sp is */
                continue;
            const double *__restrict__ wr = worst + (long long)cf * row;
            const int32_t *__restrict__ br = bits + (long long)cf * row;
            if (LDS) {
                __syncthreads();                   /* the frame before is through with es and bs */
#pragma unroll 1
                for (int k = 0; k < row_trips; ++k) {
                    const int j = tid + k * PROF_THREADS;
                    if (j < row) {
                        /* decided in double: NaN and +inf fail the first comparison, -inf and anything below the
                           range pass the second, and only what lies in (t_lo, t_hi] reaches the cast */
                        const double x = wr[j] * (double)PACX_RATE_TARGET_GRID;
                        unsigned e = E_NEVER;
                        if (x <= (double)t_hi)
                            e = x <= (double)t_lo ? 0u : (unsigned)((int)ceil(x) - t_lo);
                        es[j] = (unsigned short)e;
                        bs[j] = br[j];
                    }
                }
                __syncthreads();
            }
            int fbits[PROF_TILES];
#pragma unroll
            for (int t = 0; t < PROF_TILES; ++t)
                fbits[t] = 0;
            int live = 0;
#pragma unroll 1
            for (int sb = 0; sb < PACX_SUB; ++sb) {
                int J = sp[sb];
                const int at = sb * sub_stride;
                if (J >= row - at)                 /* at + J >= row: never read past the row */
                    J = row - 1 - at;
                if (J < 0)                         /* workgroup-uniform */
                    continue;
                ++live;
                /* ok(j) at grid entry g */
                auto ok = [&](int j, int g) -> bool {
                    if (LDS)
                        return (int)es[at + j] <= g;
                    return wr[at + j] * (double)PACX_RATE_TARGET_GRID <= (double)(t_lo + g);
                };
#pragma unroll
                for (int t = 0; t < PROF_TILES; ++t) {
                    if (t < n_tiles) {
                        const int g = base + 64 * t;
                        int hi = J;
                        if (ok(J, g)) {            /* else capped: the unit takes J */
                            int lo = -1;
                            for (int it = 0; it < SOLVE_MAX_LOOKUP && hi - lo > 1; ++it) {
                                const int mid = (lo + hi) / 2;
                                if (ok(mid, g))
                                    hi = mid;
                                else
                                    lo = mid;
                            }
                        }
                        fbits[t] += LDS ? bs[at + hi] : br[at + hi];
                    }
                }
            }
            /* ---- the frame's bytes and their length prefix (solve_frame's size rule) */
            if (live) {
#pragma unroll
                for (int t = 0; t < PROF_TILES; ++t) {
                    const int nby = (fbits[t] + 4 + 7) >> 3;
                    bytes[t] += nby > 0 ? (long long)nby + 4 : 0ll;
                }
            }
        }
        flush_row(bytes, base, n_tiles, G, out);
    }
}

}  // namespace

void pacx_k::pacx_launch_rate_profile_segments(long long n_cf, int row, int sub_stride, const double *worst,
                                               const int32_t *bits, const int32_t *steps, long long seg_cf,
                                               long long first_off, int t_lo, int t_hi, int64_t *profile, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const int G = t_hi - t_lo + 1, n_tiles = (G + PROF_THREADS - 1) / PROF_THREADS;
    const int run = (int)((n_cf + PROF_GROUPS - 1) / PROF_GROUPS);
    const unsigned grid = (unsigned)((n_cf + run - 1) / run);          /* no workgroup without a frame */
    const int row_trips = (row + PROF_THREADS - 1) / PROF_THREADS;
    const auto kernel = row <= RATE_ROW_LDS ? k_rate_profile<true> : k_rate_profile<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(PROF_THREADS), 0, st, n_cf, run, seg_cf, first_off, t_lo, t_hi, n_tiles,
                       row, sub_stride, row_trips, worst, bits, steps, (unsigned long long *)profile);
}
