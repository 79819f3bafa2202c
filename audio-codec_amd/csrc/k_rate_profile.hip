/*
 * k_rate_profile.hip -- the whole-grid rate profile of a rate curve (pacx_rate_profile, pacx_rate_profile_segments,
 * include/pacx.h): total(t / 64) of pacx_rate_solve at every target t of the range in one pass, a row per uniform
 * segment of the piece.  What k_profile.hip / k_seg_profile.hip do for a band curve, on the other curve: per unit the
 * look-ups of solve_frame (pick_dev.h) are step functions of the target.
 *
 *   k_rate_profile<LDS>  Entry j of a row passes from the grid index e_j = grid_threshold(worst[j]) on (grid_dev.h).
 *                        Per frame the workgroup's 1024 threads turn the frame's row of worst into 16-bit e_j in LDS
 *                        (G < 65536) with the row of bits beside them; then every thread runs curve_lookup
 *                        (pick_dev.h) with ok(j) := e_j <= g for each grid entry g it owns (PROF_TILES at most) and
 *                        each unit, under solve_frame's rules: a J that would leave its row cut to the row, a unit
 *                        with steps < 0 does not exist, a frame without units adds nothing, a short frame's eight
 *                        units summed BEFORE (sum + 4 + 7) >> 3.  Neighbouring g take the same path through a unit,
 *                        so the LDS reads mostly broadcast.  A workgroup walks a CONTIGUOUS run of frames (RunWalk,
 *                        grid_dev.h), as k_band_profile_seg does, keeps its bytes at the entries a thread owns in
 *                        registers and adds them to the row of the segment it is in when that changes and at its end
 *                        (flush_row): one 64-bit atomicAdd per entry.  Integer sums; every trip count is an
 *                        argument's or a constant's.
 *                        <false>: a row beyond RATE_ROW_LDS entries (no layout of pacx_rate_curve_layout has one)
 *                        does not go through LDS: every look-up reads the curve and compares 64 worst[j] <= t_lo + g
 *                        in double, the definition itself.
 */
#include <hip/hip_runtime.h>

#include "grid_dev.h"
#include "pick_dev.h"

using namespace pacx_k;

namespace {

constexpr int RATE_ROW_LDS = PACX_SUB * 513;       /* entries of a row kept in LDS: eight units of J <= 512 */
constexpr unsigned E_NEVER = 0xffffu;              /* grid_threshold's "never" as kept here: above every g a thread
                                                      owns, those beyond G included */

static_assert(PROF_TILES * PROF_THREADS < (int)E_NEVER, "grid indices are kept in 16 bits");

/* profile: [n_seg][G], row (first_off + cf) / seg_cf for frame cf.  row_trips = ceil(row / PROF_THREADS) */
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
    RunWalk W = run_walk(n_cf, run, seg_cf, first_off, G, profile);

    long long bytes[PROF_TILES];
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t)
        bytes[t] = 0;

    /* segment by segment of the run: the frames of one, then its bytes into its row */
#pragma unroll 1
    for (int cf = W.cf0; cf < W.cf1; W.left = W.seg_len, W.out += G) {
        const int end = cf + W.left < W.cf1 ? cf + W.left : W.cf1;
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
                        const unsigned e = grid_threshold(wr[j], t_lo, t_hi);
                        es[j] = (unsigned short)(e < (unsigned)G ? e : E_NEVER);
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
#pragma unroll
                for (int t = 0; t < PROF_TILES; ++t) {
                    if (t < n_tiles) {
                        const int g = base + 64 * t;
                        bool capped = false;       /* a capped unit takes J: the profile keeps sizes only */
                        const int hi = curve_lookup(J, [&](int j) -> bool {
                            if (LDS)
                                return (int)es[at + j] <= g;
                            return wr[at + j] * (double)PACX_RATE_TARGET_GRID <= (double)(t_lo + g);
                        }, capped);
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
        flush_row(bytes, base, n_tiles, G, W.out);
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
