/*
 * k_seg_profile.hip -- the whole-grid rate profile per segment of a stream (pacx_band_profile_segments,
 * pacx_profile_solve_segments, pacx_profile_clamp_add, include/pacx.h).  A profile row per segment is additive over
 * pieces of a stream in the same way the stream's profile is (k_profile.hip), so a segmented solve and the two-level
 * peak solve of a stream of any length keep the rows of the segments a piece touches, a few words per segment and one
 * stream profile of G words.  Segments are uniform stretches given by value: frame cf of the piece lies in local
 * segment (first_off + cf) / seg_cf.
 *
 *   k_band_profile_seg   band_profile_frame (grid_dev.h), k_band_profile's work per frame, on a CONTIGUOUS run of
 *                        frames (RunWalk, grid_dev.h): the workgroup adds its bytes to the row of the segment it is in
 *                        whenever that segment changes and at its end (flush_row), one 64-bit atomicAdd per entry.
 *   k_profile_solve_seg  one wave per row: profile_decide (grid_dev.h) against the row's limit (every lane takes the
 *                        same wave-uniform path), then worst_above = max of the row from the target found on, the
 *                        lanes striding over it.  A negative limit is never met.
 *   k_profile_clamp_add  stream_profile[g] += sum over s of row_s[max(g, result[s].t - t_lo)]: a thread per entry and
 *                        CLAMP_SEGS rows per workgroup and trip, one 64-bit atomicAdd per thread.
 */
#include <hip/hip_runtime.h>

#include "grid_dev.h"

using namespace pacx_k;

namespace {

constexpr int CLAMP_THREADS = 256, CLAMP_SEGS = 32, CLAMP_GRID_Y = 4096;

/* diff: n_tiles * PROF_THREADS int32 (dynamic LDS), see band_profile_frame; profile: [n_seg][G] */
__global__ __launch_bounds__(PROF_THREADS) void k_band_profile_seg(PacxTables T, long long n_cf, int run,
                                                                  long long seg_cf, long long first_off, int t_lo,
                                                                  int t_hi, int n_tiles, const double *__restrict__ nmr,
                                                                  const int32_t *__restrict__ cap,
                                                                  const int32_t *__restrict__ cap_alloc,
                                                                  unsigned long long *__restrict__ profile)
{
    extern __shared__ int diff[];
    __shared__ int wave_tot[PROF_WAVES];
    __shared__ int unit_ca[PACX_SUB];
    const BandProfileWg P = band_profile_wg(T, t_lo, t_hi, n_tiles);
    RunWalk W = run_walk(n_cf, run, seg_cf, first_off, P.G, profile);

    long long bytes[PROF_TILES];
    int fbits[PROF_TILES];
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        bytes[t] = 0;
        fbits[t] = 0;
        if (t < n_tiles)
            diff[P.base + 64 * t] = 0;
    }

#pragma unroll 1
    for (int cf = W.cf0; cf < W.cf1; W.left = W.seg_len, W.out += P.G) {
        const int end = cf + W.left < W.cf1 ? cf + W.left : W.cf1;
#pragma unroll 1
        for (; cf < end; ++cf)
            band_profile_frame(T, P, cf, t_lo, t_hi, n_tiles, nmr, cap, cap_alloc, diff, wave_tot, unit_ca, bytes, fbits);
        flush_row(bytes, P.base, n_tiles, P.G, W.out);
    }
}

/* one wave per row.  profile_decide on the row against limit[s], taken by every lane alike (the loads are
   wave-uniform).  Then the largest entry
   of the row from the target found on: `strides` = ceil(G / 64) trips, the lanes 64 apart. */
__global__ __launch_bounds__(64) void k_profile_solve_seg(const unsigned long long *__restrict__ profile,
                                                         const long long *__restrict__ limits, int t_lo, int t_hi,
                                                         int halvings, int strides, pacx_rate_result *result,
                                                         long long *worst_above)
{
    const int lane = threadIdx.x, G = t_hi - t_lo + 1;
    const long long s = blockIdx.x;
    const unsigned long long *__restrict__ row = profile + s * G;
    const long long limit = limits[s];
    int t = t_hi, met = 0;
    if (limit >= 0)                                /* a negative limit is never met */
        t = profile_decide(row, limit, t_lo, t_hi, halvings, met);
    if (lane == 0) {
        result[s].t = t;
        result[s].met = met;
        result[s].total = (int64_t)row[t - t_lo];
    }
    if (!worst_above)
        return;
    long long worst = 0;                           /* sizes are not negative */
    for (int i = 0; i < strides; ++i) {
        const int g = t - t_lo + lane + 64 * i;
        if (g < G) {
            const long long v = (long long)row[g];
            worst = v > worst ? v : worst;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(worst, off, 64);
        worst = o > worst ? o : worst;
    }
    if (lane == 0)
        worst_above[s] = worst;
}

/* thread g of workgroup (x, y): CLAMP_SEGS rows of the profile at max(g, their floor) per trip, the workgroups of a
   column gridDim.y CLAMP_SEGS rows apart (`trips` = what the launcher worked out from n_seg), one atomicAdd */
__global__ __launch_bounds__(CLAMP_THREADS) void k_profile_clamp_add(const unsigned long long *__restrict__ profile,
                                                                    const pacx_rate_result *__restrict__ result,
                                                                    long long n_seg, int trips, int t_lo, int t_hi,
                                                                    unsigned long long *__restrict__ stream_profile)
{
    const int G = t_hi - t_lo + 1;
    const int g = blockIdx.x * CLAMP_THREADS + threadIdx.x;
    if (g >= G)
        return;
    unsigned long long sum = 0ull;
#pragma unroll 1
    for (int k = 0; k < trips; ++k) {
        const long long s0 = ((long long)k * gridDim.y + blockIdx.y) * CLAMP_SEGS;
#pragma unroll 4
        for (int i = 0; i < CLAMP_SEGS; ++i) {
            const long long s = s0 + i;
            if (s < n_seg) {                       /* workgroup-uniform */
                int u = result[s].t - t_lo;        /* in the range by construction; clamped: no read leaves the row */
                u = u < 0 ? 0 : (u > G - 1 ? G - 1 : u);
                sum += profile[s * G + (g > u ? g : u)];
            }
        }
    }
    if (sum)
        atomicAdd(&stream_profile[g], sum);
}

}  // namespace

void pacx_k::pacx_launch_band_profile_segments(const PacxTables &T, long long n_cf, long long seg_cf, long long first_off,
                                               int t_lo, int t_hi, const double *nmr, const int32_t *cap,
                                               const int32_t *cap_alloc, int64_t *profile, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const int G = t_hi - t_lo + 1, n_tiles = (G + PROF_THREADS - 1) / PROF_THREADS;
    const int run = (int)((n_cf + PROF_GROUPS - 1) / PROF_GROUPS);
    const unsigned grid = (unsigned)((n_cf + run - 1) / run);          /* no workgroup without a frame */
    hipLaunchKernelGGL(k_band_profile_seg, dim3(grid), dim3(PROF_THREADS), (size_t)n_tiles * PROF_THREADS * sizeof(int), st,
                       T, n_cf, run, seg_cf, first_off, t_lo, t_hi, n_tiles, nmr, cap, cap_alloc,
                       (unsigned long long *)profile);
}

void pacx_k::pacx_launch_profile_solve_segments(long long n_seg, const int64_t *profile, const int64_t *limit_bytes,
                                                int t_lo, int t_hi, pacx_rate_result *result, int64_t *worst_above,
                                                hipStream_t st)
{
    if (n_seg <= 0)
        return;
    const int G = t_hi - t_lo + 1;
    hipLaunchKernelGGL(k_profile_solve_seg, dim3((unsigned)n_seg), dim3(64), 0, st, (const unsigned long long *)profile,
                       (const long long *)limit_bytes, t_lo, t_hi, pacx_rate_solve_pairs(t_lo, t_hi) - 2, (G + 63) / 64,
                       result, (long long *)worst_above);
}

void pacx_k::pacx_launch_profile_clamp_add(long long n_seg, const int64_t *profile, const pacx_rate_result *result,
                                           int t_lo, int t_hi, int64_t *stream_profile, hipStream_t st)
{
    if (n_seg <= 0)
        return;
    const int G = t_hi - t_lo + 1;
    const long long groups = (n_seg + CLAMP_SEGS - 1) / CLAMP_SEGS;
    const unsigned gy = (unsigned)(groups < CLAMP_GRID_Y ? groups : CLAMP_GRID_Y);   /* a grid's y has 16 bits */
    const int trips = (int)((groups + gy - 1) / gy);
    const dim3 grid((unsigned)((G + CLAMP_THREADS - 1) / CLAMP_THREADS), gy);
    hipLaunchKernelGGL(k_profile_clamp_add, grid, dim3(CLAMP_THREADS), 0, st, (const unsigned long long *)profile, result,
                       n_seg, trips, t_lo, t_hi, (unsigned long long *)stream_profile);
}
