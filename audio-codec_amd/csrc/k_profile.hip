/*
 * k_profile.hip -- the size of a band curve at every target of the grid in one pass (pacx_band_profile), and the
 * solve's decision on such a profile (pacx_profile_solve, include/pacx.h).  total(T) of pacx_band_pick is a sum of
 * integers over channel-frames, so profile[g] = total((t_lo + g) / 64) is additive over pieces of a stream in any
 * order: a stream too long for one batch is analysed piece by piece into G 64-bit words and solved on those.
 *
 *   k_band_profile    band_profile_frame (grid_dev.h) for a strided share of the channel-frames: workgroup b of 16
 *                     waves takes the frames b, b + 512, ...  The frame's bits and the workgroup's bytes at the entries
 *                     a thread owns stay in its registers (PROF_TILES of each); at its end the workgroup adds its bytes
 *                     to the profile, one 64-bit atomicAdd per entry.  k_band_profile_seg (k_seg_profile.hip) is the
 *                     other walk over the same frame work.
 *   k_profile_solve   one thread: profile_decide (grid_dev.h) on the profile.
 */
#include <hip/hip_runtime.h>

#include "grid_dev.h"

using namespace pacx_k;

namespace {

/* diff: n_tiles * PROF_THREADS int32 (dynamic LDS), see band_profile_frame */
__global__ __launch_bounds__(PROF_THREADS) void k_band_profile(PacxTables T, long long n_cf, int t_lo, int t_hi, int n_tiles,
                                                              const double *__restrict__ nmr,
                                                              const int32_t *__restrict__ cap,
                                                              const int32_t *__restrict__ cap_alloc,
                                                              unsigned long long *__restrict__ profile)
{
    extern __shared__ int diff[];
    __shared__ int wave_tot[PROF_WAVES];
    __shared__ int unit_ca[PACX_SUB];
    const BandProfileWg P = band_profile_wg(T, t_lo, t_hi, n_tiles);

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
    for (long long cf = blockIdx.x; cf < n_cf; cf += gridDim.x)
        band_profile_frame(T, P, cf, t_lo, t_hi, n_tiles, nmr, cap, cap_alloc, diff, wave_tot, unit_ca, bytes, fbits);
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        const int g = P.base + 64 * t;
        if (t < n_tiles && g < P.G && bytes[t])
            atomicAdd(&profile[g], (unsigned long long)bytes[t]);
    }
}

__global__ void k_profile_solve(const unsigned long long *__restrict__ profile, long long limit, int t_lo, int t_hi,
                                int halvings, pacx_rate_result *result)
{
    int met;
    const int t = profile_decide(profile, limit, t_lo, t_hi, halvings, met);
    result->t = t;
    result->met = met;
    result->total = (int64_t)profile[t - t_lo];
}

}  // namespace

void pacx_k::pacx_launch_band_profile(const PacxTables &T, long long n_cf, int t_lo, int t_hi, const double *nmr,
                                      const int32_t *cap, const int32_t *cap_alloc, int64_t *profile, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const int G = t_hi - t_lo + 1, n_tiles = (G + PROF_THREADS - 1) / PROF_THREADS;
    const unsigned grid = (unsigned)(n_cf < PROF_GROUPS ? n_cf : PROF_GROUPS);
    hipLaunchKernelGGL(k_band_profile, dim3(grid), dim3(PROF_THREADS), (size_t)n_tiles * PROF_THREADS * sizeof(int), st, T,
                       n_cf, t_lo, t_hi, n_tiles, nmr, cap, cap_alloc, (unsigned long long *)profile);
}

void pacx_k::pacx_launch_profile_solve(const int64_t *profile, long long limit, int t_lo, int t_hi,
                                       pacx_rate_result *result, hipStream_t st)
{
    hipLaunchKernelGGL(k_profile_solve, dim3(1), dim3(1), 0, st, (const unsigned long long *)profile, limit, t_lo, t_hi,
                       pacx_rate_solve_pairs(t_lo, t_hi) - 2, result);
}
