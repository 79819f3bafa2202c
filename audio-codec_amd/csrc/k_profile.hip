/*
 * k_profile.hip -- the size of a band curve at every target of the grid in one pass (pacx_band_profile), and the
 * solve's decision on such a profile (pacx_profile_solve, include/pacx.h).  total(T) of pacx_band_pick is a sum of
 * integers over channel-frames, so profile[g] = total((t_lo + g) / 64) is additive over pieces of a stream in any
 * order: a stream too long for one batch is analysed piece by piece into G 64-bit words and solved on those.
 *
 *   k_band_profile    Per (unit, band) the size picked is a step function of the target with at most PACX_BAND_CAND
 *                     steps: size i passes from the grid index e_i = ceil(64 nmr[b][i]) - t_lo on (0 when that is
 *                     negative, never when the entry is NaN or above the range), and the pick at g is the smallest i
 *                     with e_i <= g.  A workgroup of 16 waves walks a strided share of the channel-frames.  Per frame a
 *                     thread per band slot turns its row into the e_i; per unit the slots' threads put the steps as
 *                     deltas of a_b lines_b into a difference array of G int32 in LDS (LDS atomics), the 16 waves scan
 *                     it -- wave w owns the entries [w seg, (w + 1) seg), 64 at a time with the running sum carried,
 *                     the waves' totals through LDS -- and apply the cap rule to the unit's sum at every g.  The
 *                     frame's bits and the workgroup's bytes at the entries a thread owns stay in its registers
 *                     (PROF_TILES of each); at its end the workgroup adds its bytes to the profile, one 64-bit
 *                     atomicAdd per entry.  Integer sums only; every trip count is an argument's or a table's.
 *   k_profile_solve   one thread: the decision of pacx_rate_solve with total(t) := profile[t - t_lo] (k_rate.hip's
 *                     solve_step takes it launch by launch on a pick's total; tests hold the two together).
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int PROF_THREADS = 1024, PROF_WAVES = PROF_THREADS / 64;
constexpr int PROF_TILES = (PACX_PROFILE_MAX + PROF_THREADS - 1) / PROF_THREADS;      /* entries a thread owns, at most */
constexpr int PROF_GROUPS = 512;                   /* workgroups at most: two per CU; each takes every 512th frame */

static_assert(PACX_SUB * PACX_MAX_BANDS <= PROF_THREADS, "a thread per band slot");
static_assert(PACX_PROFILE_MAX < 65536, "grid indices are kept in 16 bits");

__device__ __forceinline__ int cand_bits(int i) { return i ? i + 1 : 0; }

/* inclusive sum over the wave's lanes 0 ... lane */
__device__ __forceinline__ int wave_scan(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off)
            v += o;
    }
    return v;
}

/* diff: n_tiles * PROF_THREADS int32 (dynamic LDS), entry g at diff[g]; the entries of thread (w, lane) are
   w * 64 n_tiles + 64 t + lane, t < n_tiles -- beyond G they stay zero and are never written out */
__global__ __launch_bounds__(PROF_THREADS) void k_band_profile(PacxTables T, long long n_cf, int t_lo, int t_hi, int n_tiles,
                                                              const double *__restrict__ nmr,
                                                              const int32_t *__restrict__ cap,
                                                              const int32_t *__restrict__ cap_alloc,
                                                              unsigned long long *__restrict__ profile)
{
    extern __shared__ int diff[];
    __shared__ int wave_tot[PROF_WAVES];
    __shared__ int unit_ca[PACX_SUB];              /* sum_b cap_alloc_b lines_b of the frame's units */
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int G = t_hi - t_lo + 1;
    const int base = w * (n_tiles * 64) + lane;
    int n_cand = 1 << T.n_mant_size_bits;
    if (n_cand > BAND_CAND)
        n_cand = BAND_CAND;
    const int miss = cand_bits(n_cand - 1);
    /* what a unit takes below every step: every band missed */
    int miss_long = 0, miss_short = 0;
    for (int b = 0; b < T.nb_long; ++b)
        miss_long += miss * T.band_lines_long[b];
    for (int b = 0; b < T.nb_short; ++b)
        miss_short += miss * T.band_lines_short[b];

    long long bytes[PROF_TILES];
    int fbits[PROF_TILES];
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        bytes[t] = 0;
        fbits[t] = 0;
        if (t < n_tiles)
            diff[base + 64 * t] = 0;
    }

#pragma unroll 1
    for (long long cf = blockIdx.x; cf < n_cf; cf += gridDim.x) {
        const int32_t *__restrict__ cp = cap + cf * PACX_SUB;
        int units = 0;
        for (int sb = 0; sb < PACX_SUB; ++sb)
            units += cp[sb] >= 0 ? 1 : 0;
        if (!units)                                /* a dropped hop: no bytes.  Workgroup-uniform, as all of cp is */
            continue;
        const bool is_short = cp[1] >= 0;          /* a long frame's slots 1-7 hold -1 */
        const int nb = is_short ? T.nb_short : T.nb_long;
        const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
        const long long row = cf * T.band_stride;
        if (tid < PACX_SUB)
            unit_ca[tid] = 0;
        __syncthreads();                           /* also: the frame before is through with diff and wave_tot */

        /* ---- a thread per band slot: the grid index from which each size passes */
        int my_unit = -1, nl = 0;
        unsigned e2[BAND_CAND / 2];                /* e_i of sizes 2 j, 2 j + 1 in the halves of a word: G < 2^16 */
#pragma unroll
        for (int j = 0; j < BAND_CAND / 2; ++j)
            e2[j] = (unsigned)G * 0x10001u;        /* never */
        if (tid < T.band_stride) {
            const int sb = is_short ? tid / nb : (tid < nb ? 0 : PACX_SUB);
            if (sb < PACX_SUB && cp[sb] >= 0) {
                my_unit = sb;
                nl = count[is_short ? tid - sb * nb : tid];
                atomicAdd(&unit_ca[sb], cap_alloc[row + tid] * nl);
                const double *__restrict__ r = nmr + (row + tid) * BAND_CAND;
#pragma unroll
                for (int i = 0; i < BAND_CAND; ++i) {
                    /* r <= t / 64 is 64 r <= t, both scalings exact; decided in double: NaN and +inf fail the first
                       comparison, -inf and anything below the range pass the second, and only what lies in
                       (t_lo, t_hi] reaches the cast */
                    const double x = r[i] * (double)PACX_RATE_TARGET_GRID;
                    if (i < n_cand && x <= (double)t_hi) {
                        const unsigned e = x <= (double)t_lo ? 0u : (unsigned)((int)ceil(x) - t_lo);
                        e2[i / 2] = i & 1 ? (e2[i / 2] & 0xffffu) | (e << 16) : (e2[i / 2] & 0xffff0000u) | e;
                    }
                }
            }
        }
        __syncthreads();

        int live = 0;
#pragma unroll 1
        for (int u = 0; u < PACX_SUB; ++u) {
            const int cap_u = cp[u];
            if (cap_u < 0)                         /* workgroup-uniform */
                continue;
            ++live;
            /* ---- the unit's steps: size i holds on [e_i, the lowest e before it), relative to every band missed */
            if (my_unit == u) {
                int hi = G;
#pragma unroll
                for (int i = 0; i < BAND_CAND; ++i) {
                    const int e = (int)(i & 1 ? e2[i / 2] >> 16 : e2[i / 2] & 0xffffu);
                    if (e < hi) {
                        const int d = (cand_bits(i) - miss) * nl;
                        if (d) {
                            atomicAdd(&diff[e], d);
                            if (hi < G)
                                atomicAdd(&diff[hi], -d);
                        }
                        hi = e;
                    }
                }
            }
            __syncthreads();
            const int ca_u = unit_ca[u];
            /* ---- scan, in place: the wave's own entries, 64 at a time, the running sum carried */
            int run = 0;
#pragma unroll 1
            for (int t = 0; t < n_tiles; ++t) {
                const int v = wave_scan(diff[base + 64 * t], lane);
                diff[base + 64 * t] = run + v;
                run += __shfl(v, 63, 64);
            }
            if (lane == 0)
                wave_tot[w] = run;
            __syncthreads();
            int carry = is_short ? miss_short : miss_long;
#pragma unroll
            for (int i = 0; i < PROF_WAVES; ++i)
                carry += i < w ? wave_tot[i] : 0;
            /* ---- the cap rule at every g: a unit whose sum exceeds its cap takes cap_alloc; diff is left zeroed for
               the next unit, whose deltas any wave may write: they wait for the barrier */
#pragma unroll
            for (int t = 0; t < PROF_TILES; ++t) {
                if (t < n_tiles) {
                    const int sum = diff[base + 64 * t] + carry;
                    diff[base + 64 * t] = 0;
                    fbits[t] += sum > cap_u ? ca_u : sum;
                }
            }
            __syncthreads();
        }
        /* ---- the frame's bytes and their length prefix (k_band_pick's size rule) */
        const int head = live * (T.n_scale_bits + nb * (T.n_mant_size_bits + T.n_scale_bits)) + 4 + 7;
#pragma unroll
        for (int t = 0; t < PROF_TILES; ++t) {
            bytes[t] += (long long)(((fbits[t] + head) >> 3) + 4);
            fbits[t] = 0;
        }
    }
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        const int g = base + 64 * t;
        if (t < n_tiles && g < G && bytes[t])
            atomicAdd(&profile[g], (unsigned long long)bytes[t]);
    }
}

__device__ __forceinline__ int floor_half(int a)   /* floor(a / 2), a of either sign */
{
    return (a - (a < 0 ? 1 : 0)) / 2;
}

/* the decision of include/pacx.h (pacx_rate_solve) with total(t) = profile[t - t_lo]; `halvings` bounds the
   bisection whatever the data: ceil(log2(t_hi - t_lo + 2)) */
__global__ void k_profile_solve(const unsigned long long *__restrict__ profile, long long limit, int t_lo, int t_hi,
                                int halvings, pacx_rate_result *result)
{
    int t = t_hi, met = 0;
    if (profile[t_hi - t_lo] <= (unsigned long long)limit) {
        int lo = t_lo - 1, hi = t_hi;
        met = 1;
        for (int it = 0; it < halvings; ++it) {
            if (hi - lo > 1) {
                const int mid = floor_half(lo + hi);
                if (profile[mid - t_lo] <= (unsigned long long)limit)
                    hi = mid;
                else
                    lo = mid;
            }
        }
        t = hi;
    }
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
