/*
 * k_seg_profile.hip -- the whole-grid rate profile per segment of a stream (pacx_band_profile_segments,
 * pacx_profile_solve_segments, pacx_profile_clamp_add, include/pacx.h).  A profile row per segment is additive over
 * pieces of a stream in the same way the stream's profile is (k_profile.hip), so a segmented solve and the two-level
 * peak solve of a stream of any length keep the rows of the segments a piece touches, a few words per segment and one
 * stream profile of G words.  Segments are uniform stretches given by value: frame cf of the piece lies in local
 * segment (first_off + cf) / seg_cf.
 *
 *   k_band_profile_seg   k_band_profile's work per frame under the same rules (its body is repeated here,
 *                        k_profile.hip is left as it is): a workgroup of 16 waves keeps the frame's bits
 *                        and its running bytes at the entries a thread owns in registers.  It walks a CONTIGUOUS run of
 *                        frames -- workgroup b takes [b run, (b + 1) run) -- and adds its bytes to the row of the
 *                        segment it is in whenever that segment changes and at its end, one 64-bit atomicAdd per
 *                        entry.  With every 512th frame per workgroup, as k_band_profile strides, a segment shorter
 *                        than 512 frames would change at every frame and every frame would cost G atomics; with runs
 *                        a workgroup flushes once per segment its run touches.  Integer sums; trip counts are
 *                        arguments' and tables'.
 *   k_profile_solve_seg  one wave per row: k_profile_solve's decision against the row's limit (every lane takes the
 *                        same wave-uniform path), then worst_above = max of the row from the target found on, the
 *                        lanes striding over it.  A negative limit is never met.
 *   k_profile_clamp_add  stream_profile[g] += sum over s of row_s[max(g, result[s].t - t_lo)]: a thread per entry and
 *                        CLAMP_SEGS rows per workgroup and trip, one 64-bit atomicAdd per thread.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int PROF_THREADS = 1024, PROF_WAVES = PROF_THREADS / 64;
constexpr int PROF_TILES = (PACX_PROFILE_MAX + PROF_THREADS - 1) / PROF_THREADS;      /* entries a thread owns, at most */
constexpr int PROF_GROUPS = 512;                   /* workgroups at most: two per CU */
constexpr int CLAMP_THREADS = 256, CLAMP_SEGS = 32, CLAMP_GRID_Y = 4096;

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

/* the workgroup's bytes into one row, and cleared: entry g of thread (w, lane) is base + 64 t.  The flush sits in the
   loop over the run's segments; `base` goes through an empty asm so that the entries' addresses and bounds are worked
   out here and not hoisted out of the loops, where they would stay in 18 vector registers across every frame and
   spill */
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

/* diff: n_tiles * PROF_THREADS int32 (dynamic LDS), as k_band_profile's.  Workgroup b walks the frames
   [b run, min((b + 1) run, n_cf)); profile: [n_seg][G], row (first_off + cf) / seg_cf for frame cf */
__global__ __launch_bounds__(PROF_THREADS) void k_band_profile_seg(PacxTables T, long long n_cf, int run,
                                                                  long long seg_cf, long long first_off, int t_lo,
                                                                  int t_hi, int n_tiles, const double *__restrict__ nmr,
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
    int fbits[PROF_TILES];
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        bytes[t] = 0;
        fbits[t] = 0;
        if (t < n_tiles)
            diff[base + 64 * t] = 0;
    }

    /* segment by segment of the run: the frames of one, then its bytes into its row */
#pragma unroll 1
    for (int cf = cf0; cf < cf1; left = seg_len, out += G) {
        const int end = cf + left < cf1 ? cf + left : cf1;
#pragma unroll 1
        for (; cf < end; ++cf) {
            const int32_t *__restrict__ cp = cap + (long long)cf * PACX_SUB;
            int units = 0;
            for (int sb = 0; sb < PACX_SUB; ++sb)
                units += cp[sb] >= 0 ? 1 : 0;
            if (!units)                            /* a dropped hop: no bytes.  Workgroup-uniform, as all of cp is */
                continue;
            const bool is_short = cp[1] >= 0;          /* a long frame's slots 1-7 hold -1 */
            const int nb = is_short ? T.nb_short : T.nb_long;
            const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
            const long long row = (long long)cf * T.band_stride;
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
                /* ---- the unit's steps: size i holds on [e_i, the lowest e before it), relative to every band
                   missed */
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
                int run_sum = 0;
#pragma unroll 1
                for (int t = 0; t < n_tiles; ++t) {
                    const int v = wave_scan(diff[base + 64 * t], lane);
                    diff[base + 64 * t] = run_sum + v;
                    run_sum += __shfl(v, 63, 64);
                }
                if (lane == 0)
                    wave_tot[w] = run_sum;
                __syncthreads();
                int carry = is_short ? miss_short : miss_long;
#pragma unroll
                for (int i = 0; i < PROF_WAVES; ++i)
                    carry += i < w ? wave_tot[i] : 0;
                /* ---- the cap rule at every g: a unit whose sum exceeds its cap takes cap_alloc; diff is left zeroed
                   for the next unit, whose deltas any wave may write: they wait for the barrier */
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
        flush_row(bytes, base, n_tiles, G, out);
    }
}

__device__ __forceinline__ int floor_half(int a)   /* floor(a / 2), a of either sign */
{
    return (a - (a < 0 ? 1 : 0)) / 2;
}

/* one wave per row.  The decision of k_profile_solve with total(t) = row[t - t_lo] against limit[s], taken by every
   lane alike (the loads are wave-uniform); `halvings` bounds the bisection whatever the data.  Then the largest entry
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
    if (limit >= 0 && row[t_hi - t_lo] <= (unsigned long long)limit) {
        int lo = t_lo - 1, hi = t_hi;
        met = 1;
        for (int it = 0; it < halvings; ++it) {
            if (hi - lo > 1) {
                const int mid = floor_half(lo + hi);
                if (row[mid - t_lo] <= (unsigned long long)limit)
                    hi = mid;
                else
                    lo = mid;
            }
        }
        t = hi;
    }
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
