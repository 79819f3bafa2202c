/*
 * grid_dev.h -- what the kernels that work on the target grid share: k_profile.hip, k_seg_profile.hip,
 * k_rate_profile.hip (a curve's size at every target of a range) and k_kept.hip (a curve kept as grid indices), with
 * the few words k_band.hip and k_rate.hip take from here.  Targets are multiples of 1 / PACX_RATE_TARGET_GRID dB,
 * t = 64 T, and a range [t_lo, t_hi] has G = t_hi - t_lo + 1 <= PACX_PROFILE_MAX of them.  Stated once here:
 *
 *   grid_threshold      the grid index from which a curve entry passes: THE rule that turns a double into an integer
 *   frame_target, grid_clamp
 *                       the target of a frame (its uniform segment's, or the one given by value) and its grid index
 *   cand_bits, floor_half, wave_scan
 *   narrow_half         one step of a solve's bisection: the smallest fitting target, mid = hi at the end
 *   PROF_*              the shape of a profile workgroup: 16 waves, the entries a thread owns
 *   band_profile_frame  what one channel-frame of a band curve adds at every entry of the grid
 *   RunWalk, flush_row  a workgroup's contiguous run of frames, segment by segment, and its bytes into a row
 *   profile_decide      the solve's decision on a profile row
 * Integer arithmetic after the one comparison in double; every trip count is an argument's, a table's or a constant.
 */
#ifndef PACX_GRID_DEV_H
#define PACX_GRID_DEV_H

#include <math.h>

#include "pacx_launch.h"

constexpr int PROF_THREADS = 1024, PROF_WAVES = PROF_THREADS / 64;
constexpr int PROF_TILES = (PACX_PROFILE_MAX + PROF_THREADS - 1) / PROF_THREADS;      /* entries a thread owns, at most */
constexpr int PROF_GROUPS = 512;                   /* workgroups of a profile launch at most: two per CU */

static_assert(PACX_SUB * PACX_MAX_BANDS <= PROF_THREADS, "a thread per band slot");
static_assert(PACX_PROFILE_MAX < 65536, "grid indices are kept in 16 bits");

/* mantissa bits of candidate i of a band curve */
__device__ __forceinline__ int cand_bits(int i) { return i ? i + 1 : 0; }

__device__ __forceinline__ int floor_half(int a)   /* floor(a / 2), a of either sign */
{
    return (a - (a < 0 ? 1 : 0)) / 2;
}

/* One narrowing of the search for the smallest target that fits, in (lo, hi] with hi known to fit: the pick at mid
   gave `fits`.  -> false: mid is the next target to try; true: the search has ended and mid = hi is its answer.  (The
   probe of t_hi that opens a search comes here with fits and mid == hi, which leaves the interval as it is.) */
__device__ __forceinline__ bool narrow_half(int &lo, int &hi, int &mid, bool fits)
{
    if (fits)
        hi = mid;
    else
        lo = mid;
    if (hi - lo > 1) {
        mid = floor_half(lo + hi);
        return false;
    }
    mid = hi;
    return true;
}

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

/* the grid index from which the curve entry v passes, G = t_hi - t_lo + 1: never.  v <= t / 64 is 64 v <= t, both
   scalings exact; decided in double: NaN, +inf and anything above the range fail the comparison and never pass; what
   reaches the cast is cut to [t_lo, t_hi] first (fmax and fmin give the bound for a NaN), so -inf and anything at or
   below the range pass from index 0 on and no value the cast is undefined for gets there.  No branch: the band
   profile runs this sixteen times per band slot and frame */
__device__ __forceinline__ unsigned grid_threshold(double v, int t_lo, int t_hi)
{
    const double x = v * (double)PACX_RATE_TARGET_GRID;
    const double in = fmin(fmax(x, (double)t_lo), (double)t_hi);
    const unsigned e = (unsigned)((int)ceil(in) - t_lo);
    return x <= (double)t_hi ? e : (unsigned)(t_hi - t_lo + 1);
}

/* the grid target of frame cf: of its uniform segment (first_off + cf) / seg_cf, or, without an array, the one given
   by value for all frames */
__device__ __forceinline__ int frame_target(const int32_t *__restrict__ target_t, int t_all, long long cf,
                                            long long seg_cf, long long first_off)
{
    return target_t ? target_t[(first_off + cf) / seg_cf] : t_all;
}

/* a grid target as an index of the range; one outside the range is clamped into it */
__device__ __forceinline__ int grid_clamp(int t, int t_lo, int t_hi)
{
    return (t < t_lo ? t_lo : (t > t_hi ? t_hi : t)) - t_lo;
}

/* what the frames of a band profile share, worked out once per workgroup.  The entries of thread (w, lane) are
   base + 64 t, t < n_tiles, base = w * 64 n_tiles + lane: beyond G they stay zero and are never written out */
struct BandProfileWg {
    int G, base, n_cand, miss;
    int miss_long, miss_short;                     /* what a unit takes below every step: every band missed */
};

__device__ __forceinline__ BandProfileWg band_profile_wg(const PacxTables &T, int t_lo, int t_hi, int n_tiles)
{
    BandProfileWg P;
    P.G = t_hi - t_lo + 1;
    P.base = (threadIdx.x >> 6) * (n_tiles * 64) + (threadIdx.x & 63);
    P.n_cand = 1 << T.n_mant_size_bits;
    if (P.n_cand > PACX_BAND_CAND)
        P.n_cand = PACX_BAND_CAND;
    P.miss = cand_bits(P.n_cand - 1);
    P.miss_long = 0;
    P.miss_short = 0;
    for (int b = 0; b < T.nb_long; ++b)
        P.miss_long += P.miss * T.band_lines_long[b];
    for (int b = 0; b < T.nb_short; ++b)
        P.miss_short += P.miss * T.band_lines_short[b];
    return P;
}

/* One channel-frame of a band curve at every entry of the grid, by a workgroup of PROF_THREADS, the only one.  Per
   (unit, band) the size picked is a step function of the target with at most PACX_BAND_CAND steps: size i passes from
   e_i = grid_threshold(nmr[b][i]) on, and the pick at g is the smallest i with e_i <= g.  A thread per band slot turns
   its row into the e_i; per unit the slots' threads put the steps as deltas of a_b lines_b into the difference array
   `diff` (n_tiles * PROF_THREADS int32 of LDS, entry g at diff[g], zero on entry and on return; LDS atomics), the 16
   waves scan it -- wave w owns the entries [w seg, (w + 1) seg), 64 at a time with the running sum carried, the waves'
   totals through wave_tot -- and apply the cap rule to the unit's sum at every g.  fbits: the frame's bits at the
   entries the thread owns, zero on entry and on return; bytes: the frame's bytes and their length prefix are added.
   wave_tot: PROF_WAVES, unit_ca: PACX_SUB int32 of LDS */
__device__ __forceinline__ void band_profile_frame(const PacxTables &T, const BandProfileWg &P, long long cf, int t_lo,
                                                   int t_hi, int n_tiles, const double *__restrict__ nmr,
                                                   const int32_t *__restrict__ cap,
                                                   const int32_t *__restrict__ cap_alloc, int *diff, int *wave_tot,
                                                   int *unit_ca, long long (&bytes)[PROF_TILES], int (&fbits)[PROF_TILES])
{
    constexpr int BAND_CAND = PACX_BAND_CAND;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int G = P.G, base = P.base, n_cand = P.n_cand, miss = P.miss;
    const int32_t *__restrict__ cp = cap + cf * PACX_SUB;
    int units = 0;
    for (int sb = 0; sb < PACX_SUB; ++sb)
        units += cp[sb] >= 0 ? 1 : 0;
    if (!units)                                    /* a dropped hop: no bytes.  Workgroup-uniform, as all of cp is */
        return;
    const bool is_short = cp[1] >= 0;              /* a long frame's slots 1-7 hold -1 */
    const int nb = is_short ? T.nb_short : T.nb_long;
    const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
    const long long row = cf * T.band_stride;
    if (tid < PACX_SUB)
        unit_ca[tid] = 0;                          /* sum_b cap_alloc_b lines_b of the frame's units */
    __syncthreads();                               /* also: the frame before is through with diff and wave_tot */

    /* ---- a thread per band slot: the grid index from which each size passes */
    int my_unit = -1, nl = 0;
    unsigned e2[BAND_CAND / 2];                    /* e_i of sizes 2 j, 2 j + 1 in the halves of a word: G < 2^16 */
#pragma unroll
    for (int j = 0; j < BAND_CAND / 2; ++j)
        e2[j] = (unsigned)G * 0x10001u;            /* never */
    if (tid < T.band_stride) {
        const int sb = is_short ? tid / nb : (tid < nb ? 0 : PACX_SUB);
        if (sb < PACX_SUB && cp[sb] >= 0) {
            my_unit = sb;
            nl = count[is_short ? tid - sb * nb : tid];
            atomicAdd(&unit_ca[sb], cap_alloc[row + tid] * nl);
            const double *__restrict__ r = nmr + (row + tid) * BAND_CAND;
#pragma unroll
            for (int i = 0; i < BAND_CAND; ++i) {
                if (i < n_cand) {
                    const unsigned e = grid_threshold(r[i], t_lo, t_hi);
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
        if (cap_u < 0)                             /* workgroup-uniform */
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
        int carry = is_short ? P.miss_short : P.miss_long;
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
    /* ---- the frame's bytes and their length prefix (band_frame's size rule, pick_dev.h) */
    const int head = live * (T.n_scale_bits + nb * (T.n_mant_size_bits + T.n_scale_bits)) + 4 + 7;
#pragma unroll
    for (int t = 0; t < PROF_TILES; ++t) {
        bytes[t] += (long long)(((fbits[t] + head) >> 3) + 4);
        fbits[t] = 0;
    }
}

/* A workgroup's contiguous run of frames, walked segment by segment: workgroup b takes [b run, min((b + 1) run,
   n_cf)), frame cf lies in segment (first_off + cf) / seg_cf and `out` is the row [G] of the segment the walk is in:
       for (int cf = W.cf0; cf < W.cf1; W.left = W.seg_len, W.out += G) {
           const int end = cf + W.left < W.cf1 ? cf + W.left : W.cf1;
           for (; cf < end; ++cf) ...                  the frames of one segment
           flush_row(bytes, base, n_tiles, G, W.out);   then its bytes into its row
       }
   With every 512th frame per workgroup a segment shorter than 512 frames would change at every frame and every frame
   would cost G atomics; with runs a workgroup flushes once per segment its run touches. */
struct RunWalk {
    int cf0, cf1;                                  /* the run */
    int seg_len;                                   /* frames of a segment after the first; beyond the run's length
                                                      no boundary matters */
    int left;                                      /* frames of the first segment from cf0 on */
    unsigned long long *__restrict__ out;
};

/* the run, and the segment its first frame lies in: the one division, before anything is held in registers.  What
   the loop carries is 32 bits wide (n_cf < 2^28): the frame, the run's end, the frames left in the segment */
__device__ __forceinline__ RunWalk run_walk(long long n_cf, int run, long long seg_cf, long long first_off, int G,
                                            unsigned long long *__restrict__ profile)
{
    RunWalk W;
    W.cf0 = blockIdx.x * run;
    W.cf1 = W.cf0 + run < (int)n_cf ? W.cf0 + run : (int)n_cf;
    const long long seg0 = (first_off + W.cf0) / seg_cf;
    const long long left0 = (seg0 + 1) * seg_cf - first_off - W.cf0;   /* >= 1: frames of segment seg0 from cf0 on */
    W.seg_len = seg_cf < run ? (int)seg_cf : run;
    W.left = left0 < run ? (int)left0 : run;
    W.out = profile + seg0 * G;
    return W;
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

/* the decision of include/pacx.h (pacx_rate_solve) with total(t) = row[t - t_lo] against a limit >= 0: the probe of
   t_hi, then the bisection; `halvings` bounds it whatever the data: ceil(log2(t_hi - t_lo + 2)).  (rate_dev.h's
   solve_decide takes the same decision launch by launch on a pick's total; tests hold the two together.)
   -> the target found, t_hi with met = 0 where the limit cannot be met */
__device__ __forceinline__ int profile_decide(const unsigned long long *__restrict__ row, long long limit, int t_lo,
                                              int t_hi, int halvings, int &met)
{
    met = 0;
    if (!(row[t_hi - t_lo] <= (unsigned long long)limit))
        return t_hi;
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
    return hi;
}

#endif
