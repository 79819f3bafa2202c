/*
 * bucket_dev.h -- the scan of a leaky bucket over the hops of a stream, stated once for k_bucket.hip (the level at
 * every hop, the buffered solves) and k_bucket_pin.hip (the level through every hop, the pinned solves).  A hop adds
 * its records and one hop's drain leaves, never below empty: F -> max(lo, F + s) with (s, lo) = (X_h - drain, 0).  Such
 * maps are closed under composition, "A then B" = (sA + sB, max(loB, loA + sB)), so every level is an exclusive scan of
 * the hops' maps applied to the start level.
 *
 *   Drain, drain_apply, drain_then
 *                       the map, and the rule that composes two
 *   BucketLds           what the scan keeps in LDS: a map per wave, four words per wave for the last reduction
 *   bucket_block<REV>   ONE workgroup of 1024 threads walks the hops 1024 at a time, a hop per thread, forward or (REV)
 *                       from the last hop to the first: the thread sums the hop's n_ch entries, the wave scans the maps
 *                       with 64-lane shuffles, the waves' totals go through LDS (16 maps, read by every thread as
 *                       broadcasts), the level at the tile's first hop stays in a register of every thread.  Forward, a
 *                       thread keeps the peak, its first hop, the first hop above the buffer and the bytes of the hops
 *                       it saw (they ascend); one workgroup reduction at the end leaves the result with thread 0.
 *   EachNothing, EachLevel
 *                       what a caller does at every hop: nothing, or L_h written where a pointer is given
 *
 * 64-bit integers throughout, no atomics, no floating point; trip counts come from arguments and constants.  Sums of s
 * are kept at or above -BUCKET_TOP, a bound no level reaches: below it the map gives lo for every level there is, so
 * cutting s there changes no result and keeps a drain of any size inside int64.
 */
#ifndef PACX_BUCKET_DEV_H
#define PACX_BUCKET_DEV_H

#include "pacx_launch.h"

constexpr int BUCKET_THREADS = 1024, BUCKET_WAVES = BUCKET_THREADS / 64;
/* above every level of the domain of include/pacx.h: start <= 2^56, (sum of x) << 16 <= 2^46 * 65539 < 2^62 + 2^56 */
constexpr long long BUCKET_TOP = (1ll << 62) + (1ll << 57);
constexpr long long BUCKET_NONE = 0x7fffffffffffffffll;      /* no hop above the buffer yet */

struct Drain {
    long long s, lo;                               /* F -> max(lo, F + s); lo >= 0, -BUCKET_TOP <= s */
};

__device__ __forceinline__ long long drain_apply(Drain a, long long f)
{
    const long long g = f + a.s;
    return g > a.lo ? g : a.lo;
}

/* a, then b.  The positive parts of s are bytes of disjoint hops, so the sum stays below BUCKET_TOP; two negative
   ones are cut at -BUCKET_TOP before they are added */
__device__ __forceinline__ Drain drain_then(Drain a, Drain b)
{
    const long long s = (b.s < 0 && a.s < -BUCKET_TOP - b.s) ? -BUCKET_TOP : a.s + b.s;
    const long long lo = a.lo + b.s;
    return Drain{s, lo > b.lo ? lo : b.lo};
}

struct BucketLds {
    Drain wave[BUCKET_WAVES];                      /* the map of every wave's 64 hops */
    long long red[BUCKET_WAVES][4];                /* the forward scan's reduction: peak, its hop, first_over, total */
};

/* The scan of include/pacx.h by the whole workgroup over scan positions j = 0 ... n_hops - 1, position j being hop j
   (forward) or hop n_hops - 1 - j (REV), from `start`.  each(h, f, xq) is called for every hop with the level f before
   its bytes xq arrive in scan order: F_h forward, max(0, R_h+1 - drain) backward.  Forward, thread 0 returns the
   result; the level behind the last position is `end_q16` of what every thread returns. */
template <bool REV, class Each>
__device__ __forceinline__ pacx_bucket_result bucket_block(long long n_hops, int n_ch, const int32_t *__restrict__ n_bytes,
                                                           long long drain_q16, long long size_bytes, long long start_q16,
                                                           BucketLds &lds, Each each)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long drain = drain_q16 < BUCKET_TOP ? drain_q16 : BUCKET_TOP;
    const long long size_q16 = size_bytes << 16;
    long long carry = start_q16;                   /* the level at the tile's first position: the same in every thread */
    long long total = 0, peak = start_q16, peak_hop = -1, over = BUCKET_NONE;
#pragma unroll 1
    for (long long base = 0; base < n_hops; base += BUCKET_THREADS) {
        const long long j = base + t;
        const bool has = j < n_hops;
        const long long h = REV ? n_hops - 1 - j : j;
        long long x = 0;
        if (has) {
            const int32_t *p = n_bytes + h * n_ch;
#pragma unroll 1
            for (int c = 0; c < n_ch; ++c) {
                const int v = p[c];
                x += v > 0 ? v + 4 : 0;
            }
        }
        const long long xq = x << 16;
        /* past the end: the identity, behind every hop there is */
        Drain inc = has ? Drain{xq - drain, 0} : Drain{0, 0};
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const Drain o = {__shfl_up(inc.s, off, 64), __shfl_up(inc.lo, off, 64)};
            if (lane >= off)
                inc = drain_then(o, inc);
        }
        const Drain before = {__shfl_up(inc.s, 1, 64), __shfl_up(inc.lo, 1, 64)};      /* the wave's positions before mine */
        if (lane == 63)
            lds.wave[w] = inc;
        __syncthreads();
        long long f = carry, next = carry;
#pragma unroll
        for (int v = 0; v < BUCKET_WAVES; ++v) {
            if (v == w)
                f = next;                          /* the level at my wave's first position */
            next = drain_apply(lds.wave[v], next);
        }
        if (lane)
            f = drain_apply(before, f);
        if (has) {
            each(h, f, xq);
            if (!REV) {
                const long long l = f + xq;
                total += x;
                if (l > peak) {
                    peak = l;
                    peak_hop = h;
                }
                if (l > size_q16 && over == BUCKET_NONE)
                    over = h;
            }
        }
        carry = next;
        __syncthreads();                           /* lds.wave is written again by the next tile */
    }
    pacx_bucket_result r = {0, start_q16, -1, -1, carry};
    if (REV)
        return r;
    /* the higher peak, of equal ones the earlier hop (-1 goes with the start level, which no hop's peak equals); the
       first hop above the buffer; the bytes */
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long p2 = __shfl_xor(peak, off, 64), h2 = __shfl_xor(peak_hop, off, 64);
        const long long o2 = __shfl_xor(over, off, 64);
        total += __shfl_xor(total, off, 64);
        if (p2 > peak || (p2 == peak && h2 < peak_hop)) {
            peak = p2;
            peak_hop = h2;
        }
        over = o2 < over ? o2 : over;
    }
    if (lane == 0) {
        lds.red[w][0] = peak;
        lds.red[w][1] = peak_hop;
        lds.red[w][2] = over;
        lds.red[w][3] = total;
    }
    __syncthreads();
    if (t == 0) {
        peak = lds.red[0][0];
        peak_hop = lds.red[0][1];
        over = lds.red[0][2];
        total = lds.red[0][3];
        for (int v = 1; v < BUCKET_WAVES; ++v) {
            const long long p2 = lds.red[v][0], h2 = lds.red[v][1], o2 = lds.red[v][2];
            total += lds.red[v][3];
            if (p2 > peak || (p2 == peak && h2 < peak_hop)) {
                peak = p2;
                peak_hop = h2;
            }
            over = o2 < over ? o2 : over;
        }
        r = pacx_bucket_result{total, peak, peak_hop, over == BUCKET_NONE ? -1 : over, carry};
    }
    return r;
}

struct EachNothing {
    __device__ __forceinline__ void operator()(long long, long long, long long) const {}
};

/* forward: L_h into level[h] where asked */
struct EachLevel {
    long long *level;
    __device__ __forceinline__ void operator()(long long h, long long f, long long xq) const
    {
        if (level)
            level[h] = f + xq;
    }
};

#endif
