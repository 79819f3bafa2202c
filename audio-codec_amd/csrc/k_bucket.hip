/*
 * k_bucket.hip -- the level of a leaky bucket over the hops of a stream (pacx_bucket_scan) and the step of the
 * buffered solves (pacx_band_solve_bucket / pacx_rate_solve_bucket, include/pacx.h).  A hop adds its records and one
 * hop's drain leaves, never below empty: F -> max(lo, F + s) with (s, lo) = (X_h - drain, 0).  Such maps are closed
 * under composition, "A then B" = (sA + sB, max(loB, loA + sB)), so every level is an exclusive scan of the hops'
 * maps applied to the start level.
 *
 *   bucket_block      ONE workgroup of 1024 threads walks the hops 1024 at a time, a hop per thread: the thread sums
 *                     the hop's n_ch entries, the wave scans the maps with 64-lane shuffles, the waves' totals go
 *                     through LDS (16 maps, read by every thread as broadcasts), the level at the tile's first hop
 *                     stays in a register of every thread.  A thread keeps the peak, its first hop, the first hop
 *                     above the buffer and the bytes of the hops it saw (they ascend); one workgroup reduction at the
 *                     end leaves the result with thread 0.
 *   k_bucket_scan     bucket_block, the result written out.
 *   k_bucket_init     the state of a buffered solve before its first pick: the plain solve's SolveState (rate_dev.h),
 *                     whose mid is the word the pick kernels read their target from.
 *   k_bucket_step     bucket_block over the n_bytes the pick before it wrote, then thread 0 takes the plain solve's
 *                     decision (k_rate.hip, solve_step) with fits := total <= limit && peak <= size << 16.
 *
 * 64-bit integers throughout, no atomics, no floating point; trip counts come from arguments and constants.  Sums of s
 * are kept at or above -BUCKET_TOP, a bound no level reaches: below it the map gives lo for every level there is, so
 * cutting s there changes no result and keeps a drain of any size inside int64.
 */
#include <hip/hip_runtime.h>

#include "grid_dev.h"   /* floor_half */
#include "rate_dev.h"   /* SolveState */

using namespace pacx_k;

namespace {

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
    long long red[BUCKET_WAVES][4];                /* the last reduction: peak, its hop, first_over, total */
};

/* the scan of include/pacx.h by the whole workgroup; thread 0 returns the result, `level` (may be null) receives L_h */
__device__ __forceinline__ pacx_bucket_result bucket_block(long long n_hops, int n_ch, const int32_t *__restrict__ n_bytes,
                                                           long long drain_q16, long long size_bytes, long long start_q16,
                                                           long long *__restrict__ level, BucketLds &lds)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long drain = drain_q16 < BUCKET_TOP ? drain_q16 : BUCKET_TOP;
    const long long size_q16 = size_bytes << 16;
    long long carry = start_q16;                   /* F at the tile's first hop: the same in every thread */
    long long total = 0, peak = start_q16, peak_hop = -1, over = BUCKET_NONE;
#pragma unroll 1
    for (long long base = 0; base < n_hops; base += BUCKET_THREADS) {
        const long long h = base + t;
        const bool has = h < n_hops;
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
        const Drain before = {__shfl_up(inc.s, 1, 64), __shfl_up(inc.lo, 1, 64)};      /* the wave's hops before mine */
        if (lane == 63)
            lds.wave[w] = inc;
        __syncthreads();
        long long f = carry, next = carry;
#pragma unroll
        for (int v = 0; v < BUCKET_WAVES; ++v) {
            if (v == w)
                f = next;                          /* the level at my wave's first hop */
            next = drain_apply(lds.wave[v], next);
        }
        if (lane)
            f = drain_apply(before, f);
        if (has) {
            const long long l = f + xq;
            if (level)
                level[h] = l;
            total += x;
            if (l > peak) {
                peak = l;
                peak_hop = h;
            }
            if (l > size_q16 && over == BUCKET_NONE)
                over = h;
        }
        carry = next;
        __syncthreads();                           /* lds.wave is written again by the next tile */
    }
    /* the higher peak, of equal ones the earlier hop (-1 goes with the start level, which no hop's peak equals) */
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
    pacx_bucket_result r = {0, start_q16, -1, -1, carry};
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

__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_scan(long long n_hops, int n_ch,
                                                               const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                               long long *__restrict__ level,
                                                               pacx_bucket_result *__restrict__ result)
{
    __shared__ BucketLds lds;
    const pacx_bucket_result r = bucket_block(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, level, lds);
    if (threadIdx.x == 0)
        *result = r;
}

__global__ void k_bucket_init(SolveState *s, int t_lo, int t_hi)
{
    *s = SolveState{t_lo - 1, t_hi, t_hi, 0, 0, 0, 0ull};            /* lo, hi, mid, phase, done, met, total */
}

/* the scan of the pick before it, then the decision of include/pacx.h (pacx_rate_solve) as k_rate.hip's solve_step
   takes it, on fits instead of total <= limit.  final: the pick ran at the target found; write both results */
__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_step(SolveState *s, long long n_hops, int n_ch,
                                                               const int32_t *__restrict__ n_bytes, long long limit,
                                                               pacx_bucket b, int final, pacx_rate_result *result,
                                                               pacx_bucket_result *bucket_result)
{
    __shared__ BucketLds lds;
    const pacx_bucket_result r = bucket_block(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, nullptr, lds);
    if (threadIdx.x != 0)
        return;
    if (final) {
        result->t = s->mid;
        result->met = s->met;
        result->total = r.total;
        *bucket_result = r;
        return;
    }
    if (s->done)
        return;
    const bool fits = r.total <= limit && r.peak_q16 <= (b.size_bytes << 16);
    if (s->phase == 0) {
        if (!fits) {                               /* unreachable: the largest target, met = 0 */
            s->done = 1;
            return;                                /* mid stays t_hi */
        }
        s->met = 1;
        s->phase = 1;
    } else if (fits) {
        s->hi = s->mid;
    } else {
        s->lo = s->mid;
    }
    if (s->hi - s->lo > 1) {
        s->mid = floor_half(s->lo + s->hi);
    } else {
        s->mid = s->hi;
        s->done = 1;
    }
}

}  // namespace

void pacx_k::pacx_launch_bucket_scan(long long n_hops, int n_ch, const int32_t *n_bytes, const pacx_bucket &b,
                                     int64_t *level, pacx_bucket_result *result, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_scan, dim3(1), dim3(BUCKET_THREADS), 0, st, n_hops, n_ch, n_bytes, b, (long long *)level,
                       result);
}

size_t pacx_k::pacx_bucket_ws_bytes(void) { return sizeof(SolveState); }

const int32_t *pacx_k::pacx_bucket_target(const PacxBucketSolve &v) { return &((const SolveState *)v.ws)->mid; }

void pacx_k::pacx_launch_bucket_init(const PacxBucketSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_init, dim3(1), dim3(1), 0, st, (SolveState *)v.ws, v.t_lo, v.t_hi);
}

void pacx_k::pacx_launch_bucket_step(const PacxBucketSolve &v, int final, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_step, dim3(1), dim3(BUCKET_THREADS), 0, st, (SolveState *)v.ws, v.n_cf / v.n_ch, v.n_ch,
                       v.n_bytes, v.limit, v.bucket, final, v.result, v.bucket_result);
}
