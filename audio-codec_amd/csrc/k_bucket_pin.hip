/*
 * k_bucket_pin.hip -- the level THROUGH every hop of a leaky bucket (pacx_bucket_through) and the kernels of the pinned
 * solves (pacx_band_solve_bucket_pinned / pacx_rate_solve_bucket_pinned, include/pacx_bucket_pin.h): a target per hop,
 * the stream's wherever the buffer allows and a pinned one where it does not.
 *
 *   through_h = F_h + R_h,   R_h = X_h + max(0, R_h+1 - drain)   (nothing behind the last hop)
 *
 * F_h is k_bucket.hip's level before hop h; R_h is the same recursion from an empty buffer over the hops in reverse
 * order.  Both are the scan of k_bucket.hip (the maps F -> max(lo, F + s), composed with 64-lane shuffles, the waves'
 * maps through LDS, the carry in a register): pin_block is that scan with the direction as a template parameter,
 * repeated here so that k_bucket.hip stays as it is.
 *
 *   pin_block<false>   the forward scan with bucket_block's result at thread 0; F_h (and L_h) written where asked
 *   pin_block<true>    the scan over the hops n_hops - 1 ... 0 from an empty buffer; hands R_h to the caller's functor
 *   k_bucket_through   forward with F_h into `through`, a barrier, backward adding R_h: through is its own workspace
 *   k_pin_init         the state, every pin free (t_lo - 1), phase_of -1, every target t_hi
 *   k_pin_step         forward over the n_bytes the pick before it wrote, thread 0 takes k_bucket_step's decision, then
 *                      ALL threads write the next target_t[h] = max(level, pin[h])
 *   k_pin_freeze       the through-scan of the probe at q: a free hop above the buffer is pinned at the phase's level;
 *                      thread 0 ends the solve or starts the next phase; all threads write the next targets
 *   k_pin_finish       the scan of the pick at the targets returned, and the three results
 *
 * ONE workgroup of 1024 threads each.  64-bit integers throughout, no atomics, no floating point; trip counts come
 * from arguments and constants.  A solve that is finished (or a phase whose bisection is) makes the kernels behind it
 * return before they scan: the state is read by every thread before the first barrier and written by thread 0 after
 * the last.
 */
#include <hip/hip_runtime.h>

#include "grid_dev.h"   /* floor_half */
#include "pacx_dev.h"

using namespace pacx_k;

namespace {

constexpr int PIN_THREADS = 1024, PIN_WAVES = PIN_THREADS / 64;
/* above every level of the domain of include/pacx_bucket.h, as k_bucket.hip's BUCKET_TOP */
constexpr long long PIN_TOP = (1ll << 62) + (1ll << 57);
constexpr long long PIN_NONE = 0x7fffffffffffffffll;         /* no hop above the buffer yet */

struct Drain {
    long long s, lo;                               /* F -> max(lo, F + s); lo >= 0, -PIN_TOP <= s */
};

__device__ __forceinline__ long long drain_apply(Drain a, long long f)
{
    const long long g = f + a.s;
    return g > a.lo ? g : a.lo;
}

/* a, then b: k_bucket.hip's rule, two negative sums cut at -PIN_TOP before they are added */
__device__ __forceinline__ Drain drain_then(Drain a, Drain b)
{
    const long long s = (b.s < 0 && a.s < -PIN_TOP - b.s) ? -PIN_TOP : a.s + b.s;
    const long long lo = a.lo + b.s;
    return Drain{s, lo > b.lo ? lo : b.lo};
}

struct PinLds {
    Drain wave[PIN_WAVES];                         /* the map of every wave's 64 hops */
    long long red[PIN_WAVES][4];                   /* the forward scan's reduction: peak, its hop, first_over, total */
    int froze;                                     /* k_pin_freeze: a hop was pinned */
    int write, next;                               /* thread 0's decision for all: write target_t at level `next` */
};

/* the state of a pinned solve: the first PIN_STATE_BYTES of its workspace, F_h and the pins behind it */
struct PinState {
    int lo, hi, mid;                               /* the bisection of the phase in flight */
    int stage;                                     /* 0: A(t_hi) is being taken, 1: bisecting, 2: p_k found, A(q) in flight */
    int finished, met;
    int k, phases, open;                           /* the phase, the bisections run, phases ran out */
    int T;                                         /* the last p_k (t_hi until there is one) */
};
constexpr size_t PIN_STATE_BYTES = 64;
static_assert(sizeof(PinState) <= PIN_STATE_BYTES, "the state has 64 bytes in front of the arrays");

/* The scan by the whole workgroup over scan positions j = 0 ... n_hops - 1, position j being hop j (forward) or hop
   n_hops - 1 - j (REV), from `start`.  each(h, f, xq) is called for every hop with the level f before its bytes
   arrive in scan order: F_h forward, max(0, R_h+1 - drain) backward.  Forward, thread 0 returns bucket_block's result. */
template <bool REV, class Each>
__device__ __forceinline__ pacx_bucket_result pin_block(long long n_hops, int n_ch, const int32_t *__restrict__ n_bytes,
                                                        long long drain_q16, long long size_bytes, long long start_q16,
                                                        PinLds &lds, Each each)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long drain = drain_q16 < PIN_TOP ? drain_q16 : PIN_TOP;
    const long long size_q16 = size_bytes << 16;
    long long carry = start_q16;                   /* the level at the tile's first position: the same in every thread */
    long long total = 0, peak = start_q16, peak_hop = -1, over = PIN_NONE;
#pragma unroll 1
    for (long long base = 0; base < n_hops; base += PIN_THREADS) {
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
        Drain inc = has ? Drain{xq - drain, 0} : Drain{0, 0};       /* past the end: the identity */
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
        for (int v = 0; v < PIN_WAVES; ++v) {
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
                if (l > size_q16 && over == PIN_NONE)
                    over = h;
            }
        }
        carry = next;
        __syncthreads();                           /* lds.wave is written again by the next tile */
    }
    pacx_bucket_result r = {0, start_q16, -1, -1, carry};
    if (REV)
        return r;
    /* the higher peak, of equal ones the earlier hop; the first hop above the buffer; the bytes */
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
        for (int v = 1; v < PIN_WAVES; ++v) {
            const long long p2 = lds.red[v][0], h2 = lds.red[v][1], o2 = lds.red[v][2];
            total += lds.red[v][3];
            if (p2 > peak || (p2 == peak && h2 < peak_hop)) {
                peak = p2;
                peak_hop = h2;
            }
            over = o2 < over ? o2 : over;
        }
        r = pacx_bucket_result{total, peak, peak_hop, over == PIN_NONE ? -1 : over, carry};
    }
    return r;
}

struct EachNothing {
    __device__ __forceinline__ void operator()(long long, long long, long long) const {}
};

/* forward: F_h into before[h], L_h into level[h] where asked */
struct EachLevels {
    long long *before, *level;
    __device__ __forceinline__ void operator()(long long h, long long f, long long xq) const
    {
        before[h] = f;
        if (level)
            level[h] = f + xq;
    }
};

/* backward: through_h = F_h + R_h over the F_h the forward pass left in io[h].  F_h and R_h hold the bytes of disjoint
   hops, so the sum stays below PIN_TOP */
struct EachThrough {
    long long *io;
    __device__ __forceinline__ void operator()(long long h, long long f, long long xq) const { io[h] += f + xq; }
};

/* `through` is not __restrict__: the backward pass reads what other threads of the workgroup wrote before the barrier */
__global__ __launch_bounds__(PIN_THREADS) void k_bucket_through(long long n_hops, int n_ch,
                                                               const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                               long long *level, long long *through,
                                                               pacx_bucket_result *__restrict__ result)
{
    __shared__ PinLds lds;
    const pacx_bucket_result r = pin_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds,
                                                  EachLevels{through, level});
    if (threadIdx.x == 0)
        *result = r;
    __syncthreads();                               /* every F_h is in `through` for the whole workgroup */
    pin_block<true>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, 0, lds, EachThrough{through});
}

/* all threads: target_t[h] = max(level, pin[h]) */
__device__ __forceinline__ void pin_targets(long long n_hops, int level, const int32_t *pin, int32_t *target_t)
{
#pragma unroll 1
    for (long long h = threadIdx.x; h < n_hops; h += PIN_THREADS) {
        const int p = pin[h];
        target_t[h] = p > level ? p : level;
    }
}

__global__ __launch_bounds__(PIN_THREADS) void k_pin_init(PinState *s, long long n_hops, int t_lo, int t_hi, int32_t *pin,
                                                         int32_t *phase_of, int32_t *target_t)
{
    if (threadIdx.x == 0)
        *s = PinState{t_lo - 1, t_hi, t_hi, 0, 0, 0, 0, 0, 0, t_hi};
#pragma unroll 1
    for (long long h = threadIdx.x; h < n_hops; h += PIN_THREADS) {
        pin[h] = t_lo - 1;
        phase_of[h] = -1;
        target_t[h] = t_hi;
    }
}

/* the scan of the pick before it and the bisection's decision, k_bucket_step's on fits(A(mid)); when the phase's level
   p_k is found, the targets of the probe at q = max(t_lo, p_k - step) -- or, with p_k = t_lo, the end of the solve */
__global__ __launch_bounds__(PIN_THREADS) void k_pin_step(PinState *s, long long n_hops, int n_ch,
                                                         const int32_t *__restrict__ n_bytes, long long limit,
                                                         pacx_bucket b, int t_lo, int step, const int32_t *pin,
                                                         int32_t *target_t)
{
    __shared__ PinLds lds;
    if (s->finished || s->stage == 2)              /* the same word for every thread: thread 0 writes behind the barriers */
        return;
    const pacx_bucket_result r = pin_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds,
                                                  EachNothing{});
    if (threadIdx.x == 0) {
        const bool fits = r.total <= limit && r.peak_q16 <= (b.size_bytes << 16);
        int write = 0, next = 0;
        bool search = true;
        if (s->stage == 0) {
            if (!fits) {                           /* unreachable: every target stays t_hi, met = 0 */
                s->finished = 1;
                search = false;
            } else {
                s->met = 1;
                s->stage = 1;
                s->phases = 1;
            }
        } else if (fits) {
            s->hi = s->mid;
        } else {
            s->lo = s->mid;
        }
        if (search) {
            write = 1;
            if (s->hi - s->lo > 1) {
                s->mid = floor_half(s->lo + s->hi);
                next = s->mid;
            } else {
                const int p = s->hi;
                s->mid = p;
                s->T = p;
                if (p == t_lo) {
                    s->finished = 1;
                    next = p;
                } else {
                    const long long q = (long long)p - step;
                    s->stage = 2;
                    next = q > t_lo ? (int)q : t_lo;
                }
            }
        }
        lds.write = write;
        lds.next = next;
    }
    __syncthreads();
    if (lds.write)
        pin_targets(n_hops, lds.next, pin, target_t);
}

/* backward over the probe at q: a FREE hop (pin below t_lo) with through_h above the buffer is pinned at p_k */
struct EachFreeze {
    const long long *before;
    int32_t *pin, *phase_of;
    long long size_q16;
    int t_lo, p, k;
    int *froze;
    __device__ __forceinline__ void operator()(long long h, long long f, long long xq) const
    {
        if (pin[h] < t_lo && before[h] + f + xq > size_q16) {
            pin[h] = p;
            phase_of[h] = k;
            *froze = 1;                            /* the same word from every thread that writes it */
        }
    }
};

__global__ __launch_bounds__(PIN_THREADS) void k_pin_freeze(PinState *s, long long n_hops, int n_ch,
                                                           const int32_t *__restrict__ n_bytes, pacx_bucket b, int t_lo,
                                                           int max_phases, long long *before, int32_t *pin,
                                                           int32_t *phase_of, int32_t *target_t)
{
    __shared__ PinLds lds;
    if (s->finished || s->stage != 2)
        return;
    const int p = s->T, k = s->k;
    if (threadIdx.x == 0)
        lds.froze = 0;
    pin_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds, EachLevels{before, nullptr});
    __syncthreads();                               /* every F_h is in the workspace, lds.froze is 0 */
    pin_block<true>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, 0, lds,
                    EachFreeze{before, pin, phase_of, b.size_bytes << 16, t_lo, p, k, &lds.froze});
    __syncthreads();                               /* the pins and lds.froze are written */
    if (threadIdx.x == 0) {
        int next = p;
        if (!lds.froze) {                          /* the buffer binds nowhere below p_k: only the size does */
            s->finished = 1;
        } else if (k == max_phases - 1) {          /* the phases ran out while the buffer bound */
            s->open = 1;
            s->finished = 1;
        } else {                                   /* p_k > t_lo: the interval holds a target */
            s->k = k + 1;
            s->phases += 1;
            s->lo = t_lo - 1;
            s->hi = p;
            s->mid = floor_half(s->lo + s->hi);
            s->stage = 1;
            next = s->mid;
        }
        lds.next = next;
    }
    __syncthreads();
    pin_targets(n_hops, lds.next, pin, target_t);
}

__global__ __launch_bounds__(PIN_THREADS) void k_pin_finish(const PinState *s, long long n_hops, int n_ch,
                                                           const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                           pacx_rate_result *result, pacx_bucket_result *bucket_result,
                                                           pacx_pin_result *pin_result)
{
    __shared__ PinLds lds;
    const pacx_bucket_result r = pin_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds,
                                                  EachNothing{});
    if (threadIdx.x != 0)
        return;
    result->t = s->T;
    result->met = s->met;
    result->total = r.total;
    *bucket_result = r;
    pin_result->phases = s->phases;
    pin_result->open = s->open;
}

}  // namespace

void pacx_k::pacx_launch_bucket_through(long long n_hops, int n_ch, const int32_t *n_bytes, const pacx_bucket &b,
                                        int64_t *level, int64_t *through, pacx_bucket_result *result, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_through, dim3(1), dim3(PIN_THREADS), 0, st, n_hops, n_ch, n_bytes, b, (long long *)level,
                       (long long *)through, result);
}

size_t pacx_k::pacx_pin_ws_unit(void) { return sizeof(long long) + 2 * sizeof(int32_t); }   /* F_h, pin[h], and padding */

size_t pacx_k::pacx_pin_ws_head(void) { return PIN_STATE_BYTES; }

/* the workspace: the state, F_h [n_hops], pin [n_hops] */
static long long *pin_before(const pacx_k::PacxPinSolve &v) { return (long long *)((char *)v.ws + PIN_STATE_BYTES); }
static int32_t *pin_pins(const pacx_k::PacxPinSolve &v) { return (int32_t *)(pin_before(v) + v.n_cf / v.n_ch); }

void pacx_k::pacx_launch_pin_init(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_init, dim3(1), dim3(PIN_THREADS), 0, st, (PinState *)v.ws, v.n_cf / v.n_ch, v.t_lo, v.t_hi,
                       pin_pins(v), v.phase_of, v.target_t);
}

void pacx_k::pacx_launch_pin_step(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_step, dim3(1), dim3(PIN_THREADS), 0, st, (PinState *)v.ws, v.n_cf / v.n_ch, v.n_ch, v.n_bytes,
                       v.limit, v.bucket, v.t_lo, v.pin_step_t, (const int32_t *)pin_pins(v), v.target_t);
}

void pacx_k::pacx_launch_pin_freeze(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_freeze, dim3(1), dim3(PIN_THREADS), 0, st, (PinState *)v.ws, v.n_cf / v.n_ch, v.n_ch,
                       v.n_bytes, v.bucket, v.t_lo, v.max_phases, pin_before(v), pin_pins(v), v.phase_of, v.target_t);
}

void pacx_k::pacx_launch_pin_finish(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_finish, dim3(1), dim3(PIN_THREADS), 0, st, (const PinState *)v.ws, v.n_cf / v.n_ch, v.n_ch,
                       v.n_bytes, v.bucket, v.result, v.bucket_result, v.pin_result);
}
