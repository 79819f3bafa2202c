/*
 * k_bucket_pin.hip -- the level THROUGH every hop of a leaky bucket (pacx_bucket_through) and the kernels of the pinned
 * solves (pacx_band_solve_bucket_pinned / pacx_rate_solve_bucket_pinned, include/pacx_bucket_pin.h): a target per hop,
 * the stream's wherever the buffer allows and a pinned one where it does not.
 *
 *   through_h = F_h + R_h,   R_h = X_h + max(0, R_h+1 - drain)   (nothing behind the last hop)
 *
 * F_h is k_bucket.hip's level before hop h; R_h is the same recursion from an empty buffer over the hops in reverse
 * order.  Both are the scan of bucket_dev.h, bucket_block, whose direction is a template parameter: forward it hands
 * F_h to the caller's functor and leaves the result with thread 0, backward (the hops n_hops - 1 ... 0 from an empty
 * buffer) it hands over max(0, R_h+1 - drain).  Here is only what pinning adds:
 *
 *   PinState           the state of a pinned solve; PinLds: the scan's LDS and three words thread 0 tells the others
 *   EachLevels, EachThrough, EachFreeze
 *                      what the scans do at every hop: F_h (and L_h) written, through_h summed, a free hop pinned
 *   k_bucket_through   forward with F_h into `through`, a barrier, backward adding R_h: through is its own workspace
 *   k_pin_init         the state, every pin free (t_lo - 1), phase_of -1, every target t_hi
 *   k_pin_step         forward over the n_bytes the pick before it wrote, thread 0 narrows the phase's bisection on
 *                      k_bucket_step's fits (narrow_half), then ALL threads write the next target_t[h] =
 *                      max(level, pin[h])
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

#include "bucket_dev.h"
#include "grid_dev.h"   /* floor_half, narrow_half */

using namespace pacx_k;

namespace {

/* the scan's LDS, and three words beside it */
struct PinLds {
    BucketLds scan;
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

/* forward: F_h into before[h], L_h into level[h] where asked.  (Written out, not through EachLevel: the compiler
   schedules k_bucket_through's stores differently behind the nested call, and that kernel measured 1.6 % slower) */
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
   hops, so the sum stays below BUCKET_TOP */
struct EachThrough {
    long long *io;
    __device__ __forceinline__ void operator()(long long h, long long f, long long xq) const { io[h] += f + xq; }
};

/* `through` is not __restrict__: the backward pass reads what other threads of the workgroup wrote before the barrier */
__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_through(long long n_hops, int n_ch,
                                                                  const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                                  long long *level, long long *through,
                                                                  pacx_bucket_result *__restrict__ result)
{
    __shared__ PinLds lds;
    const pacx_bucket_result r = bucket_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16,
                                                     lds.scan, EachLevels{through, level});
    if (threadIdx.x == 0)
        *result = r;
    __syncthreads();                               /* every F_h is in `through` for the whole workgroup */
    bucket_block<true>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, 0, lds.scan, EachThrough{through});
}

/* all threads: target_t[h] = max(level, pin[h]) */
__device__ __forceinline__ void pin_targets(long long n_hops, int level, const int32_t *pin, int32_t *target_t)
{
#pragma unroll 1
    for (long long h = threadIdx.x; h < n_hops; h += BUCKET_THREADS) {
        const int p = pin[h];
        target_t[h] = p > level ? p : level;
    }
}

__global__ __launch_bounds__(BUCKET_THREADS) void k_pin_init(PinState *s, long long n_hops, int t_lo, int t_hi,
                                                            int32_t *pin, int32_t *phase_of, int32_t *target_t)
{
    if (threadIdx.x == 0)
        *s = PinState{t_lo - 1, t_hi, t_hi, 0, 0, 0, 0, 0, 0, t_hi};
#pragma unroll 1
    for (long long h = threadIdx.x; h < n_hops; h += BUCKET_THREADS) {
        pin[h] = t_lo - 1;
        phase_of[h] = -1;
        target_t[h] = t_hi;
    }
}

/* the scan of the pick before it and the bisection's narrowing on k_bucket_step's fits(A(mid)) (the probe of t_hi
   that opens the solve leaves the interval as it is: narrow_half, grid_dev.h); when the phase's level p_k is found,
   the targets of the probe at q = max(t_lo, p_k - step) -- or, with p_k = t_lo, the end of the solve */
__global__ __launch_bounds__(BUCKET_THREADS) void k_pin_step(PinState *s, long long n_hops, int n_ch,
                                                            const int32_t *__restrict__ n_bytes, long long limit,
                                                            pacx_bucket b, int t_lo, int step, const int32_t *pin,
                                                            int32_t *target_t)
{
    __shared__ PinLds lds;
    if (s->finished || s->stage == 2)              /* the same word for every thread: thread 0 writes behind the barriers */
        return;
    const pacx_bucket_result r = bucket_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16,
                                                     lds.scan, EachNothing{});
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
        }
        if (search) {
            write = 1;
            if (!narrow_half(s->lo, s->hi, s->mid, fits)) {
                next = s->mid;
            } else {
                const int p = s->mid;              /* the phase's level: the smallest target that fits */
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

__global__ __launch_bounds__(BUCKET_THREADS) void k_pin_freeze(PinState *s, long long n_hops, int n_ch,
                                                              const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                              int t_lo, int max_phases, long long *before, int32_t *pin,
                                                              int32_t *phase_of, int32_t *target_t)
{
    __shared__ PinLds lds;
    if (s->finished || s->stage != 2)
        return;
    const int p = s->T, k = s->k;
    if (threadIdx.x == 0)
        lds.froze = 0;
    bucket_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds.scan,
                        EachLevels{before, nullptr});
    __syncthreads();                               /* every F_h is in the workspace, lds.froze is 0 */
    bucket_block<true>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, 0, lds.scan,
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

__global__ __launch_bounds__(BUCKET_THREADS) void k_pin_finish(const PinState *s, long long n_hops, int n_ch,
                                                              const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                              pacx_rate_result *result,
                                                              pacx_bucket_result *bucket_result,
                                                              pacx_pin_result *pin_result)
{
    __shared__ PinLds lds;
    const pacx_bucket_result r = bucket_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16,
                                                     lds.scan, EachNothing{});
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
    hipLaunchKernelGGL(k_bucket_through, dim3(1), dim3(BUCKET_THREADS), 0, st, n_hops, n_ch, n_bytes, b, (long long *)level,
                       (long long *)through, result);
}

size_t pacx_k::pacx_pin_ws_unit(void) { return sizeof(long long) + 2 * sizeof(int32_t); }   /* F_h, pin[h], and padding */

size_t pacx_k::pacx_pin_ws_head(void) { return PIN_STATE_BYTES; }

/* the workspace: the state, F_h [n_hops], pin [n_hops] */
static long long *pin_before(const pacx_k::PacxPinSolve &v) { return (long long *)((char *)v.ws + PIN_STATE_BYTES); }
static int32_t *pin_pins(const pacx_k::PacxPinSolve &v) { return (int32_t *)(pin_before(v) + v.n_cf / v.n_ch); }

void pacx_k::pacx_launch_pin_init(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_init, dim3(1), dim3(BUCKET_THREADS), 0, st, (PinState *)v.ws, v.n_cf / v.n_ch, v.t_lo, v.t_hi,
                       pin_pins(v), v.phase_of, v.target_t);
}

void pacx_k::pacx_launch_pin_step(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_step, dim3(1), dim3(BUCKET_THREADS), 0, st, (PinState *)v.ws, v.n_cf / v.n_ch, v.n_ch, v.n_bytes,
                       v.limit, v.bucket, v.t_lo, v.pin_step_t, (const int32_t *)pin_pins(v), v.target_t);
}

void pacx_k::pacx_launch_pin_freeze(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_freeze, dim3(1), dim3(BUCKET_THREADS), 0, st, (PinState *)v.ws, v.n_cf / v.n_ch, v.n_ch,
                       v.n_bytes, v.bucket, v.t_lo, v.max_phases, pin_before(v), pin_pins(v), v.phase_of, v.target_t);
}

void pacx_k::pacx_launch_pin_finish(const PacxPinSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_pin_finish, dim3(1), dim3(BUCKET_THREADS), 0, st, (const PinState *)v.ws, v.n_cf / v.n_ch, v.n_ch,
                       v.n_bytes, v.bucket, v.result, v.bucket_result, v.pin_result);
}
