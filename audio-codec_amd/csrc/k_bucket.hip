/*
 * k_bucket.hip -- the level of a leaky bucket over the hops of a stream (pacx_bucket_scan) and the step of the
 * buffered solves (pacx_band_solve_bucket / pacx_rate_solve_bucket, include/pacx.h), on the scan of bucket_dev.h.
 *
 *   k_bucket_scan     bucket_block forward, L_h written where asked and the result written out.
 *   k_bucket_init     the state of a buffered solve before its first pick: the plain solve's SolveState (rate_dev.h),
 *                     whose mid is the word the pick kernels read their target from.
 *   k_bucket_step     bucket_block over the n_bytes the pick before it wrote, then thread 0 takes the plain solve's
 *                     decision (rate_dev.h, solve_decide) with fits := total <= limit && peak <= size << 16.
 *
 * ONE workgroup of 1024 threads each, the scan's 768 bytes of LDS; 64-bit integers throughout, no atomics, no floating
 * point; trip counts come from arguments and constants.
 */
#include <hip/hip_runtime.h>

#include "bucket_dev.h"
#include "rate_dev.h"   /* SolveState, solve_decide */

using namespace pacx_k;

namespace {

__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_scan(long long n_hops, int n_ch,
                                                               const int32_t *__restrict__ n_bytes, pacx_bucket b,
                                                               long long *__restrict__ level,
                                                               pacx_bucket_result *__restrict__ result)
{
    __shared__ BucketLds lds;
    const pacx_bucket_result r = bucket_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds,
                                                     EachLevel{level});
    if (threadIdx.x == 0)
        *result = r;
}

__global__ void k_bucket_init(SolveState *s, int t_lo, int t_hi)
{
    *s = SolveState{t_lo - 1, t_hi, t_hi, 0, 0, 0, 0ull};            /* lo, hi, mid, phase, done, met, total */
}

/* the scan of the pick before it, then the decision of include/pacx.h (pacx_rate_solve), solve_decide, on the two
   conditions instead of total <= limit.  final: the pick ran at the target found; write both results */
__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_step(SolveState *s, long long n_hops, int n_ch,
                                                               const int32_t *__restrict__ n_bytes, long long limit,
                                                               pacx_bucket b, int final, pacx_rate_result *result,
                                                               pacx_bucket_result *bucket_result)
{
    __shared__ BucketLds lds;
    const pacx_bucket_result r = bucket_block<false>(n_hops, n_ch, n_bytes, b.drain_q16, b.size_bytes, b.start_q16, lds,
                                                     EachNothing{});
    if (threadIdx.x != 0)
        return;
    if (final) {
        result->t = s->mid;
        result->met = s->met;
        result->total = r.total;
        *bucket_result = r;
        return;
    }
    solve_decide(s, r.total <= limit && r.peak_q16 <= (b.size_bytes << 16));
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
