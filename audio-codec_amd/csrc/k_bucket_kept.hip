/*
 * k_bucket_kept.hip -- the buffered solve for a stream in chunks, on curves kept as thresholds
 * (include/pacx_bucket_kept.h): a chunk's bytes at every target of a pass, the scans of those targets carried from
 * chunk to chunk, and the tree of the bisection's next decisions.
 *
 *   k_band_bytes_kept      band_frame (pick_dev.h) without its outputs, once per target, on BandCurveRegs: one wave per
 *                          channel-frame, a lane per (unit, band) slot, the slot's sixteen indices loaded ONCE (two
 *                          16-byte loads per slot) and tested against every target from registers.
 *   k_rate_bytes_kept      solve_frame (pick_dev.h, final = 0) per channel-frame and target: one wave per channel-frame,
 *                          a lane per target.  Neighbouring targets walk mostly the same look-ups, so the wave stages
 *                          the frame's row of indices in LDS once (2 bytes an entry) and every look-up reads it there;
 *                          a row too long for LDS is read where it lies.
 *   k_bucket_scan_targets  a workgroup per target: bucket_block (bucket_dev.h) over the target's row from the level
 *                          the stream so far ended at, folded into the target's result by thread 0.
 *   k_bucket_tree_begin, k_bucket_tree_step
 *                          one thread: solve_decide (rate_dev.h) walked down the heap of a pass's targets, and the next
 *                          pass's targets, each found by walking solve_decide from the state along the slot's path.
 *
 * Trip counts come from arguments, tables and constants; integer arithmetic, no atomics on results, no scratch.
 */
#include <hip/hip_runtime.h>

#include "bucket_dev.h"
#include "grid_dev.h"
#include "pick_dev.h"
#include "rate_dev.h"   /* SolveState, solve_decide */

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int BYTES_THREADS = 256;
constexpr int BYTES_WAVES = BYTES_THREADS / 64;    /* channel-frames per workgroup of the band kernel, one per wave */
constexpr int BAND_SLOTS = PACX_SUB * PACX_MAX_BANDS / 64;         /* band slots of a row per lane, band_frame's SLOTS */
constexpr int RATE_LDS_ROW = 16384;                /* entries of a row staged in LDS at most: 32 KB */
constexpr int TREE_TARGETS = PACX_BUCKET_TREE_TARGETS;

/* a frame's kept band curve in registers: lane l holds the indices of the slots l + 64 q, as band_frame asks for them */
struct BandCurveRegs {
    unsigned w[BAND_SLOTS][BAND_CAND / 2];         /* indices 2 j, 2 j + 1 of slot lane + 64 q in the halves of w[q][j] */
    long long row;                                 /* cf * band_stride: band slot `at` of lowest() is slot at - row */
    const uint8_t *__restrict__ cap_alloc;
    int g;
    __device__ __forceinline__ int lowest(long long at, int n_cand) const
    {
        const int q = (int)(at - row) >> 6;        /* a constant of band_frame's unrolled loop: nothing is indexed */
        int pick = BAND_CAND;                      /* the lowest passing i of all 16: at or above n_cand, none below */
#pragma unroll
        for (int j = BAND_CAND / 2 - 1; j >= 0; --j) {
            unsigned v = w[0][j];
#pragma unroll
            for (int k = 1; k < BAND_SLOTS; ++k)
                v = q == k ? w[k][j] : v;
            if ((int)(v >> 16) <= g)
                pick = 2 * j + 1;
            if ((int)(v & 0xffffu) <= g)
                pick = 2 * j;
        }
        return pick < n_cand ? pick : -1;
    }
    __device__ __forceinline__ int cap_alloc_of(long long at) const { return cap_alloc[at]; }
};

/* what a frame adds to the body (band_frame's, solve_frame's return) -> its n_bytes */
__device__ __forceinline__ int frame_n_bytes(unsigned long long body) { return body ? (int)(body - 4ull) : 0; }

__global__ __launch_bounds__(BYTES_THREADS) void k_band_bytes_kept(PacxTables T, long long n_cf, int n_targets,
                                                                  const int32_t *__restrict__ target_t, int t_lo, int t_hi,
                                                                  const uint16_t *__restrict__ e,
                                                                  const int32_t *__restrict__ cap,
                                                                  const uint8_t *__restrict__ cap_alloc,
                                                                  int32_t *__restrict__ n_bytes_t)
{
    __shared__ int unit_sum[BYTES_WAVES][PACX_SUB], unit_miss[BYTES_WAVES][PACX_SUB];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long cf = (long long)blockIdx.x * BYTES_WAVES + w;
    if (cf >= n_cf)                                /* wave-uniform */
        return;
    BandCurveRegs curve;
    curve.row = cf * T.band_stride;
    curve.cap_alloc = cap_alloc;
    curve.g = 0;
#pragma unroll
    for (int q = 0; q < BAND_SLOTS; ++q) {
        const int slot = lane + 64 * q;
        uint4 lo = {0u, 0u, 0u, 0u}, hi = lo;
        if (slot < T.band_stride) {                /* every slot of the row is written in a kept curve */
            static_assert(BAND_CAND == 16, "a band's indices are two 16-byte loads");
            const uint4 *__restrict__ r = (const uint4 *)(e + (curve.row + slot) * BAND_CAND);
            lo = r[0];
            hi = r[1];
        }
        curve.w[q][0] = lo.x, curve.w[q][1] = lo.y, curve.w[q][2] = lo.z, curve.w[q][3] = lo.w;
        curve.w[q][4] = hi.x, curve.w[q][5] = hi.y, curve.w[q][6] = hi.z, curve.w[q][7] = hi.w;
    }
#pragma unroll 1
    for (int m = 0; m < n_targets; ++m) {
        curve.g = grid_clamp(target_t[m], t_lo, t_hi);
        const unsigned long long body = band_frame(T, cf, curve, cap, false, nullptr, nullptr, nullptr, unit_sum[w],
                                                   unit_miss[w]);
        if (lane == 0)
            n_bytes_t[(long long)m * n_cf + cf] = frame_n_bytes(body);
    }
}

/* one wave per channel-frame, lane m the frame at target m; staged: the row's indices go through LDS */
__global__ __launch_bounds__(64) void k_rate_bytes_kept(long long n_cf, int n_targets,
                                                        const int32_t *__restrict__ target_t, int t_lo, int t_hi, int row,
                                                        int sub_stride, int staged, const uint16_t *__restrict__ e,
                                                        const int32_t *__restrict__ bits,
                                                        const int32_t *__restrict__ steps, int32_t *__restrict__ n_bytes_t)
{
    extern __shared__ uint16_t row_e[];            /* staged: [row] */
    const long long cf = blockIdx.x;
    if (cf >= n_cf)
        return;
    const int lane = threadIdx.x;
    const long long at = cf * (long long)row;
    if (staged) {
        for (int j = lane; j < row; j += 64)
            row_e[j] = e[at + j];
        wave_lds_fence();
    }
    if (lane >= n_targets)
        return;
    const int g = grid_clamp(target_t[lane], t_lo, t_hi);
    unsigned long long body;
    if (staged)
        body = solve_frame(cf, row, sub_stride, [&](long long i) { return (int)row_e[i - at] <= g; }, bits, steps, 0,
                           nullptr, nullptr, nullptr);
    else
        body = solve_frame(cf, row, sub_stride, [&](long long i) { return (int)e[i] <= g; }, bits, steps, 0, nullptr,
                           nullptr, nullptr);
    n_bytes_t[(long long)lane * n_cf + cf] = frame_n_bytes(body);
}

/* acc is read by every thread before the scan and written by thread 0 behind the scan's barriers */
__global__ __launch_bounds__(BUCKET_THREADS) void k_bucket_scan_targets(long long n_hops, int n_ch,
                                                                       const int32_t *__restrict__ n_bytes_t,
                                                                       long long row_stride, long long drain_q16,
                                                                       long long size_bytes, long long hop_off,
                                                                       pacx_bucket_result *acc)
{
    __shared__ BucketLds lds;
    const int m = blockIdx.x;
    const long long start = acc[m].end_q16;
    const pacx_bucket_result r = bucket_block<false>(n_hops, n_ch, n_bytes_t + m * row_stride, drain_q16, size_bytes,
                                                     start, lds, EachNothing{});
    if (threadIdx.x != 0)
        return;
    pacx_bucket_result a = acc[m];
    a.total += r.total;
    if (r.peak_hop >= 0 && r.peak_q16 > a.peak_q16) {              /* of equal peaks the earlier hop stands */
        a.peak_q16 = r.peak_q16;
        a.peak_hop = r.peak_hop + hop_off;
    }
    if (a.first_over < 0 && r.first_over >= 0)
        a.first_over = r.first_over + hop_off;
    a.end_q16 = r.end_q16;
    acc[m] = a;
}

/* the state of a solve in the caller's memory: the plain solve's words and the scan at the target that stands */
struct TreeState {
    SolveState s;
    pacx_bucket_result kept;
};
static_assert(sizeof(TreeState) <= PACX_BUCKET_TREE_STATE_BYTES, "the state block of include/pacx_bucket_kept.h");

/* the targets of the next pass, in heap order, and every acc the scan of no hop.  Slot k is reached from slot 0 by
   the decisions that the bits of k + 1 below its highest spell, the first decision first (the child of k is
   2k + 1 + fits, so k + 1 doubles and takes fits); a slot below the solve's end keeps the target found */
__device__ __forceinline__ void tree_next_pass(const SolveState s, int levels, long long start_q16, int32_t *target_t,
                                               pacx_bucket_result *acc)
{
    const int n = (1 << levels) - 1;
    for (int k = 0; k < TREE_TARGETS; ++k) {
        SolveState c = s;
        const int q = k + 1, depth = 31 - __builtin_clz(q);
        for (int d = depth - 1; d >= 0; --d)
            solve_decide(&c, ((q >> d) & 1) != 0);
        target_t[k] = k < n ? c.mid : s.mid;
        acc[k] = pacx_bucket_result{0, start_q16, -1, -1, start_q16};
    }
}

__global__ __launch_bounds__(1) void k_bucket_tree_begin(TreeState *S, int t_lo, int t_hi, int levels, long long start_q16, int32_t *target_t,
                                    pacx_bucket_result *acc)
{
    const SolveState s = {t_lo - 1, t_hi, t_hi, 0, 0, 0, 0ull};        /* k_bucket_init's: lo, hi, mid, phase, done, met */
    S->s = s;
    S->kept = pacx_bucket_result{0, start_q16, -1, -1, start_q16};
    tree_next_pass(s, levels, start_q16, target_t, acc);
}

__global__ __launch_bounds__(1) void k_bucket_tree_step(TreeState *S, long long limit, long long size_bytes, long long start_q16, int levels,
                                   int32_t *target_t, pacx_bucket_result *acc, pacx_rate_result *result,
                                   pacx_bucket_result *bucket_result)
{
    SolveState s = S->s;
    pacx_bucket_result kept = S->kept;
    int k = 0;
    for (int d = 0; d < levels; ++d) {
        if (s.done)
            break;
        const pacx_bucket_result a = acc[k];
        const bool fits = a.total <= limit && a.peak_q16 <= (size_bytes << 16);
        const bool first = s.phase == 0;           /* the probe of t_hi: its scan is the answer's if it fails */
        solve_decide(&s, fits);
        if (fits || first)                         /* hi moved to this probe */
            kept = a;
        k = 2 * k + 1 + (fits ? 1 : 0);
    }
    S->s = s;
    S->kept = kept;
    tree_next_pass(s, levels, start_q16, target_t, acc);
    result->t = s.mid;
    result->met = s.met;
    result->total = kept.total;
    *bucket_result = kept;
}

}  // namespace

void pacx_k::pacx_launch_band_bytes_thresholds(const PacxTables &T, long long n_cf, int n_targets, const int32_t *target_t,
                                               int t_lo, int t_hi, const uint16_t *e, const int32_t *cap,
                                               const uint8_t *cap_alloc, int32_t *n_bytes_t, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const unsigned grid = (unsigned)((n_cf + BYTES_WAVES - 1) / BYTES_WAVES);
    hipLaunchKernelGGL(k_band_bytes_kept, dim3(grid), dim3(BYTES_THREADS), 0, st, T, n_cf, n_targets, target_t, t_lo, t_hi,
                       e, cap, cap_alloc, n_bytes_t);
}

void pacx_k::pacx_launch_rate_bytes_thresholds(long long n_cf, int row, int sub_stride, int n_targets,
                                               const int32_t *target_t, int t_lo, int t_hi, const uint16_t *e,
                                               const int32_t *bits, const int32_t *steps, int32_t *n_bytes_t,
                                               hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const int staged = row <= RATE_LDS_ROW;
    hipLaunchKernelGGL(k_rate_bytes_kept, dim3((unsigned)n_cf), dim3(64), staged ? (size_t)row * sizeof(uint16_t) : 0, st,
                       n_cf, n_targets, target_t, t_lo, t_hi, row, sub_stride, staged, e, bits, steps, n_bytes_t);
}

void pacx_k::pacx_launch_bucket_scan_targets(long long n_hops, int n_ch, int n_targets, const int32_t *n_bytes_t,
                                             long long row_stride, long long drain_q16, long long size_bytes,
                                             long long hop_off, pacx_bucket_result *acc, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_scan_targets, dim3((unsigned)n_targets), dim3(BUCKET_THREADS), 0, st, n_hops, n_ch,
                       n_bytes_t, row_stride, drain_q16, size_bytes, hop_off, acc);
}

void pacx_k::pacx_launch_bucket_tree_begin(void *state, int t_lo, int t_hi, int levels, long long start_q16,
                                           int32_t *target_t, pacx_bucket_result *acc, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_tree_begin, dim3(1), dim3(1), 0, st, (TreeState *)state, t_lo, t_hi, levels, start_q16,
                       target_t, acc);
}

void pacx_k::pacx_launch_bucket_tree_step(void *state, long long limit, long long size_bytes, long long start_q16,
                                          int levels, int32_t *target_t, pacx_bucket_result *acc, pacx_rate_result *result,
                                          pacx_bucket_result *bucket_result, hipStream_t st)
{
    hipLaunchKernelGGL(k_bucket_tree_step, dim3(1), dim3(1), 0, st, (TreeState *)state, limit, size_bytes, start_q16,
                       levels, target_t, acc, result, bucket_result);
}
