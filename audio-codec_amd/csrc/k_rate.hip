/*
 * k_rate.hip -- coding to a target noise-to-mask ratio (pacx_encode_pack_nmr_batch / pacx_encode_pack_budget_batch,
 * include/pacx.h): the BitAlloc budget of every long block and every short sub-block is a number of its own; and to
 * an average bit rate (pacx_rate_curve_batch / pacx_rate_solve): one target for the stream, found on stored curves.
 *
 *   k_rate_search<M>   one wave per unit (M = 1024: a long block, M = 128: a short sub-block).  Reads the unit's
 *                      lines, masked threshold and SMRs once; keeps the lines, the band tables, the band maxima of
 *                      |x 2^overall| and the band means of m[k] = 10^((T[k] - 96) / 10) in LDS.  One evaluation
 *                      ok(B): BitAlloc(B) on half a wave (bitalloc_half, the encoder's own), per band the scale
 *                      factor of the stored maximum, per line mantissa -> the decoder's dequantiser ->
 *                      n[k] = 4 (x - xh)^2 into LDS, then the band sums in k_nmr's order (lanes stride over the
 *                      band, butterfly of shuffles) and max_b NMR_b <= target.  The cap budget is evaluated first,
 *                      then the bisection of include/pacx.h: at most 1 + ceil(log2(J + 1)) evaluations, J <= 512.
 *                      Writes the budget, the allocation that passed (or the cap's) and the status bits.
 *   k_bitalloc_budget  k_bitalloc with the budget of every unit read from the caller's array, two units per wave.
 *   k_rate_curve<M>    k_rate_search's units, preamble (rate_unit) and evaluation (rate_eval), every step j = 0 ... J
 *                      instead of a bisection: worst[j] = max_b NMR_b and bits[j] = what pack_body writes for the
 *                      allocation of budget 32 j (pacx_rate_curve_batch).
 *   k_solve_pick       pacx_rate_solve / pacx_rate_solve_segments: one channel-frame per thread finds its segment in
 *                      the boundaries (segment_of, rate_dev.h), picks the budget of each of its units from the curve
 *                      at the target its segment has in flight and sums the frame's bytes; one 64-bit atomicAdd per
 *                      workgroup and segment present.
 *   k_rate_pick        pacx_rate_pick / pacx_rate_pick_segments: the same pick of every frame at a target given with
 *                      the call, one per uniform segment; writes the outputs, sums nothing.  Both run solve_frame
 *                      (pick_dev.h) with ok := the stored double <= the target; k_kept.hip runs it on kept grid indices.
 *   k_solve_init, k_solve_step
 *                      one thread per segment: a SolveState each, and the bisection's decision on the segment's total.
 *                      The host enqueues a fixed number of pick / step pairs and waits for none; pairs after a
 *                      segment's answer is known do nothing for it.  The whole-stream solve is the one-segment case:
 *                      its table {0, n_cf, limit} is written by k_solve_init, not uploaded.
 *   k_peak_init, k_peak_step, k_peak_finish
 *                      pacx_rate_solve_peak / pacx_band_solve_peak: the second level of the solve.  The segments' states
 *                      hold their floors after the drive above without its last pick; one more state, the stream's,
 *                      is driven by the same solve_step on picks at max(stream target, floor of the frame's segment)
 *                      (k_solve_pick<true>, k_band_pick_seg<true>).
 * RateLds, RateUnit, rate_unit, wave_sum, SolveState and solve_decide live in rate_dev.h: k_band.hip and k_bucket.hip
 * share them.
 *
 * All arithmetic that decides an integer code goes through pacx_exact.h and is compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"
#include "wave_fft.h"   /* wave_lds_fence */
#include "quant_dev.h"
#include "rate_dev.h"   /* RateLds, RateUnit, rate_unit, wave_sum, SolveState, solve_decide */
#include "pick_dev.h"   /* solve_frame; frame_target (grid_dev.h) */

using namespace pacx_k;

namespace {

constexpr int RATE_MAX_EVAL = 12;                  /* 1 + ceil(log2(J + 1)) for J < 2048; the entry point keeps J <= 512 */

/* One evaluation, the only one: the unit coded with BitAlloc budget 32 step -> max_b NMR_b, the allocation of band l
   in `bits` (lanes with u.has) and BitAlloc's guard bits in `acap`.  ok(B) of include/pacx.h is lane 0's
   rate_eval(...) <= target: both kernels take lane 0's value.  Leaves S.v, S.ba, S.sf free for the next call. */
template <int M>
__device__ __forceinline__ double rate_eval(const PacxTables &T, RateLds<M> &S, const RateUnit &u, int step, int &bits,
                                            int &acap)
{
    constexpr int PER = M / 64;
    const int lane = threadIdx.x, half = lane >> 5, l = lane & 31;
    const int nb = u.nb;
    const double up = u.up, inv = u.inv;
    bits = 0;
    acap = 0;
    bitalloc_half(half == 0, u.has, u.sv, u.nl, (double)(32 * step), u.max_mant, S.cp[half], half, l, bits, acap,
                  T.guard != 0, nb);
    if (u.has) {
        S.ba[l] = bits;
        S.sf[l] = pacx_scale_factor(__longlong_as_double((long long)S.bmax[l]), T.n_scale_bits, bits);
    }
    wave_lds_fence();
#pragma unroll 1
    for (int j = 0; j < PER; ++j) {
        const int k = lane + 64 * j;
        const int b = S.band[k];
        const int ba = S.ba[b];
        const double xv = S.x[k];
        double d = 0.0;
        if (ba)
            d = pacx_dequantize(pacx_mantissa(xv * up, S.sf[b], T.n_scale_bits, ba), S.sf[b], T.n_scale_bits, ba);
        const double e = xv - d * inv;
        S.v[k] = (e * e) * 4.0;
    }
    wave_lds_fence();
    double worst = -INFINITY;
    for (int b = 0; b < nb; ++b) {
        double sn = 0.0;
        for (int k = lane; k < S.cnt[b]; k += 64)
            sn += S.v[S.lower[b] + k];
        sn = wave_sum(sn);
        const double r = 10.0 * log10((sn / (double)S.cnt[b] + PACX_EPS) / S.mm[b]);
        worst = r > worst ? r : worst;
    }
    wave_lds_fence();                              /* v, ba, sf free for the next evaluation */
    return worst;
}

template <int M>
__global__ __launch_bounds__(64) void k_rate_search(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                   long long n_units, double target_db, double max_bps,
                                                   const double *__restrict__ lines, const double *__restrict__ thr,
                                                   const double *__restrict__ smr, const int32_t *__restrict__ overall,
                                                   int32_t *__restrict__ budget, int32_t *__restrict__ bit_alloc,
                                                   uint32_t *__restrict__ status)
{
    constexpr bool SHORT = (M == PACX_M_SHORT);
    __shared__ RateLds<M> S;
    const int lane = threadIdx.x, half = lane >> 5, l = lane & 31;
    const long long unit = blockIdx.x;
    if (unit >= n_units)
        return;
    const long long cf = SHORT ? unit / PACX_SUB : unit;
    const int sb = SHORT ? (int)(unit % PACX_SUB) : 0;
    const long long frame = cf / n_ch;
    const unsigned fl = flags ? flags[frame] : 0u;
    if (SHORT != ((fl & 2u) != 0))
        return;                                    /* the other instance's */
    const int nb = SHORT ? T.nb_short : T.nb_long;
    const long long boff = cf * T.band_stride + sb * nb;
    const bool has = half == 0 && l < nb;          /* BitAlloc's lanes: band l on the first half wave */
    if (!SHORT && lane < PACX_SUB)
        budget[cf * PACX_SUB + lane] = 0;          /* long frames use [0], written below by lane 0 again */
    if (SHORT) {
        /* the reference drops the hop for every channel when any channel holds an all-zero short sub-block
           (coder/pacfile.py:530-533): nothing is written for it, its budgets are 0 */
        unsigned st = 0;
        for (int c = 0; c < n_ch; ++c)
            st |= status[frame * n_ch + c];
        if (st & 2u) {
            if (has)
                bit_alloc[boff + l] = 0;
            if (lane == 0)
                budget[cf * PACX_SUB + sb] = 0;
            return;
        }
    }
    const RateUnit u = rate_unit<M>(T, S, cf, sb, fl, max_bps, lines, thr, smr, overall);
    const int J = u.J;

    /* ---- the search: 32 J first, then the bisection */
    int lo = -1, hi = J, mid = J;
    int best = 0, best_cap = 0;
    bool capped = false;
    for (int it = 0; it < RATE_MAX_EVAL; ++it) {
        int bits = 0, acap = 0;
        const bool ok = __shfl(rate_eval<M>(T, S, u, mid, bits, acap) <= target_db ? 1 : 0, 0, 64) != 0;   /* wave-uniform */
        if (it == 0) {
            best = bits;
            best_cap = acap;
            if (!ok) {
                capped = true;
                break;
            }
        } else if (ok) {
            hi = mid;
            best = bits;
            best_cap = acap;
        } else {
            lo = mid;
        }
        if (hi - lo <= 1)
            break;
        mid = (lo + hi) / 2;
    }
    if (has)
        bit_alloc[boff + l] = best;
    if (lane == 0) {
        budget[cf * PACX_SUB + sb] = 32 * hi;
        const unsigned st = (capped ? 128u : 0u) | ((best_cap & 1) ? 4u : 0u) | ((best_cap & 2) ? 16u : 0u);
        if (st)
            atomicOr(&status[cf], st);             /* PACX_ST_RATE_CAP, _ALLOC_CAP, _GUARD */
    }
}

/* Every budget of a unit instead of a bisection over them: worst[j] = rate_eval(j) and bits[j] = what pack_body
   (k_quant.hip) writes for the allocation of budget 32 j, j = 0 ... J.  Row layout of include/pacx.h
   (pacx_rate_curve_batch): sub-block sb at sb * sub_stride; steps[cf][8] = J of every unit, -1 where there is none. */
template <int M>
__global__ __launch_bounds__(64) void k_rate_curve(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                  long long n_units, double max_bps, int row, int sub_stride,
                                                  const double *__restrict__ lines, const double *__restrict__ thr,
                                                  const double *__restrict__ smr, const int32_t *__restrict__ overall,
                                                  const uint32_t *__restrict__ status, double *__restrict__ worst_out,
                                                  int32_t *__restrict__ bits_out, int32_t *__restrict__ steps)
{
    constexpr bool SHORT = (M == PACX_M_SHORT);
    __shared__ RateLds<M> S;
    const int lane = threadIdx.x;
    const long long unit = blockIdx.x;
    if (unit >= n_units)
        return;
    const long long cf = SHORT ? unit / PACX_SUB : unit;
    const int sb = SHORT ? (int)(unit % PACX_SUB) : 0;
    const long long frame = cf / n_ch;
    const unsigned fl = flags ? flags[frame] : 0u;
    if (SHORT != ((fl & 2u) != 0))
        return;                                    /* the other instance's */
    if (!SHORT && lane < PACX_SUB)
        steps[cf * PACX_SUB + lane] = -1;          /* long frames use [0], written below by lane 0 again */
    if (SHORT) {
        unsigned st = 0;                           /* a hop the reference drops, as in k_rate_search */
        for (int c = 0; c < n_ch; ++c)
            st |= status[frame * n_ch + c];
        if (st & 2u) {
            if (lane == 0)
                steps[cf * PACX_SUB + sb] = -1;
            return;
        }
    }
    const RateUnit u = rate_unit<M>(T, S, cf, sb, fl, max_bps, lines, thr, smr, overall);
    const long long at = cf * (long long)row + (long long)sb * sub_stride;
    int J = u.J;
    if (sb * sub_stride + J >= row)                /* the entry point refuses such a row; never write past it */
        J = row - 1 - sb * sub_stride < -1 ? -1 : row - 1 - sb * sub_stride;
    for (int j = 0; j <= J; ++j) {
        int bits = 0, acap = 0;
        const double w = rate_eval<M>(T, S, u, j, bits, acap);
        /* pack_body: the overall scale, then per band its size, its scale factor and its mantissas */
        int n = u.has ? T.n_mant_size_bits + T.n_scale_bits + bits * u.nl : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            n += __shfl_xor(n, off, 64);
        if (lane == 0) {
            worst_out[at + j] = w;
            bits_out[at + j] = n + T.n_scale_bits;
        }
    }
    if (lane == 0)
        steps[cf * PACX_SUB + sb] = J;
}

/* k_bitalloc (k_quant.hip) with a budget per unit: budget[cf][8], long frames use [0] */
__global__ __launch_bounds__(64) void k_bitalloc_budget(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                       long long n_cf, const int32_t *__restrict__ budget,
                                                       const double *__restrict__ smr, int32_t *__restrict__ bit_alloc,
                                                       uint32_t *__restrict__ status)
{
    __shared__ double cp[2][32];
    const int lane = threadIdx.x, half = lane >> 5, l = lane & 31;
    const bool dense = !flags;                     /* without flags every frame is one long block */
    const long long unit = (long long)blockIdx.x * 2 + half;
    const long long cf = dense ? unit : unit / PACX_SUB;
    const int sb = dense ? 0 : (int)(unit % PACX_SUB);
    bool alive = cf < n_cf;
    const unsigned fl = (alive && flags) ? flags[cf / n_ch] : 0u;
    const bool is_short = (fl & 2u) != 0;
    if (!is_short && sb != 0)
        alive = false;
    const int nb = is_short ? T.nb_short : T.nb_long;
    const int32_t *__restrict__ n_lines = is_short ? T.band_lines_short : T.band_lines_long;
    const double b = alive ? (double)budget[cf * PACX_SUB + sb] : 0.0;
    int max_mant = 1 << T.n_mant_size_bits;
    if (max_mant > 16)
        max_mant = 16;
    const long long off = cf * T.band_stride + (is_short ? sb * nb : 0);
    const bool has = alive && l < nb;
    const double s = has ? smr[off + l] : 0.0;
    const int nl = has ? n_lines[l] : 0;
    int bits = 0, cap = 0;
    bitalloc_half(alive, has, s, nl, b, max_mant, cp[half], half, l, bits, cap, T.guard != 0,
                  T.nb_long > T.nb_short ? T.nb_long : T.nb_short);
    if (has)
        bit_alloc[off + l] = bits;
    if (alive && cap && l == 0)
        atomicOr(&status[cf], ((cap & 1) ? 4u : 0u) | ((cap & 2) ? 16u : 0u));   /* ALLOC_CAP, GUARD */
}

/* ---- the solve of pacx_rate_solve_segments (include/pacx.h): one target per stretch of consecutive channel-frames,
   on the stored curves, a SolveState each; pacx_rate_solve's whole stream is one such stretch ---- */
constexpr int SOLVE_THREADS = 256;

/* solve_decide (rate_dev.h) on the total the pick before it left: k_solve_step takes it for every segment.  final:
   write the result */
__device__ __forceinline__ void solve_step(SolveState *s, long long limit, int final, pacx_rate_result *result)
{
    const unsigned long long total = s->total;
    s->total = 0ull;
    if (final) {
        result->t = s->mid;
        result->met = s->met;
        result->total = (int64_t)total;
        return;
    }
    solve_decide(s, total <= (unsigned long long)limit);
}

/* one thread per segment: the state of a solve before its first pick.  one: the whole-stream solve's table, seg_first
   {0, n_cf} and its limit, written here on the stream instead of uploaded (n_seg == 1); nullptr: the table is in place */
__global__ __launch_bounds__(SOLVE_THREADS) void k_solve_init(SolveState *s, int n_seg, int t_lo, int t_hi,
                                                             long long *one, long long n_cf, long long limit)
{
    const long long i = (long long)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    if (i < n_seg)
        s[i] = SolveState{t_lo - 1, t_hi, t_hi, 0, 0, 0, 0ull};      /* lo, hi, mid, phase, done, met, total */
    if (one && i == 0) {
        one[0] = 0;
        one[1] = n_cf;
        one[2] = limit;
    }
}

/* the sum of a workgroup's frames: through the waves, then LDS; thread 0 holds it */
__device__ __forceinline__ unsigned long long solve_block_sum(unsigned long long mine, unsigned long long *part)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0)
        part[threadIdx.x >> 6] = mine;
    __syncthreads();
    unsigned long long all = 0ull;
    if (threadIdx.x == 0)
        for (int w = 0; w < SOLVE_THREADS / 64; ++w)
            all += part[w];
    return all;
}

/* one channel-frame per thread (solve_frame, pick_dev.h) with a state per segment: every frame takes the target of
   its segment's state and adds to that segment's total.  A frame whose segment is done does no look-ups before the
   last launch.
   final: the last launch, at the targets found, which also writes the outputs.  A workgroup whose frames lie in one
   segment (every workgroup of a whole-stream solve) sums them through the waves and adds once; one that straddles
   boundaries sums the runs of equal segments in LDS (the frames of a segment are consecutive) and adds once per
   segment present.
   PEAK (pacx_rate_solve_peak, stage B): the segments' states rest, their mid is the segment's floor, and the state in
   flight is the stream's, s[n_seg]: every frame takes max(stream target, its segment's floor).  Before the last
   launch a workgroup adds all its frames to the stream's total, once, whatever their segments; the last launch adds
   per segment exactly as above.  The instance without PEAK is the kernel as it was. */
template <bool PEAK>
__global__ __launch_bounds__(SOLVE_THREADS) void k_solve_pick(SolveState *__restrict__ s,
                                                             const long long *__restrict__ seg_first, int n_seg,
                                                             int search_steps, long long n_cf, int row, int sub_stride,
                                                             const double *__restrict__ worst,
                                                             const int32_t *__restrict__ bits,
                                                             const int32_t *__restrict__ steps, int final,
                                                             int32_t *__restrict__ budget, int32_t *__restrict__ n_bytes,
                                                             uint8_t *__restrict__ capped)
{
    __shared__ unsigned long long part[SOLVE_THREADS / 64];
    __shared__ unsigned long long run[SOLVE_THREADS];
    __shared__ int seg_of[SOLVE_THREADS];
    const int t = threadIdx.x;
    const long long cf = (long long)blockIdx.x * SOLVE_THREADS + t;
    int seg = -1;                                  /* past the end: no segment, nothing to add */
    unsigned long long mine = 0ull;
    if (cf < n_cf) {
        seg = segment_of(seg_first, n_seg, search_steps, cf);
        const SolveState *mystate = s + seg, *flying = PEAK ? s + n_seg : mystate;
        if (final || !flying->done) {
            int mid = flying->mid;
            if (PEAK && mystate->mid > mid)
                mid = mystate->mid;                /* the segment's floor */
            const double target = (double)mid / 64.0;
            mine = solve_frame(cf, row, sub_stride, [&](long long i) { return worst[i] <= target; }, bits, steps, final,
                               budget, n_bytes, capped);
        }
    }
    seg_of[t] = seg;
    __syncthreads();
    const long long left = n_cf - (long long)blockIdx.x * SOLVE_THREADS;          /* >= 1: frames of this workgroup */
    const int last = left < SOLVE_THREADS ? (int)left - 1 : SOLVE_THREADS - 1;
    const bool whole = PEAK && !final;             /* the stream's total takes the workgroup as it is */
    const int first_seg = whole ? n_seg : seg_of[0];
    if (whole || first_seg == seg_of[last]) {      /* workgroup-uniform: one total */
        const unsigned long long all = solve_block_sum(mine, part);
        if (t == 0 && all)
            atomicAdd(&s[first_seg].total, all);
        return;
    }
    /* segmented sum: after the step of stride off, run[t] holds the frames [t, t + 2 off) of t's own run */
    run[t] = mine;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < SOLVE_THREADS; off <<= 1) {
        const bool same = t + off < SOLVE_THREADS && seg_of[t + off] == seg;
        const unsigned long long add = same ? run[t + off] : 0ull;
        __syncthreads();
        mine += add;
        run[t] = mine;
        __syncthreads();
    }
    if (seg >= 0 && mine && (t == 0 || seg_of[t - 1] != seg))
        atomicAdd(&s[seg].total, mine);
}

/* solve_frame at a known target, outputs written (pacx_rate_pick / pacx_rate_pick_segments): one channel-frame per
   thread, no reduction, no state.  The frame lies in uniform segment (first_off + cf) / seg_cf and takes
   target_t[segment] / 64; target_t == nullptr: every frame takes t_all / 64 */
__global__ __launch_bounds__(SOLVE_THREADS) void k_rate_pick(long long n_cf, long long seg_cf, long long first_off,
                                                            const int32_t *__restrict__ target_t, int t_all, int row,
                                                            int sub_stride, const double *__restrict__ worst,
                                                            const int32_t *__restrict__ bits,
                                                            const int32_t *__restrict__ steps,
                                                            int32_t *__restrict__ budget, int32_t *__restrict__ n_bytes,
                                                            uint8_t *__restrict__ capped)
{
    const long long cf = (long long)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    if (cf >= n_cf)
        return;
    const double target = (double)frame_target(target_t, t_all, cf, seg_cf, first_off) / 64.0;
    solve_frame(cf, row, sub_stride, [&](long long i) { return worst[i] <= target; }, bits, steps, 1, budget, n_bytes,
                capped);
}

/* one thread per segment: solve_step with the segment's limit; final: result[seg] */
__global__ __launch_bounds__(SOLVE_THREADS) void k_solve_step(SolveState *s, int n_seg,
                                                             const long long *__restrict__ limit, int final,
                                                             pacx_rate_result *result)
{
    const long long i = (long long)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    if (i < n_seg)
        solve_step(s + i, limit[i], final, result + i);
}

/* ---- the second level (pacx_rate_solve_peak / pacx_band_solve_peak): the stream's state is s[n_seg] ---- */

/* one thread per segment, after stage A: the state's mid is the segment's floor u_s.  Writes it out, clears the
   segment's total and starts the stream's state */
__global__ __launch_bounds__(SOLVE_THREADS) void k_peak_init(SolveState *s, int n_seg, int t_lo, int t_hi,
                                                            int32_t *__restrict__ floor)
{
    const long long i = (long long)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    if (i < n_seg) {
        floor[i] = s[i].mid;
        s[i].total = 0ull;
    }
    if (i == 0)
        s[n_seg] = SolveState{t_lo - 1, t_hi, t_hi, 0, 0, 0, 0ull};
}

/* one thread: solve_step on the stream's total against the stream's limit; final: result_stream */
__global__ void k_peak_step(SolveState *stream, long long limit, int final, pacx_rate_result *result)
{
    solve_step(stream, limit, final, result);
}

/* one thread per segment, after the last pick: result[seg] at T_s = max(t*, u_s), met measured there against the
   segment's peak; the segments' totals summed into the stream's (integers: in any order) for k_peak_step's final */
__global__ __launch_bounds__(SOLVE_THREADS) void k_peak_finish(SolveState *s, int n_seg,
                                                              const long long *__restrict__ peak,
                                                              pacx_rate_result *__restrict__ result)
{
    __shared__ unsigned long long part[SOLVE_THREADS / 64];
    const long long i = (long long)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    const SolveState *stream = s + n_seg;
    unsigned long long total = 0ull;
    if (i < n_seg) {
        total = s[i].total;
        s[i].total = 0ull;
        result[i].t = stream->mid > s[i].mid ? stream->mid : s[i].mid;
        result[i].met = total <= (unsigned long long)peak[i] ? 1 : 0;
        result[i].total = (int64_t)total;
    }
    const unsigned long long all = solve_block_sum(total, part);
    if (threadIdx.x == 0 && all)
        atomicAdd(&s[n_seg].total, all);
}

}  // namespace

size_t pacx_k::pacx_rate_solve_ws_bytes(void) { return sizeof(SolveState); }

int pacx_k::pacx_rate_solve_pairs(int t_lo, int t_hi)
{
    /* the probe of t_hi, ceil(log2(t_hi - t_lo + 2)) halvings at most, the pick that writes the outputs */
    int n = 0;
    while ((1ll << n) < (long long)t_hi - t_lo + 2)
        ++n;
    return 2 + n;
}

/* the solve's init and step, one thread per segment, for pacx_solve_drive (pacx_launch.h) */
void pacx_k::pacx_launch_solve_init_segments(const PacxSolve &v, hipStream_t st)
{
    hipLaunchKernelGGL(k_solve_init, dim3((unsigned)((v.n_seg + SOLVE_THREADS - 1) / SOLVE_THREADS)), dim3(SOLVE_THREADS),
                       0, st, (SolveState *)v.ws, v.n_seg, v.t_lo, v.t_hi, v.one_limit ? v.seg : nullptr, v.n_cf,
                       v.one_limit ? *v.one_limit : 0ll);
}

void pacx_k::pacx_launch_solve_step_segments(const PacxSolve &v, int final, hipStream_t st)
{
    hipLaunchKernelGGL(k_solve_step, dim3((unsigned)((v.n_seg + SOLVE_THREADS - 1) / SOLVE_THREADS)), dim3(SOLVE_THREADS),
                       0, st, (SolveState *)v.ws, v.n_seg, v.seg + v.n_seg + 1, final, v.result);
}

int pacx_k::pacx_segment_search_steps(int n_seg)
{
    int n = 0;                                     /* ceil(log2(n_seg)): halvings of [0, n_seg) down to one segment */
    while ((1ll << n) < (long long)n_seg)
        ++n;
    return n;
}

void pacx_k::pacx_launch_rate_curve(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                    double max_bits_per_sample, int row, int sub_stride, const double *lines,
                                    const double *thr, const double *smr, const int32_t *overall, const uint32_t *status,
                                    double *worst, int32_t *bits, int32_t *steps, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL((k_rate_curve<PACX_M_LONG>), dim3((unsigned)n_cf), dim3(64), 0, st, T, flags, n_ch, n_cf,
                       max_bits_per_sample, row, sub_stride, lines, thr, smr, overall, status, worst, bits, steps);
    if (flags)
        hipLaunchKernelGGL((k_rate_curve<PACX_M_SHORT>), dim3((unsigned)(n_cf * PACX_SUB)), dim3(64), 0, st, T, flags,
                           n_ch, n_cf * PACX_SUB, max_bits_per_sample, row, sub_stride, lines, thr, smr, overall, status,
                           worst, bits, steps);
}

void pacx_k::pacx_launch_rate_solve_segments(const PacxSolve &v, int row, int sub_stride, const double *worst,
                                             const int32_t *bits, const int32_t *steps, int32_t *budget,
                                             int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    const unsigned grid = (unsigned)((v.n_cf + SOLVE_THREADS - 1) / SOLVE_THREADS);
    pacx_solve_drive(v, st, [&](int search, int final) {
        hipLaunchKernelGGL(k_solve_pick<false>, dim3(grid), dim3(SOLVE_THREADS), 0, st, (SolveState *)v.ws, v.seg,
                           v.n_seg, search, v.n_cf, row, sub_stride, worst, bits, steps, final, budget, n_bytes, capped);
    });
}

void pacx_k::pacx_launch_rate_pick_segments(long long n_cf, int row, int sub_stride, const double *worst,
                                            const int32_t *bits, const int32_t *steps, long long seg_cf,
                                            long long first_off, const int32_t *target_t, int t_all, int32_t *budget,
                                            int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const unsigned grid = (unsigned)((n_cf + SOLVE_THREADS - 1) / SOLVE_THREADS);
    hipLaunchKernelGGL(k_rate_pick, dim3(grid), dim3(SOLVE_THREADS), 0, st, n_cf, seg_cf, first_off, target_t, t_all, row,
                       sub_stride, worst, bits, steps, budget, n_bytes, capped);
}

/* the second level's init, step and finish for pacx_peak_drive (pacx_launch.h) */
void pacx_k::pacx_launch_peak_init(const PacxSolve &v, const PacxSolveStream &p, hipStream_t st)
{
    hipLaunchKernelGGL(k_peak_init, dim3((unsigned)((v.n_seg + SOLVE_THREADS - 1) / SOLVE_THREADS)), dim3(SOLVE_THREADS),
                       0, st, (SolveState *)v.ws, v.n_seg, v.t_lo, v.t_hi, p.floor);
}

void pacx_k::pacx_launch_peak_step(const PacxSolve &v, const PacxSolveStream &p, int final, hipStream_t st)
{
    if (final)
        hipLaunchKernelGGL(k_peak_finish, dim3((unsigned)((v.n_seg + SOLVE_THREADS - 1) / SOLVE_THREADS)),
                           dim3(SOLVE_THREADS), 0, st, (SolveState *)v.ws, v.n_seg, v.seg + v.n_seg + 1, v.result);
    hipLaunchKernelGGL(k_peak_step, dim3(1), dim3(1), 0, st, (SolveState *)v.ws + v.n_seg, p.limit, final, p.result);
}

void pacx_k::pacx_launch_rate_solve_peak(const PacxSolve &v, const PacxSolveStream &p, int row, int sub_stride,
                                         const double *worst, const int32_t *bits, const int32_t *steps,
                                         int32_t *budget, int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    const unsigned grid = (unsigned)((v.n_cf + SOLVE_THREADS - 1) / SOLVE_THREADS);
    pacx_peak_drive(v, p, st, [&](int search, int final, bool peak) {
        const auto pick = peak ? k_solve_pick<true> : k_solve_pick<false>;
        hipLaunchKernelGGL(pick, dim3(grid), dim3(SOLVE_THREADS), 0, st, (SolveState *)v.ws, v.seg, v.n_seg, search,
                           v.n_cf, row, sub_stride, worst, bits, steps, final, budget, n_bytes, capped);
    });
}

void pacx_k::pacx_launch_rate_search(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                     double target_nmr_db, double max_bits_per_sample, const double *lines,
                                     const double *thr, const double *smr, const int32_t *overall, int32_t *budget,
                                     int32_t *bit_alloc, uint32_t *status, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL((k_rate_search<PACX_M_LONG>), dim3((unsigned)n_cf), dim3(64), 0, st, T, flags, n_ch, n_cf,
                       target_nmr_db, max_bits_per_sample, lines, thr, smr, overall, budget, bit_alloc, status);
    if (flags)
        hipLaunchKernelGGL((k_rate_search<PACX_M_SHORT>), dim3((unsigned)(n_cf * PACX_SUB)), dim3(64), 0, st, T, flags,
                           n_ch, n_cf * PACX_SUB, target_nmr_db, max_bits_per_sample, lines, thr, smr, overall, budget,
                           bit_alloc, status);
}

void pacx_k::pacx_launch_bitalloc_budget(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                         const int32_t *budget, const double *smr, int32_t *bit_alloc,
                                         uint32_t *status, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const long long units = flags ? n_cf * PACX_SUB : n_cf;       /* two units per wave */
    hipLaunchKernelGGL(k_bitalloc_budget, dim3((unsigned)((units + 1) / 2)), dim3(64), 0, st, T, flags, n_ch, n_cf,
                       budget, smr, bit_alloc, status);
}
