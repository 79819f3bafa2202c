/*
 * k_band.hip -- bits handed to the bands one by one against a noise-to-mask target (pacx_band_curve_batch /
 * pacx_band_pick / pacx_band_solve / pacx_encode_pack_alloc_batch, include/pacx.h).  In this coder the noise of a
 * band depends on that band's own mantissa size and on nothing else, so the smallest stream that keeps every band at
 * or below a target is found band by band on a stored curve of PACX_BAND_CAND sizes.
 *
 *   k_band_curve<M>   one wave per unit (M = 1024: a long block, M = 128: a short sub-block), k_rate_search's units and
 *                     preamble (rate_unit, rate_dev.h).  Candidate 0 (no bits) is the lines' own energy; for each of the
 *                     other sizes one pass over the lines in LDS with every band at that size: scale factor of the
 *                     stored maximum, mantissa -> the decoder's dequantiser -> n[k] = 4 (x - xh)^2, then the band sums
 *                     in k_nmr's order (lanes stride over the band, butterfly of shuffles).  One BitAlloc at the cap
 *                     budget 32 J (bitalloc_half, the encoder's own) gives the allocation of a unit that cannot have
 *                     what its bands ask for.
 *   k_band_pick       works on the arrays alone: one wave per channel-frame, a lane per (unit, band) pair scans the
 *                     band's sizes in ascending order for the first at or below the target; the unit sums go through
 *                     LDS, the frame's bits through the wave: band_frame (pick_dev.h) on the stored doubles
 *                     (BandCurveNmr), the frame work k_kept.hip runs on kept grid indices.
 *   k_band_pick_useg  pacx_band_pick_segments: k_band_pick with the target of the frame's segment, the segments uniform
 *                     stretches given by value ((first_off + cf) / seg_cf) and one grid target each in an array.
 *   k_band_pick_seg   pacx_band_solve / pacx_band_solve_segments: the same frame work with one SolveState per stretch of
 *                     consecutive channel-frames (the whole stream is one stretch); the wave finds its frame's segment
 *                     in the boundaries (segment_of, rate_dev.h) and adds the frame's bytes to that segment's total:
 *                     integer sums, one 64-bit atomicAdd per workgroup and segment present.  k_rate.hip's k_solve_init /
 *                     k_solve_step decide per segment.  <true>: pacx_band_solve_peak's picks at max(stream target,
 *                     segment floor), see there.
 *   k_band_sanitize   a caller's allocation made representable (below 2 -> 0, above maxMantBits -> maxMantBits), and
 *                     an all-zero allocation for a channel-frame whose record would leave PACX_PAYLOAD_STRIDE.
 *
 * All arithmetic that decides an integer code goes through pacx_exact.h and is compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"
#include "wave_fft.h"   /* wave_lds_fence */
#include "quant_dev.h"
#include "rate_dev.h"
#include "pick_dev.h"   /* band_frame, BandCurveNmr; frame_target (grid_dev.h) */

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int PICK_THREADS = 256;                  /* four channel-frames per workgroup, one per wave */

/* NMR_b of every band from the n[k] in S.v: lane b keeps band b's value (k_nmr's order of additions) */
template <int M>
__device__ __forceinline__ double band_nmr(const RateLds<M> &S, int nb, int lane)
{
    double mine = 0.0;
    for (int b = 0; b < nb; ++b) {
        double sn = 0.0;
        for (int k = lane; k < S.cnt[b]; k += 64)
            sn += S.v[S.lower[b] + k];
        sn = wave_sum(sn);
        const double r = 10.0 * log10((sn / (double)S.cnt[b] + PACX_EPS) / S.mm[b]);
        if (lane == b)
            mine = r;
    }
    return mine;
}

template <int M>
__global__ __launch_bounds__(64) void k_band_curve(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                  long long n_units, double max_bps,
                                                  const double *__restrict__ lines, const double *__restrict__ thr,
                                                  const double *__restrict__ smr, const int32_t *__restrict__ overall,
                                                  uint32_t *__restrict__ status, double *__restrict__ nmr,
                                                  int32_t *__restrict__ cap, int32_t *__restrict__ cap_alloc)
{
    constexpr bool SHORT = (M == PACX_M_SHORT);
    constexpr int PER = M / 64;
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
    /* slots of the row no band of this frame uses: no allocation */
    if (!SHORT || sb == PACX_SUB - 1)
        for (int s = (SHORT ? PACX_SUB * nb : nb) + lane; s < T.band_stride; s += 64)
            cap_alloc[cf * T.band_stride + s] = 0;
    if (!SHORT && lane < PACX_SUB)
        cap[cf * PACX_SUB + lane] = -1;            /* long frames use [0], written below by lane 0 again */
    if (SHORT) {
        unsigned st = 0;                           /* a hop the reference drops, as in k_rate_search */
        for (int c = 0; c < n_ch; ++c)
            st |= status[frame * n_ch + c];
        if (st & 2u) {
            if (lane < nb)
                cap_alloc[boff + lane] = 0;
            if (lane == 0)
                cap[cf * PACX_SUB + sb] = -1;
            return;
        }
    }
    const RateUnit u = rate_unit<M>(T, S, cf, sb, fl, max_bps, lines, thr, smr, overall);
    const double up = u.up, inv = u.inv;
    const int n_cand = u.max_mant;                 /* sizes 0, 2, 3, ..., maxMantBits */
    double *__restrict__ out = nmr + (boff + lane) * BAND_CAND;      /* lane b: the row of band b */

    /* ---- candidate 0: nothing is coded, the noise is the lines themselves */
#pragma unroll 1
    for (int j = 0; j < PER; ++j) {
        const int k = lane + 64 * j;
        const double e = S.x[k];
        S.v[k] = (e * e) * 4.0;
    }
    wave_lds_fence();
    {
        const double r = band_nmr<M>(S, nb, lane);
        if (lane < nb)
            out[0] = r;
    }
    wave_lds_fence();
    /* ---- candidates 1 ... n_cand - 1: every band with i + 1 bits */
    for (int i = 1; i < n_cand; ++i) {
        const int bits = i + 1;
        if (lane < nb)
            S.sf[lane] = pacx_scale_factor(__longlong_as_double((long long)S.bmax[lane]), T.n_scale_bits, bits);
        wave_lds_fence();
#pragma unroll 1
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            const int b = S.band[k];
            const double xv = S.x[k];
            double d = 0.0;
            if (b < nb)                            /* lines no band covers are not coded */
                d = pacx_dequantize(pacx_mantissa(xv * up, S.sf[b], T.n_scale_bits, bits), S.sf[b], T.n_scale_bits, bits);
            const double e = xv - d * inv;
            S.v[k] = (e * e) * 4.0;
        }
        wave_lds_fence();
        const double r = band_nmr<M>(S, nb, lane);
        if (lane < nb)
            out[i] = r;
        wave_lds_fence();                          /* v, sf free for the next size */
    }
    if (lane < nb)
        for (int i = n_cand; i < BAND_CAND; ++i)
            out[i] = INFINITY;

    /* ---- the allocation of a unit that cannot have what its bands ask for: BitAlloc at the cap budget */
    int bits = 0, acap = 0;
    bitalloc_half(half == 0, u.has, u.sv, u.nl, (double)(32 * u.J), u.max_mant, S.cp[half], half, l, bits, acap,
                  T.guard != 0, nb);
    if (u.has)
        cap_alloc[boff + l] = bits;
    if (lane == 0) {
        cap[cf * PACX_SUB + sb] = 32 * u.J;
        const unsigned st = ((acap & 1) ? 4u : 0u) | ((acap & 2) ? 16u : 0u);
        if (st)
            atomicOr(&status[cf], st);             /* PACX_ST_ALLOC_CAP, _GUARD */
    }
}

constexpr int PICK_WAVES = PICK_THREADS / 64;

/* band_frame for one channel-frame per wave at `target` (pacx_band_pick): the outputs are written */
__global__ __launch_bounds__(PICK_THREADS) void k_band_pick(PacxTables T, long long n_cf, double target,
                                                           const double *__restrict__ nmr,
                                                           const int32_t *__restrict__ cap,
                                                           const int32_t *__restrict__ cap_alloc,
                                                           int32_t *__restrict__ bit_alloc, int32_t *__restrict__ n_bytes,
                                                           uint8_t *__restrict__ capped)
{
    __shared__ int unit_sum[PICK_WAVES][PACX_SUB], unit_miss[PICK_WAVES][PACX_SUB];
    const int w = threadIdx.x >> 6;
    const long long cf = (long long)blockIdx.x * PICK_WAVES + w;
    if (cf < n_cf)                                 /* wave-uniform */
        band_frame(T, cf, BandCurveNmr{nmr, cap_alloc, target}, cap, true, bit_alloc, n_bytes, capped, unit_sum[w],
                   unit_miss[w]);
}

/* k_band_pick with one target per uniform segment (pacx_band_pick_segments): the wave's frame lies in segment
   (first_off + cf) / seg_cf and takes target_t[segment] / 64, read through the scalar cache */
__global__ __launch_bounds__(PICK_THREADS) void k_band_pick_useg(PacxTables T, long long n_cf, long long seg_cf,
                                                                long long first_off,
                                                                const int32_t *__restrict__ target_t,
                                                                const double *__restrict__ nmr,
                                                                const int32_t *__restrict__ cap,
                                                                const int32_t *__restrict__ cap_alloc,
                                                                int32_t *__restrict__ bit_alloc,
                                                                int32_t *__restrict__ n_bytes,
                                                                uint8_t *__restrict__ capped)
{
    __shared__ int unit_sum[PICK_WAVES][PACX_SUB], unit_miss[PICK_WAVES][PACX_SUB];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long cf = (long long)blockIdx.x * PICK_WAVES + w;
    if (cf < n_cf) {                               /* wave-uniform */
        const double target = (double)frame_target(target_t, 0, cf, seg_cf, first_off) / 64.0;
        band_frame(T, cf, BandCurveNmr{nmr, cap_alloc, target}, cap, true, bit_alloc, n_bytes, capped, unit_sum[w],
                   unit_miss[w]);
    }
}

/* k_band_pick as a pick of the solve, with a state per segment: the wave takes the target its frame's segment has in
   flight and adds to that segment's total; a frame whose segment is done is not scanned before the last launch.
   final: the last launch, at the targets found, which also writes the outputs.  A workgroup whose four frames lie in
   one segment (every workgroup of a whole-stream solve) adds once, one that straddles a boundary once per wave.
   PEAK (pacx_band_solve_peak, stage B; k_rate.hip, k_solve_pick): the segments' states rest with their floor in mid,
   the state in flight is the stream's, s[n_seg], and the wave's target is max(stream target, its segment's floor) --
   two more words through the scalar cache.  Before the last launch a workgroup adds its frames to the stream's total,
   once; the last launch adds per segment as above.  The instance without PEAK is the kernel as it was. */
template <bool PEAK>
__global__ __launch_bounds__(PICK_THREADS) void k_band_pick_seg(PacxTables T, SolveState *__restrict__ s,
                                                               const long long *__restrict__ seg_first, int n_seg,
                                                               int search_steps, long long n_cf,
                                                               const double *__restrict__ nmr,
                                                               const int32_t *__restrict__ cap,
                                                               const int32_t *__restrict__ cap_alloc, int final,
                                                               int32_t *__restrict__ bit_alloc,
                                                               int32_t *__restrict__ n_bytes,
                                                               uint8_t *__restrict__ capped)
{
    __shared__ int unit_sum[PICK_WAVES][PACX_SUB], unit_miss[PICK_WAVES][PACX_SUB];
    __shared__ unsigned long long part[PICK_WAVES];
    __shared__ int seg_of[PICK_WAVES];
    /* the wave's index in a scalar register: its frame, the boundaries searched and its segment's state are then read
       once per wave through the scalar cache, not by every lane (two vector loads less at the head of every wave) */
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long cf = (long long)blockIdx.x * PICK_WAVES + w;
    int seg = -1;                                  /* past the end: no segment, nothing to add */
    unsigned long long mine = 0ull;
    if (cf < n_cf) {                               /* wave-uniform, and so is everything read through seg */
        seg = segment_of(seg_first, n_seg, search_steps, cf);
        const SolveState *mystate = s + seg, *flying = PEAK ? s + n_seg : mystate;
        if (final || !flying->done) {
            int mid = flying->mid;
            if (PEAK && mystate->mid > mid)
                mid = mystate->mid;                /* the segment's floor */
            mine = band_frame(T, cf, BandCurveNmr{nmr, cap_alloc, (double)mid / 64.0}, cap, final != 0, bit_alloc,
                              n_bytes, capped, unit_sum[w], unit_miss[w]);
        }
    }
    if (lane == 0) {
        part[w] = mine;
        seg_of[w] = seg;
    }
    __syncthreads();
    const long long left = n_cf - (long long)blockIdx.x * PICK_WAVES;             /* >= 1: frames of this workgroup */
    const int last = left < PICK_WAVES ? (int)left - 1 : PICK_WAVES - 1;
    const bool whole = PEAK && !final;             /* the stream's total takes the workgroup as it is */
    if (whole || seg_of[0] == seg_of[last]) {      /* workgroup-uniform: one total */
        if (threadIdx.x == 0) {
            unsigned long long all = 0ull;
            for (int i = 0; i < PICK_WAVES; ++i)
                all += part[i];
            if (all)
                atomicAdd(&s[whole ? n_seg : seg_of[0]].total, all);
        }
    } else if (lane == 0 && seg >= 0 && mine) {
        atomicAdd(&s[seg].total, mine);
    }
}

/* a caller's allocation as k_quantize and k_pack may read it: one wave per channel-frame */
__global__ __launch_bounds__(64) void k_band_sanitize(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                     long long n_cf, const int32_t *in, int32_t *out,
                                                     uint32_t *__restrict__ status,
                                                     int payload_stride)
{
    constexpr int SLOTS = PACX_SUB * PACX_MAX_BANDS / 64;
    const int lane = threadIdx.x;
    const long long cf = blockIdx.x;
    if (cf >= n_cf)
        return;
    const bool is_short = flags && (flags[cf / n_ch] & 2u) != 0;
    const int nb = is_short ? T.nb_short : T.nb_long;
    const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
    const int n_slots = is_short ? PACX_SUB * nb : nb;
    int max_mant = 1 << T.n_mant_size_bits;
    if (max_mant > 16)
        max_mant = 16;
    const long long row = cf * T.band_stride;
    int a[SLOTS];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int slot = lane + 64 * q;
        a[q] = 0;
        if (slot < n_slots && slot < T.band_stride) {
            const int v = in[row + slot];
            a[q] = v < 2 ? 0 : (v > max_mant ? max_mant : v);
            sum += T.n_mant_size_bits + T.n_scale_bits + a[q] * count[is_short ? slot % nb : slot];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        sum += __shfl_xor(sum, off, 64);
    /* k_pack's size rule; a record that would leave its slot is coded without bits and flagged */
    const int nby = (sum + (is_short ? PACX_SUB : 1) * T.n_scale_bits + 4 + 7) >> 3;
    const bool fits = nby <= payload_stride;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int slot = lane + 64 * q;
        if (slot < T.band_stride)
            out[row + slot] = fits ? a[q] : 0;
    }
    if (!fits && lane == 0)
        atomicOr(&status[cf], 128u);               /* PACX_ST_RATE_CAP */
}

}  // namespace

void pacx_k::pacx_launch_band_curve(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                    double max_bits_per_sample, const double *lines, const double *thr,
                                    const double *smr, const int32_t *overall, uint32_t *status, double *nmr,
                                    int32_t *cap, int32_t *cap_alloc, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL((k_band_curve<PACX_M_LONG>), dim3((unsigned)n_cf), dim3(64), 0, st, T, flags, n_ch, n_cf,
                       max_bits_per_sample, lines, thr, smr, overall, status, nmr, cap, cap_alloc);
    if (flags)
        hipLaunchKernelGGL((k_band_curve<PACX_M_SHORT>), dim3((unsigned)(n_cf * PACX_SUB)), dim3(64), 0, st, T, flags,
                           n_ch, n_cf * PACX_SUB, max_bits_per_sample, lines, thr, smr, overall, status, nmr, cap,
                           cap_alloc);
}

void pacx_k::pacx_launch_band_pick(const PacxTables &T, long long n_cf, double target, const double *nmr,
                                   const int32_t *cap, const int32_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes,
                                   uint8_t *capped, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const unsigned grid = (unsigned)((n_cf + PICK_WAVES - 1) / PICK_WAVES);
    hipLaunchKernelGGL(k_band_pick, dim3(grid), dim3(PICK_THREADS), 0, st, T, n_cf, target, nmr, cap, cap_alloc, bit_alloc,
                       n_bytes, capped);
}

void pacx_k::pacx_launch_band_pick_segments(const PacxTables &T, long long n_cf, long long seg_cf, long long first_off,
                                            const int32_t *target_t, const double *nmr, const int32_t *cap,
                                            const int32_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes,
                                            uint8_t *capped, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const unsigned grid = (unsigned)((n_cf + PICK_WAVES - 1) / PICK_WAVES);
    hipLaunchKernelGGL(k_band_pick_useg, dim3(grid), dim3(PICK_THREADS), 0, st, T, n_cf, seg_cf, first_off, target_t, nmr,
                       cap, cap_alloc, bit_alloc, n_bytes, capped);
}

void pacx_k::pacx_launch_band_solve_segments(const PacxTables &T, const PacxSolve &v, const double *nmr,
                                             const int32_t *cap, const int32_t *cap_alloc, int32_t *bit_alloc,
                                             int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    const unsigned grid = (unsigned)((v.n_cf + PICK_WAVES - 1) / PICK_WAVES);
    pacx_solve_drive(v, st, [&](int search, int final) {
        hipLaunchKernelGGL(k_band_pick_seg<false>, dim3(grid), dim3(PICK_THREADS), 0, st, T, (SolveState *)v.ws, v.seg,
                           v.n_seg, search, v.n_cf, nmr, cap, cap_alloc, final, bit_alloc, n_bytes, capped);
    });
}

void pacx_k::pacx_launch_band_solve_peak(const PacxTables &T, const PacxSolve &v, const PacxSolveStream &p,
                                         const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                                         int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    const unsigned grid = (unsigned)((v.n_cf + PICK_WAVES - 1) / PICK_WAVES);
    pacx_peak_drive(v, p, st, [&](int search, int final, bool peak) {
        const auto pick = peak ? k_band_pick_seg<true> : k_band_pick_seg<false>;
        hipLaunchKernelGGL(pick, dim3(grid), dim3(PICK_THREADS), 0, st, T, (SolveState *)v.ws, v.seg, v.n_seg, search,
                           v.n_cf, nmr, cap, cap_alloc, final, bit_alloc, n_bytes, capped);
    });
}

void pacx_k::pacx_launch_band_sanitize(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                       const int32_t *in, int32_t *out, uint32_t *status, int payload_stride,
                                       hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_band_sanitize, dim3((unsigned)n_cf), dim3(64), 0, st, T, flags, n_ch, n_cf, in, out, status,
                       payload_stride);
}
