/*
 * k_rate.hip -- coding to a target noise-to-mask ratio (pacx_encode_pack_nmr_batch / pacx_encode_pack_budget_batch,
 * include/pacx.h): the BitAlloc budget of every long block and every short sub-block is a number of its own.
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
 *
 * All arithmetic that decides an integer code goes through pacx_exact.h and is compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"
#include "wave_fft.h"   /* wave_lds_fence */
#include "quant_dev.h"

using namespace pacx_k;

namespace {

constexpr int RATE_MAX_EVAL = 12;                  /* 1 + ceil(log2(J + 1)) for J < 2048; the entry point keeps J <= 512 */
constexpr int RATE_SLOTS = PACX_MAX_BANDS + 1;     /* the bands and the dummy band of the lines no band covers */

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
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
    constexpr int PER = M / 64;                    /* lines per lane */
    __shared__ double v_l[M];                      /* m[k] while the band means are taken, then n[k] of an evaluation */
    __shared__ double x_l[M];                      /* the unit's lines */
    __shared__ uint8_t band_l[M];                  /* band of every line (nb: none) */
    __shared__ double cp[2][32];
    __shared__ double mm_s[PACX_MAX_BANDS];        /* M_b */
    __shared__ unsigned long long bmax[RATE_SLOTS];
    __shared__ int ba_s[RATE_SLOTS], sf_s[RATE_SLOTS], lower_s[PACX_MAX_BANDS], cnt_s[PACX_MAX_BANDS];
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

    /* ---- what every evaluation shares: line lane + 64 j belongs to lane `lane` (coalesced, and LDS without bank
       conflicts); the lines stay in LDS, so the evaluations' line loop need not be unrolled */
    const long long loff = cf * PACX_M_LONG + sb * PACX_M_SHORT;
    const uint8_t *__restrict__ band_of = SHORT ? T.line_band_short : T.line_band_long;
    const int ov = overall[cf * PACX_SUB + sb];
    const double up = (double)(1 << ov);           /* mdctLines *= (1 << overallScale) */
    const double inv = ldexp(1.0, -ov);            /* the decoder's division: a power of two, exact */
    if (lane < RATE_SLOTS) {
        bmax[lane] = 0ull;
        ba_s[lane] = 0;
        sf_s[lane] = 0;
    }
    const int32_t *__restrict__ lower = SHORT ? T.band_lower_short : T.band_lower_long;
    const int32_t *__restrict__ count = SHORT ? T.band_lines_short : T.band_lines_long;
    if (lane < nb) {
        int cnt = count[lane];
        if (lower[lane] + cnt > M)                 /* a table that runs past the block (build_bands refuses it) */
            cnt = M - lower[lane];
        lower_s[lane] = lower[lane];
        cnt_s[lane] = cnt;
    }
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int k = lane + 64 * j;
        const double xv = lines[loff + k];
        x_l[k] = xv;
        band_l[k] = band_of[k];
        /* 10^y by exp2(y log2 10), as k_nmr */
        v_l[k] = exp2(((thr[loff + k] - 96.0) / 10.0) * 3.32192809488736234787);
        /* band maxima of |x 2^overall| on the bit pattern (quant_dev.h, long_scale_factors): they do not depend on the
           allocation, only the scale factor taken from them does */
        atomicMax(&bmax[band_of[k]], (unsigned long long)__double_as_longlong(fabs(xv * up)));
    }
    wave_lds_fence();
    for (int b = 0; b < nb; ++b) {
        double sm = 0.0;
        for (int k = lane; k < cnt_s[b]; k += 64)
            sm += v_l[lower_s[b] + k];
        sm = wave_sum(sm);
        if (lane == 0)
            mm_s[b] = sm / (double)cnt_s[b];
    }
    wave_lds_fence();

    const double sv = has ? smr[boff + l] : 0.0;
    const int nl = has ? count[l] : 0;
    int max_mant = 1 << T.n_mant_size_bits;
    if (max_mant > 16)
        max_mant = 16;
    /* the existing rule with the cap rate in place of the handle's */
    const double cap = pacx_bit_budget(max_bps, M, SHORT ? 1 : 0, (fl & 5u) != 0, T.n_scale_bits, T.n_mant_size_bits, nb,
                                       0, 0);
    const double jf = floor(cap / 32.0);
    const int J = jf > 0.0 ? (jf < 2047.0 ? (int)jf : 2047) : 0;

    /* ---- the search: 32 J first, then the bisection */
    int lo = -1, hi = J, mid = J;
    int best = 0, best_cap = 0;
    bool capped = false;
    for (int it = 0; it < RATE_MAX_EVAL; ++it) {
        int bits = 0, acap = 0;
        bitalloc_half(half == 0, has, sv, nl, (double)(32 * mid), max_mant, cp[half], half, l, bits, acap, T.guard != 0,
                      nb);
        if (has) {
            ba_s[l] = bits;
            sf_s[l] = pacx_scale_factor(__longlong_as_double((long long)bmax[l]), T.n_scale_bits, bits);
        }
        wave_lds_fence();
#pragma unroll 1
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            const int b = band_l[k];
            const int ba = ba_s[b];
            const double xv = x_l[k];
            double d = 0.0;
            if (ba)
                d = pacx_dequantize(pacx_mantissa(xv * up, sf_s[b], T.n_scale_bits, ba), sf_s[b], T.n_scale_bits, ba);
            const double e = xv - d * inv;
            v_l[k] = (e * e) * 4.0;
        }
        wave_lds_fence();
        double worst = -INFINITY;
        for (int b = 0; b < nb; ++b) {
            double sn = 0.0;
            for (int k = lane; k < cnt_s[b]; k += 64)
                sn += v_l[lower_s[b] + k];
            sn = wave_sum(sn);
            const double r = 10.0 * log10((sn / (double)cnt_s[b] + PACX_EPS) / mm_s[b]);
            worst = r > worst ? r : worst;
        }
        const bool ok = __shfl(worst <= target_db ? 1 : 0, 0, 64) != 0;       /* wave-uniform */
        wave_lds_fence();                          /* v_l, ba_s, sf_s free for the next evaluation */
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

}  // namespace

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
