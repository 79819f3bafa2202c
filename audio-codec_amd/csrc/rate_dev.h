/*
 * rate_dev.h -- what the kernels that code to a noise-to-mask target share: k_rate.hip (the budget search, the rate
 * curve, the solve) and k_band.hip (the band-by-band allocation).  One wave per unit -- a long block or a short
 * sub-block: the unit's preamble (lines, line bands, band maxima and band means of the mask into LDS), the wave sum
 * of k_nmr's order, and the few words of state of a solve with the decision taken on them (k_bucket.hip shares those
 * two).  Included with -ffp-contract=off like the files it serves.
 */
#ifndef PACX_RATE_DEV_H
#define PACX_RATE_DEV_H

#include <math.h>

#include "grid_dev.h"   /* narrow_half */
#include "pacx_dev.h"
#include "wave_fft.h"   /* wave_lds_fence */

constexpr int RATE_SLOTS = PACX_MAX_BANDS + 1;     /* the bands and the dummy band of the lines no band covers */

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

/* what a unit's evaluations share, in LDS */
template <int M>
struct RateLds {
    double v[M];                                   /* m[k] while the band means are taken, then n[k] of an evaluation */
    double x[M];                                   /* the unit's lines */
    uint8_t band[M];                               /* band of every line (nb: none) */
    double cp[2][32];
    double mm[PACX_MAX_BANDS];                     /* M_b */
    unsigned long long bmax[RATE_SLOTS];
    int ba[RATE_SLOTS], sf[RATE_SLOTS], lower[PACX_MAX_BANDS], cnt[PACX_MAX_BANDS];
};

/* and in registers */
struct RateUnit {
    int nb, nl, max_mant, J;
    bool has;                                      /* BitAlloc's lanes: band l on the first half wave */
    double sv, up, inv;
};

/* the preamble of k_rate_search, k_rate_curve and k_band_curve: lines, line bands, band maxima and the band means of the mask into
   LDS, the unit's SMRs and J into registers.  Called by the whole wave. */
template <int M>
__device__ __forceinline__ RateUnit rate_unit(const PacxTables &T, RateLds<M> &S, long long cf, int sb, unsigned fl,
                                              double max_bps, const double *__restrict__ lines,
                                              const double *__restrict__ thr, const double *__restrict__ smr,
                                              const int32_t *__restrict__ overall)
{
    constexpr bool SHORT = (M == PACX_M_SHORT);
    constexpr int PER = M / 64;                    /* lines per lane */
    const int lane = threadIdx.x, half = lane >> 5, l = lane & 31;
    RateUnit u;
    u.nb = SHORT ? T.nb_short : T.nb_long;
    const int nb = u.nb;
    const long long boff = cf * T.band_stride + sb * nb;
    u.has = half == 0 && l < nb;
    /* ---- what every evaluation shares: line lane + 64 j belongs to lane `lane` (coalesced, and LDS without bank
       conflicts); the lines stay in LDS, so the evaluations' line loop need not be unrolled */
    const long long loff = cf * PACX_M_LONG + sb * PACX_M_SHORT;
    const uint8_t *__restrict__ band_of = SHORT ? T.line_band_short : T.line_band_long;
    const int ov = overall[cf * PACX_SUB + sb];
    u.up = (double)(1 << ov);                      /* mdctLines *= (1 << overallScale) */
    u.inv = ldexp(1.0, -ov);                       /* the decoder's division: a power of two, exact */
    const double up = u.up;
    if (lane < RATE_SLOTS) {
        S.bmax[lane] = 0ull;
        S.ba[lane] = 0;
        S.sf[lane] = 0;
    }
    const int32_t *__restrict__ lower = SHORT ? T.band_lower_short : T.band_lower_long;
    const int32_t *__restrict__ count = SHORT ? T.band_lines_short : T.band_lines_long;
    if (lane < nb) {
        int cnt = count[lane];
        if (lower[lane] + cnt > M)                 /* a table that runs past the block (build_bands refuses it) */
            cnt = M - lower[lane];
        S.lower[lane] = lower[lane];
        S.cnt[lane] = cnt;
    }
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int k = lane + 64 * j;
        const double xv = lines[loff + k];
        S.x[k] = xv;
        S.band[k] = band_of[k];
        /* 10^y by exp2(y log2 10), as k_nmr */
        S.v[k] = exp2(((thr[loff + k] - 96.0) / 10.0) * 3.32192809488736234787);
        /* band maxima of |x 2^overall| on the bit pattern (quant_dev.h, long_scale_factors): they do not depend on the
           allocation, only the scale factor taken from them does */
        atomicMax(&S.bmax[band_of[k]], (unsigned long long)__double_as_longlong(fabs(xv * up)));
    }
    wave_lds_fence();
    for (int b = 0; b < nb; ++b) {
        double sm = 0.0;
        for (int k = lane; k < S.cnt[b]; k += 64)
            sm += S.v[S.lower[b] + k];
        sm = wave_sum(sm);
        if (lane == 0)
            S.mm[b] = sm / (double)S.cnt[b];
    }
    wave_lds_fence();

    u.sv = u.has ? smr[boff + l] : 0.0;
    u.nl = u.has ? count[l] : 0;
    u.max_mant = 1 << T.n_mant_size_bits;
    if (u.max_mant > 16)
        u.max_mant = 16;
    /* the existing rule with the cap rate in place of the handle's */
    u.J = pacx_rate_steps(max_bps, M, SHORT ? 1 : 0, (fl & 5u) != 0, T.n_scale_bits, T.n_mant_size_bits, nb);
    return u;
}

/* lo / hi / mid on the target grid, t = 64 T */
struct SolveState {
    int lo, hi, mid;
    int phase;                                     /* 0: total(t_hi) is being taken, 1: the bisection */
    int done, met;
    unsigned long long total;                      /* of the pick in flight */
};

/* the decision of include/pacx.h (pacx_rate_solve) on whether the pick at s->mid fits, the only one: k_rate.hip's
   solve_step takes it on total <= limit, k_bucket.hip's k_bucket_step with the bucket's peak as a second condition */
__device__ __forceinline__ void solve_decide(SolveState *s, bool fits)
{
    if (s->done)
        return;
    if (s->phase == 0) {
        if (!fits) {                               /* unreachable: the largest target, met = 0 */
            s->done = 1;
            return;                                /* mid stays t_hi */
        }
        s->met = 1;
        s->phase = 1;
    }
    if (narrow_half(s->lo, s->hi, s->mid, fits))
        s->done = 1;
}

/* the segment of channel-frame cf, 0 <= cf < first[n_seg]: the s with first[s] <= cf < first[s + 1] (first[0] = 0,
   non-decreasing, so an empty segment is never the answer).  `steps` halvings, pacx_segment_search_steps(n_seg) of
   them: the trip count is the caller's argument, not the data's. */
__device__ __forceinline__ int segment_of(const long long *__restrict__ first, int n_seg, int steps, long long cf)
{
    int lo = 0, hi = n_seg;                        /* first[lo] <= cf < first[hi] */
    for (int it = 0; it < steps; ++it) {
        const int mid = lo + (hi - lo) / 2;
        if (hi - lo > 1) {
            if (first[mid] <= cf)
                lo = mid;
            else
                hi = mid;
        }
    }
    return lo;
}

#endif
