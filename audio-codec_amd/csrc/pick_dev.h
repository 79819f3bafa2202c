/*
 * pick_dev.h -- the pick of one channel-frame on a stored curve, one per curve kind, parameterised by how an entry of
 * the curve is tested against the target.  k_band.hip and k_rate.hip test the stored double against the caller's
 * double target (a target of pacx_band_pick / pacx_rate_pick need not lie on any range's grid); k_kept.hip tests the
 * kept grid index e <= g (grid_dev.h, grid_threshold); k_rate_profile.hip runs the look-up at every entry of a grid.
 *
 *   curve_lookup        the look-up of a unit in a rate curve: the cap test on entry J first, then the bisection
 *   solve_frame<Ok>     pick(unit, T) for every unit of a channel-frame on a rate curve, by one thread
 *   band_frame<Curve>   the same on a band curve, by one wave; BandCurveNmr, BandCurveKept are the two curves
 */
#ifndef PACX_PICK_DEV_H
#define PACX_PICK_DEV_H

#include "grid_dev.h"   /* cand_bits */
#include "wave_fft.h"   /* wave_lds_fence */

constexpr int PICK_MAX_LOOKUP = 12;                /* halvings of a look-up: 1 + ceil(log2(J + 1)) for J < 2048 */

/* the step of a unit with steps 0 ... J whose entry passes, ok(j) non-decreasing in j as the coder makes it (else:
   the path of this bisection, not a minimum): the cap test on entry J first -- a unit that fails it takes J and sets
   `capped` -- then at most PICK_MAX_LOOKUP halvings */
template <class Ok>
__device__ __forceinline__ int curve_lookup(int J, Ok ok, bool &capped)
{
    int hi = J;
    if (!ok(J)) {
        capped = true;
    } else {
        int lo = -1;
        for (int it = 0; it < PICK_MAX_LOOKUP && hi - lo > 1; ++it) {
            const int mid = (lo + hi) / 2;
            if (ok(mid))
                hi = mid;
            else
                lo = mid;
        }
    }
    return hi;
}

/* pick(unit, T) of every unit of one channel-frame on a rate curve, the only one: the look-ups in the curve, the
   frame's bytes and, in the launch that writes (final), its outputs.  ok(i): entry i of the curve's arrays passes at
   the frame's target.  A J that would leave its row is cut to the row; a unit with steps < 0 does not exist.
   -> what the frame adds to the body: its bytes and their length prefix */
template <class Ok>
__device__ __forceinline__ unsigned long long solve_frame(long long cf, int row, int sub_stride, Ok ok,
                                                          const int32_t *__restrict__ bits,
                                                          const int32_t *__restrict__ steps, int final,
                                                          int32_t *__restrict__ budget, int32_t *__restrict__ n_bytes,
                                                          uint8_t *__restrict__ capped)
{
    int sum = 0, units = 0;
    bool cap = false;
    for (int sb = 0; sb < PACX_SUB; ++sb) {
        int J = steps[cf * PACX_SUB + sb];
        int b = 0;
        if (J >= 0) {
            const int base = sb * sub_stride;
            if (base + J >= row)                   /* never read past the row */
                J = row - 1 - base;
        }
        if (J >= 0) {
            const long long at = cf * (long long)row + sb * sub_stride;
            const int hi = curve_lookup(J, [&](int j) { return ok(at + j); }, cap);
            sum += bits[at + hi];
            b = 32 * hi;
            ++units;
        }
        if (final)
            budget[cf * PACX_SUB + sb] = b;
    }
    const int nby = units ? (sum + 4 + 7) >> 3 : 0;
    if (final) {
        n_bytes[cf] = nby;
        capped[cf] = cap ? 1 : 0;
    }
    return nby > 0 ? (unsigned long long)nby + 4ull : 0ull;
}

/* a band curve as stored, float64 [n_cf][band_stride][PACX_BAND_CAND], against a target in dB */
struct BandCurveNmr {
    const double *__restrict__ nmr;
    const int32_t *__restrict__ cap_alloc;
    double target;
    /* the lowest candidate below n_cand of band slot `at` that passes, or -1 */
    __device__ __forceinline__ int lowest(long long at, int n_cand) const
    {
        const double *__restrict__ r = nmr + at * PACX_BAND_CAND;
        int pick = -1;
        for (int i = n_cand - 1; i >= 0; --i)      /* the ascending scan's first pass = the lowest passing i */
            if (r[i] <= target)
                pick = i;
        return pick;
    }
    __device__ __forceinline__ int cap_alloc_of(long long at) const { return cap_alloc[at]; }
};

/* a band curve kept as grid indices (k_band_thresholds), uint16 [n_cf][band_stride][PACX_BAND_CAND], against the grid
   index g: the band's 16 indices in two 16-byte loads */
struct BandCurveKept {
    const uint16_t *__restrict__ e;
    const uint8_t *__restrict__ cap_alloc;
    int g;
    __device__ __forceinline__ int lowest(long long at, int n_cand) const
    {
        static_assert(PACX_BAND_CAND == 16, "a band's indices are two 16-byte loads");
        const uint4 *__restrict__ r = (const uint4 *)(e + at * PACX_BAND_CAND);
        const uint4 lo = r[0], hi = r[1];
        const unsigned w[PACX_BAND_CAND / 2] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        int pick = PACX_BAND_CAND;                 /* the lowest passing i of all 16: at or above n_cand, none below */
#pragma unroll
        for (int i = PACX_BAND_CAND - 1; i >= 0; --i) {
            const int ei = (int)(i & 1 ? w[i / 2] >> 16 : w[i / 2] & 0xffffu);
            if (ei <= g)
                pick = i;
        }
        return pick < n_cand ? pick : -1;
    }
    __device__ __forceinline__ int cap_alloc_of(long long at) const { return cap_alloc[at]; }
};

/* pick(unit, T) of include/pacx.h for every unit of one channel-frame on a band curve, by one wave, the only one: a
   lane per (unit, band) pair takes the lowest passing size of its band from the curve, the unit sums go through the
   wave's LDS row (unit_sum, unit_miss: PACX_SUB int32 each, zeroed here), the cap rule, the frame's bits through the
   wave.  write: the outputs are written.
   -> what the frame adds to the body: its bytes and their length prefix (every lane holds it) */
template <class Curve>
__device__ __forceinline__ unsigned long long band_frame(const PacxTables &T, long long cf, const Curve &curve,
                                                         const int32_t *__restrict__ cap, bool write,
                                                         int32_t *__restrict__ bit_alloc, int32_t *__restrict__ n_bytes,
                                                         uint8_t *__restrict__ capped, int *unit_sum, int *unit_miss)
{
    constexpr int SLOTS = PACX_SUB * PACX_MAX_BANDS / 64;          /* band slots of a row per lane, at most */
    const int lane = threadIdx.x & 63;
    if (lane < PACX_SUB) {
        unit_sum[lane] = 0;
        unit_miss[lane] = 0;
    }
    wave_lds_fence();
    const int32_t *__restrict__ cp = cap + cf * PACX_SUB;
    const bool is_short = cp[1] >= 0;              /* a long frame's slots 1-7 and a dropped hop's eight hold -1 */
    const int nb = is_short ? T.nb_short : T.nb_long;
    const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
    int n_cand = 1 << T.n_mant_size_bits;
    if (n_cand > PACX_BAND_CAND)
        n_cand = PACX_BAND_CAND;
    const long long row = cf * T.band_stride;
    int a[SLOTS], nl[SLOTS], sbs[SLOTS];
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int slot = lane + 64 * q;
        const int sb = is_short ? slot / nb : (slot < nb ? 0 : PACX_SUB);
        const int b = is_short ? slot - sb * nb : slot;
        a[q] = 0;
        nl[q] = 0;
        sbs[q] = -1;
        if (slot < T.band_stride && sb < PACX_SUB && cp[sb] >= 0) {
            const int pick = curve.lowest(row + slot, n_cand);
            sbs[q] = sb;
            nl[q] = count[b];
            a[q] = cand_bits(pick < 0 ? n_cand - 1 : pick);
            atomicAdd(&unit_sum[sb], a[q] * nl[q]);
            if (pick < 0)
                atomicOr(&unit_miss[sb], 1);
        }
    }
    wave_lds_fence();
    int sum = 0;
    bool any_cap = false;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int slot = lane + 64 * q;
        if (sbs[q] >= 0) {
            const bool over = unit_sum[sbs[q]] > cp[sbs[q]];
            if (over)
                a[q] = curve.cap_alloc_of(row + slot);
            any_cap = any_cap || over || unit_miss[sbs[q]] != 0;
            sum += T.n_mant_size_bits + T.n_scale_bits + a[q] * nl[q];
        }
        if (write && slot < T.band_stride)
            bit_alloc[row + slot] = a[q];
    }
    int units = 0;
    for (int sb = 0; sb < PACX_SUB; ++sb)
        units += cp[sb] >= 0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        sum += __shfl_xor(sum, off, 64);
    const bool cap_cf = __builtin_amdgcn_ballot_w64(any_cap) != 0ull;
    const int nby = units ? (sum + units * T.n_scale_bits + 4 + 7) >> 3 : 0;
    if (write && lane == 0) {
        n_bytes[cf] = nby;
        capped[cf] = cap_cf ? 1 : 0;
    }
    return nby > 0 ? (unsigned long long)nby + 4ull : 0ull;
}

#endif
