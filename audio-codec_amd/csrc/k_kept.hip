/*
 * k_kept.hip -- a curve in the integer form that decides a pick on the grid, and the picks on that form
 * (pacx_band_thresholds, pacx_band_pick_thresholds[_segments], pacx_rate_thresholds, pacx_rate_pick_thresholds[_segments],
 * include/pacx.h).  A curve entry x passes at the grid target t iff 64 x <= t, so all that a pick at a target of
 * [t_lo, t_hi] reads of x is the grid index from which it passes, e = ceil(64 x) - t_lo cut to [0, G] (G: never):
 * 16 bits where the curve has 64.  k_profile.hip and k_rate_profile.hip work these indices out in LDS per frame; here
 * they are written out, so that a chunked encode can keep them between its passes instead of taking the curve twice.
 *
 *   k_band_thresholds  one workgroup per channel-frame, a thread per pair of candidates of a band slot: one 16-byte
 *                      load of the curve, one packed 4-byte store of two indices.  Every entry of the row is written
 *                      (G where there is no band, no unit or no such size); cap is copied, cap_alloc narrowed to a byte
 *                      (0 where there is no band).
 *   k_rate_thresholds  one workgroup per channel-frame, a thread per entry of the row: G and 0 bits where no unit uses
 *                      the entry; steps with a J that would leave the row cut to the row, as the pick cuts it.
 *   k_band_pick_kept   k_band_pick's frame work (k_band.hip, band_frame: repeated here, that file is left as it is)
 *                      with e_i <= g in place of nmr[i] <= T: one wave per channel-frame, a lane per (unit, band) pair,
 *                      the band's 16 indices in two 16-byte loads.
 *   k_rate_pick_kept   k_rate_pick's frame work (k_rate.hip, solve_frame) with ok(j) := e_j <= g: one channel-frame per
 *                      thread.
 * The picks take one grid target per uniform segment (frame cf lies in segment (first_off + cf) / seg_cf), or, without
 * an array, one for all frames by value: the one-segment case.  A target outside the range is clamped into it.
 * Trip counts come from tables and arguments only; integer arithmetic after the one comparison in double.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"
#include "wave_fft.h"   /* wave_lds_fence */

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int KEPT_THREADS = 256;
constexpr int KEPT_WAVES = KEPT_THREADS / 64;      /* channel-frames per workgroup of the band pick, one per wave */
constexpr int KEPT_MAX_LOOKUP = 12;                /* k_rate.hip, SOLVE_MAX_LOOKUP: the bisection's bound */

static_assert(PACX_PROFILE_MAX < 65536, "grid indices are kept in 16 bits");
static_assert(BAND_CAND == 16, "a band's indices are two 16-byte loads");

__device__ __forceinline__ int cand_bits(int i) { return i ? i + 1 : 0; }

/* the grid index from which x passes: r <= t / 64 is 64 r <= t, both scalings exact; decided in double: NaN and +inf
   fail the first comparison, -inf and anything at or below the range pass the second, and only what lies in
   (t_lo, t_hi] reaches the cast */
__device__ __forceinline__ unsigned threshold_of(double v, int t_lo, int t_hi)
{
    const double x = v * (double)PACX_RATE_TARGET_GRID;
    if (!(x <= (double)t_hi))
        return (unsigned)(t_hi - t_lo + 1);
    return x <= (double)t_lo ? 0u : (unsigned)((int)ceil(x) - t_lo);
}

/* the frame's target as a grid index: of its segment, or the one given by value; clamped into the range */
__device__ __forceinline__ int grid_index(const int32_t *__restrict__ target_t, int t_all, long long cf, long long seg_cf,
                                          long long first_off, int t_lo, int t_hi)
{
    const int t = target_t ? target_t[(first_off + cf) / seg_cf] : t_all;
    return (t < t_lo ? t_lo : (t > t_hi ? t_hi : t)) - t_lo;
}

/* pairs: band_stride * BAND_CAND / 2, the 16-byte pieces of a frame's row */
__global__ __launch_bounds__(KEPT_THREADS) void k_band_thresholds(PacxTables T, long long n_cf, int pairs, int t_lo,
                                                                 int t_hi, const double *__restrict__ nmr,
                                                                 const int32_t *__restrict__ cap,
                                                                 const int32_t *__restrict__ cap_alloc,
                                                                 uint16_t *__restrict__ e, int32_t *__restrict__ kcap,
                                                                 uint8_t *__restrict__ kcap_alloc)
{
    const long long cf = blockIdx.x;
    if (cf >= n_cf)
        return;
    const unsigned G = (unsigned)(t_hi - t_lo + 1);
    const int32_t *__restrict__ cp = cap + cf * PACX_SUB;
    const bool is_short = cp[1] >= 0;              /* a long frame's slots 1-7 and a dropped hop's eight hold -1 */
    const int nb = is_short ? T.nb_short : T.nb_long;
    int n_cand = 1 << T.n_mant_size_bits;
    if (n_cand > BAND_CAND)
        n_cand = BAND_CAND;
    const long long row = cf * T.band_stride;
    const double2 *__restrict__ in = (const double2 *)(nmr + row * BAND_CAND);
    unsigned *__restrict__ out = (unsigned *)(e + row * BAND_CAND);
    if (threadIdx.x < PACX_SUB)
        kcap[cf * PACX_SUB + threadIdx.x] = cp[threadIdx.x];
    for (int p = threadIdx.x; p < pairs; p += KEPT_THREADS) {
        const int slot = p / (BAND_CAND / 2), i = 2 * (p % (BAND_CAND / 2));
        const int sb = is_short ? slot / nb : (slot < nb ? 0 : PACX_SUB);
        const bool live = sb < PACX_SUB && cp[sb] >= 0;
        unsigned e0 = G, e1 = G;
        if (live) {
            const double2 v = in[p];
            if (i < n_cand)
                e0 = threshold_of(v.x, t_lo, t_hi);
            if (i + 1 < n_cand)
                e1 = threshold_of(v.y, t_lo, t_hi);
        }
        out[p] = e0 | (e1 << 16);
        if (i == 0) {
            int a = 0;
            if (live) {
                a = cap_alloc[row + slot];
                a = a < 0 ? 0 : (a > 255 ? 255 : a);
            }
            kcap_alloc[row + slot] = (uint8_t)a;
        }
    }
}

__global__ __launch_bounds__(KEPT_THREADS) void k_rate_thresholds(long long n_cf, int row, int sub_stride, int t_lo,
                                                                 int t_hi, const double *__restrict__ worst,
                                                                 const int32_t *__restrict__ bits,
                                                                 const int32_t *__restrict__ steps,
                                                                 uint16_t *__restrict__ e, int32_t *__restrict__ kbits,
                                                                 int32_t *__restrict__ ksteps)
{
    const long long cf = blockIdx.x;
    if (cf >= n_cf)
        return;
    const unsigned G = (unsigned)(t_hi - t_lo + 1);
    int J[PACX_SUB];
#pragma unroll
    for (int sb = 0; sb < PACX_SUB; ++sb) {        /* workgroup-uniform */
        J[sb] = steps[cf * PACX_SUB + sb];
        const int base = sb * sub_stride;
        if (J[sb] >= 0 && base + J[sb] >= row)     /* a J that would leave its row is cut to the row */
            J[sb] = row - 1 - base;
    }
    if (threadIdx.x < PACX_SUB) {
        int mine = -1;
#pragma unroll
        for (int sb = 0; sb < PACX_SUB; ++sb)
            mine = (int)threadIdx.x == sb ? J[sb] : mine;
        ksteps[cf * PACX_SUB + threadIdx.x] = mine;
    }
    const long long at = cf * (long long)row;
    for (int j = threadIdx.x; j < row; j += KEPT_THREADS) {
        bool used = false;
#pragma unroll
        for (int sb = 0; sb < PACX_SUB; ++sb)
            used = used || (J[sb] >= 0 && j >= sb * sub_stride && j - sb * sub_stride <= J[sb]);
        unsigned ej = G;
        int bj = 0;
        if (used) {
            ej = threshold_of(worst[at + j], t_lo, t_hi);
            bj = bits[at + j];
        }
        e[at + j] = (uint16_t)ej;
        kbits[at + j] = bj;
    }
}

/* band_frame of k_band.hip on the indices: pick(unit, T) for every unit of one channel-frame at the grid index g, by
   one wave.  unit_sum, unit_miss: the wave's LDS rows, zeroed here */
__device__ __forceinline__ void kept_band_frame(const PacxTables &T, long long cf, int g, const uint16_t *__restrict__ e,
                                                const int32_t *__restrict__ cap, const uint8_t *__restrict__ cap_alloc,
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
    const bool is_short = cp[1] >= 0;
    const int nb = is_short ? T.nb_short : T.nb_long;
    const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
    int n_cand = 1 << T.n_mant_size_bits;
    if (n_cand > BAND_CAND)
        n_cand = BAND_CAND;
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
            const uint4 *__restrict__ r = (const uint4 *)(e + (row + slot) * BAND_CAND);
            const uint4 lo = r[0], hi = r[1];
            const unsigned w[BAND_CAND / 2] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            int pick = -1;
#pragma unroll
            for (int i = BAND_CAND - 1; i >= 0; --i) {             /* the ascending scan's first pass = the lowest passing i */
                const int ei = (int)(i & 1 ? w[i / 2] >> 16 : w[i / 2] & 0xffffu);
                if (i < n_cand && ei <= g)
                    pick = i;
            }
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
                a[q] = cap_alloc[row + slot];
            any_cap = any_cap || over || unit_miss[sbs[q]] != 0;
            sum += T.n_mant_size_bits + T.n_scale_bits + a[q] * nl[q];
        }
        if (slot < T.band_stride)
            bit_alloc[row + slot] = a[q];
    }
    int units = 0;
    for (int sb = 0; sb < PACX_SUB; ++sb)
        units += cp[sb] >= 0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        sum += __shfl_xor(sum, off, 64);
    const bool cap_cf = __builtin_amdgcn_ballot_w64(any_cap) != 0ull;
    if (lane == 0) {
        n_bytes[cf] = units ? (sum + units * T.n_scale_bits + 4 + 7) >> 3 : 0;
        capped[cf] = cap_cf ? 1 : 0;
    }
}

__global__ __launch_bounds__(KEPT_THREADS) void k_band_pick_kept(PacxTables T, long long n_cf, long long seg_cf,
                                                                long long first_off,
                                                                const int32_t *__restrict__ target_t, int t_all,
                                                                int t_lo, int t_hi, const uint16_t *__restrict__ e,
                                                                const int32_t *__restrict__ cap,
                                                                const uint8_t *__restrict__ cap_alloc,
                                                                int32_t *__restrict__ bit_alloc,
                                                                int32_t *__restrict__ n_bytes,
                                                                uint8_t *__restrict__ capped)
{
    __shared__ int unit_sum[KEPT_WAVES][PACX_SUB], unit_miss[KEPT_WAVES][PACX_SUB];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long cf = (long long)blockIdx.x * KEPT_WAVES + w;
    if (cf < n_cf)                                 /* wave-uniform */
        kept_band_frame(T, cf, grid_index(target_t, t_all, cf, seg_cf, first_off, t_lo, t_hi), e, cap, cap_alloc,
                        bit_alloc, n_bytes, capped, unit_sum[w], unit_miss[w]);
}

/* solve_frame of k_rate.hip on the indices: one channel-frame per thread */
__global__ __launch_bounds__(KEPT_THREADS) void k_rate_pick_kept(long long n_cf, long long seg_cf, long long first_off,
                                                                const int32_t *__restrict__ target_t, int t_all,
                                                                int t_lo, int t_hi, int row, int sub_stride,
                                                                const uint16_t *__restrict__ e,
                                                                const int32_t *__restrict__ bits,
                                                                const int32_t *__restrict__ steps,
                                                                int32_t *__restrict__ budget,
                                                                int32_t *__restrict__ n_bytes,
                                                                uint8_t *__restrict__ capped)
{
    const long long cf = (long long)blockIdx.x * KEPT_THREADS + threadIdx.x;
    if (cf >= n_cf)
        return;
    const int g = grid_index(target_t, t_all, cf, seg_cf, first_off, t_lo, t_hi);
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
            int hi = J;
            if (!((int)e[at + J] <= g)) {          /* the cap test on entry J comes first */
                cap = true;
            } else {
                int lo = -1;
                for (int it = 0; it < KEPT_MAX_LOOKUP && hi - lo > 1; ++it) {
                    const int mid = (lo + hi) / 2;
                    if ((int)e[at + mid] <= g)
                        hi = mid;
                    else
                        lo = mid;
                }
            }
            sum += bits[at + hi];
            b = 32 * hi;
            ++units;
        }
        budget[cf * PACX_SUB + sb] = b;
    }
    n_bytes[cf] = units ? (sum + 4 + 7) >> 3 : 0;
    capped[cf] = cap ? 1 : 0;
}

}  // namespace

void pacx_k::pacx_launch_band_thresholds(const PacxTables &T, long long n_cf, int t_lo, int t_hi, const double *nmr,
                                         const int32_t *cap, const int32_t *cap_alloc, uint16_t *e, int32_t *kept_cap,
                                         uint8_t *kept_cap_alloc, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_band_thresholds, dim3((unsigned)n_cf), dim3(KEPT_THREADS), 0, st, T, n_cf,
                       T.band_stride * (BAND_CAND / 2), t_lo, t_hi, nmr, cap, cap_alloc, e, kept_cap, kept_cap_alloc);
}

void pacx_k::pacx_launch_band_pick_thresholds(const PacxTables &T, long long n_cf, long long seg_cf, long long first_off,
                                              const int32_t *target_t, int t_all, int t_lo, int t_hi, const uint16_t *e,
                                              const int32_t *cap, const uint8_t *cap_alloc, int32_t *bit_alloc,
                                              int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const unsigned grid = (unsigned)((n_cf + KEPT_WAVES - 1) / KEPT_WAVES);
    hipLaunchKernelGGL(k_band_pick_kept, dim3(grid), dim3(KEPT_THREADS), 0, st, T, n_cf, seg_cf, first_off, target_t, t_all,
                       t_lo, t_hi, e, cap, cap_alloc, bit_alloc, n_bytes, capped);
}

void pacx_k::pacx_launch_rate_thresholds(long long n_cf, int row, int sub_stride, int t_lo, int t_hi, const double *worst,
                                         const int32_t *bits, const int32_t *steps, uint16_t *e, int32_t *kept_bits,
                                         int32_t *kept_steps, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_rate_thresholds, dim3((unsigned)n_cf), dim3(KEPT_THREADS), 0, st, n_cf, row, sub_stride, t_lo,
                       t_hi, worst, bits, steps, e, kept_bits, kept_steps);
}

void pacx_k::pacx_launch_rate_pick_thresholds(long long n_cf, int row, int sub_stride, long long seg_cf,
                                              long long first_off, const int32_t *target_t, int t_all, int t_lo, int t_hi,
                                              const uint16_t *e, const int32_t *bits, const int32_t *steps,
                                              int32_t *budget, int32_t *n_bytes, uint8_t *capped, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    const unsigned grid = (unsigned)((n_cf + KEPT_THREADS - 1) / KEPT_THREADS);
    hipLaunchKernelGGL(k_rate_pick_kept, dim3(grid), dim3(KEPT_THREADS), 0, st, n_cf, seg_cf, first_off, target_t, t_all,
                       t_lo, t_hi, row, sub_stride, e, bits, steps, budget, n_bytes, capped);
}
