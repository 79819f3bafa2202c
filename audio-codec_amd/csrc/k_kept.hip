/*
 * k_kept.hip -- a curve in the integer form that decides a pick on the grid, and the picks on that form
 * (pacx_band_thresholds, pacx_band_pick_thresholds[_segments], pacx_rate_thresholds, pacx_rate_pick_thresholds[_segments],
 * include/pacx.h).  A curve entry x passes at the grid target t iff 64 x <= t, so all that a pick at a target of
 * [t_lo, t_hi] reads of x is the grid index from which it passes, e = ceil(64 x) - t_lo cut to [0, G] (G: never):
 * 16 bits where the curve has 64 (grid_threshold, grid_dev.h).  The profile kernels work these indices out in LDS per
 * frame; here they are written out, so that a chunked encode can keep them between its passes instead of taking the
 * curve twice.
 *
 *   k_band_thresholds  one workgroup per channel-frame, a thread per pair of candidates of a band slot: one 16-byte
 *                      load of the curve, one packed 4-byte store of two indices.  Every entry of the row is written
 *                      (G where there is no band, no unit or no such size); cap is copied, cap_alloc narrowed to a byte
 *                      (0 where there is no band).
 *   k_rate_thresholds  one workgroup per channel-frame, a thread per entry of the row: G and 0 bits where no unit uses
 *                      the entry; steps with a J that would leave the row cut to the row, as the pick cuts it.
 *   k_band_pick_kept   band_frame (pick_dev.h), k_band_pick's frame work, on the kept curve (BandCurveKept: e_i <= g in
 *                      place of nmr[i] <= T): one wave per channel-frame, a lane per (unit, band) pair.
 *   k_rate_pick_kept   solve_frame (pick_dev.h), k_rate_pick's frame work, with ok(j) := e_j <= g: one channel-frame per
 *                      thread.
 * The picks take one grid target per uniform segment or one for all frames by value (frame_target), clamped into the
 * range (grid_clamp, both grid_dev.h).
 * Trip counts come from tables and arguments only; integer arithmetic after the one comparison in double.
 */
#include <hip/hip_runtime.h>

#include "grid_dev.h"
#include "pick_dev.h"

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int KEPT_THREADS = 256;
constexpr int KEPT_WAVES = KEPT_THREADS / 64;      /* channel-frames per workgroup of the band pick, one per wave */

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
                e0 = grid_threshold(v.x, t_lo, t_hi);
            if (i + 1 < n_cand)
                e1 = grid_threshold(v.y, t_lo, t_hi);
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
            ej = grid_threshold(worst[at + j], t_lo, t_hi);
            bj = bits[at + j];
        }
        e[at + j] = (uint16_t)ej;
        kbits[at + j] = bj;
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
    if (cf < n_cf) {                               /* wave-uniform */
        const int g = grid_clamp(frame_target(target_t, t_all, cf, seg_cf, first_off), t_lo, t_hi);
        band_frame(T, cf, BandCurveKept{e, cap_alloc, g}, cap, true, bit_alloc, n_bytes, capped, unit_sum[w],
                   unit_miss[w]);
    }
}

/* solve_frame on the indices: one channel-frame per thread */
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
    const int g = grid_clamp(frame_target(target_t, t_all, cf, seg_cf, first_off), t_lo, t_hi);
    solve_frame(cf, row, sub_stride, [&](long long i) { return (int)e[i] <= g; }, bits, steps, 1, budget, n_bytes,
                capped);
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
