/*
 * pvq_dev.h -- the pyramid-VQ codebook layer the gain-shape encoder (k_vq.hip) and decoder
 * (k_vq_dec.hip) share: the resident tables, the codebook sizes N(l,k) / P(l,k) with their closed
 * forms for l <= 2, and the wave helpers both walks use.  No kernels and no LDS here: the LDS
 * copies of the row offsets and the per-kernel sizing stay with the kernels they are tuned for.
 * The other thing the two files share, the scalar rule of a split (angle bits, angle code and
 * value, mid/side bits) and the gain's quantiser, is vq_exact.h: it also builds for the host.
 */
#ifndef PACX_PVQ_DEV_H
#define PACX_PVQ_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* Codebook tables in HBM (pacx_vq_tables.h builds them).  VqView and VqDecView begin with one of
   these; pacx_create fills one and hands it to both pacx_*_view_fill.  The table of log2(tan) of the
   split angles stays a member of each view: it follows log_mu1 in VqView, and moving it in here
   would move kernarg offsets under the encoder's kernels. */
struct PvqTables {
    const uint64_t *n_tab, *p_tab;     /* rows l >= 3 of N(l,k) and of P(l,k) = sum_{j<=k} N(l,j) */
    const int32_t *row_off;            /* [l_max + 1] start of row l in the two tables */
    const int32_t *k_of;
    const uint8_t *w_of;
    const double *half_log2;
    int l_max;
};

/* N(l,k): vectors of l integers with k pulses */
__device__ __forceinline__ uint64_t pvq_N(const PvqTables &V, int l, long long k)
{
    if (k < 0)
        return 0;
    if (l <= 0)
        return k == 0 ? 1ull : 0ull;
    if (k == 0)
        return 1ull;
    if (l == 1)
        return 2ull;
    if (l == 2)
        return 4ull * (uint64_t)k;
    return V.n_tab[V.row_off[l] + k];
}

/* sum_{j=0..k} N(l,j); 0 for k < 0 */
__device__ __forceinline__ uint64_t pvq_P(const PvqTables &V, int l, long long k)
{
    if (k < 0)
        return 0;
    if (l <= 0)
        return 1ull;
    if (l == 1)
        return 1ull + 2ull * (uint64_t)k;
    if (l == 2)
        return 1ull + 2ull * (uint64_t)k * (uint64_t)(k + 1);
    return V.p_tab[V.row_off[l] + k];
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = v + __shfl_xor(v, off, 64);
    return v;
}

/* The device library's atan / log / log2(tan) / cos / sin / pow are polynomial evaluations with one
   or two dozen 64-bit coefficients.  Inlined into the band loop the compiler hoists every
   coefficient out of the loops into a VGPR pair of its own -- some sixty registers held for
   constants, which is what had k_vq at 168 VGPRs with 20 spilled (the spill reloads sat inside the
   Horner chains).  As real calls (once or twice per tree node, wave-uniform arguments) the
   coefficients live only inside the callee.  Each file defines the wrappers it calls with this. */
#define PVQ_LIBM_CALL __device__ __attribute__((noinline))

#endif
