/*
 * k_vq_band.hip -- the band curve of the gain-shape coder (pacx_vq_band_curve_batch, include/pacx.h).  Without SBR
 * the noise of a gain-shape coded band depends on that band's own allocation and on nothing else, so the curve is
 * taken with the coder and the decoder themselves: one pass per size with every band at that size through k_vq*,
 * k_vq_dec* and k_nmr.  What is left to do around those passes is here, all of it a few words per channel-frame:
 *
 *   k_vq_band_cap     cap = 32 J of every unit (pacx_rate_steps with the cap rate, as k_band_curve takes it), -1 where
 *                     there is none, and the same numbers as budgets (0 where there is no unit) for k_bitalloc_budget,
 *                     which makes cap_alloc of them.
 *   k_vq_band_fill    before a pass: every band slot of a live frame at bits(i), and the front end's status words
 *                     copied to the pass's own (the coder reads PACX_ST_ZERO_SUBBLOCK there and raises its own bits
 *                     there: the handle's kept words stay as the front end left them).
 *   k_vq_band_store   after a pass: k_nmr's row into column i of the curve.  A band the coder dropped to 0 bits (all
 *                     its lines are zero: it codes nothing at any size) gets -inf, every band of a channel-frame the
 *                     pass flagged PACX_ST_VQ_UNDEFINED gets +inf; with i = 0 (Xh = 0: the row of a decode of zeros)
 *                     also the columns from n_cand on, +inf.  A dropped hop's rows are not written.
 *   k_vq_band_zero    cap_alloc as a unit coded with it comes out: 0 in the bands the coder dropped, in a dropped hop
 *                     and in the slots no band uses.
 *
 * One thread per band slot (per unit slot in k_vq_band_cap); plain vector loads and stores; every trip count is a
 * table's or an argument's.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"

using namespace pacx_k;

namespace {

constexpr int BAND_CAND = PACX_BAND_CAND;
constexpr int VQB_THREADS = 256;

/* the frame of a slot: its flags, and whether it is a short-coded hop the reference drops */
struct VqbFrame {
    bool is_short, dropped;
    unsigned fl;
};

__device__ __forceinline__ VqbFrame vqb_frame(const uint8_t *__restrict__ flags, int n_ch, long long cf,
                                              const uint32_t *__restrict__ status)
{
    VqbFrame f;
    const long long frame = cf / n_ch;
    f.fl = flags ? flags[frame] : 0u;
    f.is_short = (f.fl & 2u) != 0;
    unsigned st = 0;
    if (f.is_short)
        for (int c = 0; c < n_ch; ++c)
            st |= status[frame * n_ch + c];
    f.dropped = (st & PACX_ST_ZERO_SUBBLOCK) != 0;
    return f;
}

__global__ __launch_bounds__(VQB_THREADS) void k_vq_band_cap(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                             long long n_cf, double max_bps,
                                                             const uint32_t *__restrict__ status,
                                                             int32_t *__restrict__ cap, int32_t *__restrict__ budget)
{
    const long long at = (long long)blockIdx.x * VQB_THREADS + threadIdx.x;
    if (at >= n_cf * PACX_SUB)
        return;
    const long long cf = at / PACX_SUB;
    const int sb = (int)(at % PACX_SUB);
    const VqbFrame f = vqb_frame(flags, n_ch, cf, status);
    int v = -1;
    if (f.is_short ? !f.dropped : sb == 0)
        v = 32 * pacx_rate_steps(max_bps, f.is_short ? PACX_M_SHORT : PACX_M_LONG, f.is_short ? 1 : 0, (f.fl & 5u) != 0,
                                 T.n_scale_bits, T.n_mant_size_bits, f.is_short ? T.nb_short : T.nb_long);
    cap[at] = v;
    budget[at] = v < 0 ? 0 : v;
}

__global__ __launch_bounds__(VQB_THREADS) void k_vq_band_fill(PacxTables T, long long n_cf, int bits,
                                                              const uint32_t *__restrict__ status_in,
                                                              int32_t *__restrict__ alloc,
                                                              uint32_t *__restrict__ status_out)
{
    const long long at = (long long)blockIdx.x * VQB_THREADS + threadIdx.x;
    if (at >= n_cf * T.band_stride)
        return;
    alloc[at] = bits;                              /* the coder reads the slots of its frame's bands and no others */
    if (at < n_cf)
        status_out[at] = status_in[at];
}

__global__ __launch_bounds__(VQB_THREADS) void k_vq_band_store(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                               long long n_cf, int cand,
                                                               const double *__restrict__ row,
                                                               const int32_t *__restrict__ alloc,
                                                               const uint32_t *__restrict__ status_front,
                                                               const uint32_t *__restrict__ status_pass,
                                                               double *__restrict__ nmr)
{
    const long long at = (long long)blockIdx.x * VQB_THREADS + threadIdx.x;
    if (at >= n_cf * T.band_stride)
        return;
    const long long cf = at / T.band_stride;
    const int slot = (int)(at % T.band_stride);
    const VqbFrame f = vqb_frame(flags, n_ch, cf, status_front);
    if (f.dropped || slot >= (f.is_short ? PACX_SUB * T.nb_short : T.nb_long))
        return;                                    /* no band: not written, as k_band_curve leaves it */
    double v = row[at];
    if (alloc[at] == 0)
        v = -INFINITY;
    if (status_pass && (status_pass[cf] & PACX_ST_VQ_UNDEFINED))
        v = INFINITY;
    double *__restrict__ out = nmr + at * BAND_CAND;
    out[cand] = v;
    if (cand == 0) {
        int n_cand = 1 << T.n_mant_size_bits;
        if (n_cand > BAND_CAND)
            n_cand = BAND_CAND;
        for (int i = n_cand; i < BAND_CAND; ++i)
            out[i] = INFINITY;
    }
}

__global__ __launch_bounds__(VQB_THREADS) void k_vq_band_zero(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                              long long n_cf, const int32_t *__restrict__ alloc,
                                                              const uint32_t *__restrict__ status_front,
                                                              int32_t *__restrict__ cap_alloc)
{
    const long long at = (long long)blockIdx.x * VQB_THREADS + threadIdx.x;
    if (at >= n_cf * T.band_stride)
        return;
    const long long cf = at / T.band_stride;
    const int slot = (int)(at % T.band_stride);
    const VqbFrame f = vqb_frame(flags, n_ch, cf, status_front);
    if (f.dropped || slot >= (f.is_short ? PACX_SUB * T.nb_short : T.nb_long) || alloc[at] == 0)
        cap_alloc[at] = 0;
}

inline unsigned vqb_grid(long long n)
{
    return (unsigned)((n + VQB_THREADS - 1) / VQB_THREADS);
}

}  // namespace

void pacx_k::pacx_launch_vq_band_cap(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                     double max_bits_per_sample, const uint32_t *status, int32_t *cap, int32_t *budget,
                                     hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_vq_band_cap, dim3(vqb_grid(n_cf * PACX_SUB)), dim3(VQB_THREADS), 0, st, T, flags, n_ch, n_cf,
                       max_bits_per_sample, status, cap, budget);
}

void pacx_k::pacx_launch_vq_band_fill(const PacxTables &T, long long n_cf, int bits, const uint32_t *status_in,
                                      int32_t *alloc, uint32_t *status_out, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_vq_band_fill, dim3(vqb_grid(n_cf * T.band_stride)), dim3(VQB_THREADS), 0, st, T, n_cf, bits,
                       status_in, alloc, status_out);
}

void pacx_k::pacx_launch_vq_band_store(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, int cand,
                                       const double *row, const int32_t *alloc, const uint32_t *status_front,
                                       const uint32_t *status_pass, double *nmr, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_vq_band_store, dim3(vqb_grid(n_cf * T.band_stride)), dim3(VQB_THREADS), 0, st, T, flags, n_ch,
                       n_cf, cand, row, alloc, status_front, status_pass, nmr);
}

void pacx_k::pacx_launch_vq_band_zero(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                      const int32_t *alloc, const uint32_t *status_front, int32_t *cap_alloc,
                                      hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_vq_band_zero, dim3(vqb_grid(n_cf * T.band_stride)), dim3(VQB_THREADS), 0, st, T, flags, n_ch,
                       n_cf, alloc, status_front, cap_alloc);
}
