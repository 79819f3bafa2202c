/*
 * k_nmr.hip -- noise-to-mask ratios of coded blocks (pacx_nmr_batch / pacx_nmr_summary, include/pacx.h).
 *
 *   k_nmr          one wave per channel-frame: n[k] = 4 (X[k] - Xh[k])^2 and m[k] = 10^((T[k] - 96) / 10) per
 *                  line, their means per band, NMR_b = 10 log10((N_b + eps) / M_b).  Reads 24 KB per
 *                  channel-frame (original lines, decoded lines, threshold) once, coalesced; writes
 *                  3 x band_stride doubles.  The per-line values pass through 16 KB of LDS so that every band
 *                  (a run of lines) is summed by the whole wave: lanes stride over the run, then a butterfly
 *                  of wave shuffles -- a fixed order, so the sums are the same bits on every run.
 *   k_nmr_summary  counts, counts above 0 dB, maximum and a 0.5 dB histogram per band index, long blocks and
 *                  short sub-blocks apart: a workgroup takes one band index and a stripe of the batch, gathers in
 *                  LDS with integer atomics and adds what it found to the caller's summary with integer atomics.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "pacx_launch.h"

using namespace pacx_k;

namespace {

constexpr int NMR_PER = PACX_M_LONG / 64;          /* lines per lane */
constexpr unsigned NMR_NO_PAYLOAD = 2u | 8u | 32u | 64u;   /* PACX_ST_ZERO_SUBBLOCK, _VQ_UNDEFINED, _MALFORMED, _REF_RAISES */

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_nmr(PacxTables T, const uint8_t *__restrict__ flags, int n_ch, long long n_cf,
                                            const double *__restrict__ lines, const double *__restrict__ dec_lines,
                                            const int32_t *__restrict__ overall, const double *__restrict__ thr,
                                            const uint32_t *__restrict__ status, double *__restrict__ noise,
                                            double *__restrict__ mask, double *__restrict__ nmr_db)
{
    __shared__ double n_l[PACX_M_LONG];
    __shared__ double m_l[PACX_M_LONG];
    const int lane = threadIdx.x;
    const long long cf = blockIdx.x;
    if (cf >= n_cf)
        return;
    const int stride = T.band_stride;
    double *__restrict__ o_n = noise + cf * stride;
    double *__restrict__ o_m = mask + cf * stride;
    double *__restrict__ o_r = nmr_db + cf * stride;
    const bool is_short = flags && (flags[cf / n_ch] & 2u);
    const int nb = is_short ? T.nb_short : T.nb_long;
    const int n_units = is_short ? PACX_SUB * nb : nb;
    /* slots no band uses, and every slot of a frame without a payload */
    const bool dead = status && (status[cf] & NMR_NO_PAYLOAD);
    for (int u = (dead ? 0 : n_units) + lane; u < stride; u += 64) {
        o_n[u] = NAN;
        o_m[u] = NAN;
        o_r[u] = NAN;
    }
    if (dead)
        return;

    const long long loff = cf * PACX_M_LONG;
    double x[NMR_PER], d[NMR_PER], t[NMR_PER];
#pragma unroll
    for (int j = 0; j < NMR_PER; ++j) {
        x[j] = lines[loff + lane + 64 * j];
        d[j] = dec_lines[loff + lane + 64 * j];
        t[j] = thr[loff + lane + 64 * j];
    }
    /* 2^-overallScale: line lane + 64 j of a short frame belongs to sub-block j / 2 */
    const int32_t *__restrict__ ov = overall + cf * PACX_SUB;
    const double inv_long = ldexp(1.0, -ov[0]);
#pragma unroll
    for (int j = 0; j < NMR_PER; ++j) {
        const double inv = is_short ? ldexp(1.0, -ov[j >> 1]) : inv_long;
        const double e = x[j] - d[j] * inv;                  /* a power of two: exact, as the decoder's division */
        n_l[lane + 64 * j] = (e * e) * 4.0;
        /* 10^y by exp2(y log2 10): relative error below 1e-14 for |y| < 20, far inside what the measure resolves */
        m_l[lane + 64 * j] = exp2(((t[j] - 96.0) / 10.0) * 3.32192809488736234787);
    }
    __syncthreads();                                         /* one wave per workgroup */

    const int32_t *__restrict__ lower = is_short ? T.band_lower_short : T.band_lower_long;
    const int32_t *__restrict__ count = is_short ? T.band_lines_short : T.band_lines_long;
    const int m_block = is_short ? PACX_M_SHORT : PACX_M_LONG;
    for (int u = 0; u < n_units; ++u) {
        const int sb = u / nb, b = u - sb * nb;
        const int lo = sb * PACX_M_SHORT + lower[b];
        int cnt = count[b];
        if (lower[b] + cnt > m_block)                        /* a table that runs past the block (build_bands refuses it) */
            cnt = m_block - lower[b];
        double sn = 0.0, sm = 0.0;
        for (int k = lane; k < cnt; k += 64) {
            sn += n_l[lo + k];
            sm += m_l[lo + k];
        }
        sn = wave_sum(sn);
        sm = wave_sum(sm);
        if (lane == 0) {
            const double nn = sn / (double)cnt, mm = sm / (double)cnt;
            o_n[u] = nn;
            o_m[u] = mm;
            o_r[u] = 10.0 * log10((nn + PACX_EPS) / mm);
        }
    }
}

constexpr int SUM_WORDS = PACX_NMR_SUMMARY_WORDS;
constexpr int SUM_THREADS = 256;
constexpr int SUM_STRIPES = 64;                    /* workgroups per band index */

/* unsigned order = numeric order; no double maps to 0 */
__device__ __forceinline__ unsigned long long order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(SUM_THREADS) void k_nmr_summary(PacxTables T, const uint8_t *__restrict__ flags, int n_ch,
                                                             long long n_cf, const double *__restrict__ nmr_db,
                                                             unsigned long long *__restrict__ summary)
{
    __shared__ unsigned int hist[SUM_WORDS];                /* [PACX_NMR_MAX] unused here */
    __shared__ unsigned long long best;
    const int kind = blockIdx.y / PACX_NMR_MAX_BANDS, b = blockIdx.y % PACX_NMR_MAX_BANDS;
    const int nb = kind ? T.nb_short : T.nb_long;
    if (b >= nb)
        return;
    for (int i = threadIdx.x; i < SUM_WORDS; i += SUM_THREADS)
        hist[i] = 0u;
    if (threadIdx.x == 0)
        best = 0ull;
    __syncthreads();
    /* a launch holds fewer than 2^31 values (pacx_nmr_summary bounds n_cf), so the 32-bit LDS counters cannot wrap */
    const int per = kind ? PACX_SUB : 1;
    const long long n_vals = n_cf * per;
    unsigned long long mine = 0ull;
    for (long long i = (long long)blockIdx.x * SUM_THREADS + threadIdx.x; i < n_vals;
         i += (long long)gridDim.x * SUM_THREADS) {
        const long long cf = i / per;
        const int sb = (int)(i - cf * per);
        const bool is_short = flags && (flags[cf / n_ch] & 2u);
        if (is_short != (kind != 0))
            continue;
        const double v = nmr_db[cf * T.band_stride + sb * nb + b];
        if (v != v)
            continue;
        const double pos = floor((v - PACX_NMR_HIST_LO) / PACX_NMR_HIST_STEP);
        const int bin = pos < 0.0 ? 0 : (pos >= (double)PACX_NMR_HIST_BINS ? PACX_NMR_HIST_BINS + 1 : 1 + (int)pos);
        atomicAdd(&hist[PACX_NMR_HIST + bin], 1u);
        atomicAdd(&hist[PACX_NMR_COUNT], 1u);
        if (v > 0.0)
            atomicAdd(&hist[PACX_NMR_AUDIBLE], 1u);
        const unsigned long long key = order_key(v);
        mine = key > mine ? key : mine;
    }
    if (mine)
        atomicMax(&best, mine);
    __syncthreads();
    unsigned long long *__restrict__ out = summary + ((size_t)kind * PACX_NMR_MAX_BANDS + b) * SUM_WORDS;
    for (int i = threadIdx.x; i < SUM_WORDS; i += SUM_THREADS) {
        if (i == PACX_NMR_MAX) {
            if (best)
                atomicMax(&out[i], best);
        } else if (hist[i]) {
            atomicAdd(&out[i], (unsigned long long)hist[i]);
        }
    }
}

}  // namespace

void pacx_k::pacx_launch_nmr(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, const double *lines,
                             const double *dec_lines, const int32_t *overall, const double *thr, const uint32_t *status,
                             double *noise, double *mask, double *nmr_db, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    hipLaunchKernelGGL(k_nmr, dim3((unsigned)n_cf), dim3(64), 0, st, T, flags, n_ch, n_cf, lines, dec_lines, overall, thr,
                       status, noise, mask, nmr_db);
}

void pacx_k::pacx_launch_nmr_summary(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                     const double *nmr_db, unsigned long long *summary, hipStream_t st)
{
    if (n_cf <= 0)
        return;
    long long stripes = (n_cf * PACX_SUB + SUM_THREADS - 1) / SUM_THREADS;
    if (stripes > SUM_STRIPES)
        stripes = SUM_STRIPES;
    hipLaunchKernelGGL(k_nmr_summary, dim3((unsigned)stripes, 2 * PACX_NMR_MAX_BANDS), dim3(SUM_THREADS), 0, st, T, flags,
                       n_ch, n_cf, nmr_db, summary);
}
