/*
 * mdct_dev.h -- the pieces of the long-block MDCT of int16 PCM that k_mdct_long_v2 (k_mdct2.hip),
 * k_mdct_long_x2p (k_mdct3.hip) and the transform inside k_front_long (k_psy.hip) are built from.
 * The encode path rests on the three giving THE SAME BITS for a frame (tests/test_gpu_parity.py,
 * tests/test_gpu_fused_front.py): every rounding operation of the fold, the post-twiddle, the scale
 * and the guard is written here once.  A kernel keeps what is its own: where window values and
 * twiddles come from (LDS tables or registers), how the PCM reaches LDS, how frames are interleaved,
 * its waits.  Everything is __forceinline__ and indexes register arrays by unrolled constants only
 * (wave_fft.h has the story of an array that went to scratch).
 *
 * One frame, one wave: lane L folds inputs n = L + 64 n1 into v[n1], runs fft512n (wave_fft.h),
 * and ends up holding y[L + 64 k3]; X[2k] = Re y[k] and X[2k+1] = -Im y[511-k] sit in mirrored
 * lanes, one 64-lane reversal pairs them so every store is a contiguous 16 bytes per lane.
 */
#ifndef PACX_MDCT_DEV_H
#define PACX_MDCT_DEV_H

#include "pacx_dev.h"
#include "wave_fft.h"

/* The window tables the fold multiplies by carry the PCM scale 2/65535 (coder/pcmfile.py:89-99
   mapping) and the MDCT's 2/N = 2^-10: the transform is linear, so the int16 codes go through it as
   exact integers and each product w'[i]*c carries one rounding.  Against the reference's order
   (round x = 2c/65535 first, then window) this moves a line by ~1e-16 of the block maximum, three
   orders below the 2e-13 that separates the two FFT algorithms. */
constexpr double MDCT_LONG_KSCALE = (2.0 / 65535.0) * (2.0 / PACX_N_LONG);

/* The four samples of fold input n (of N/4) of a block of N samples, k_mdct.hip's header has the
   formulas: re comes from i0, i1 and im from i2, i3.  n1 is the unrolled register index of n
   (n < N/8 exactly when n1 < 4), so the branch is resolved at compile time. */
template <int N>
__device__ __forceinline__ void mdct_fold_index(int n1, int n, int &i0, int &i1, int &i2, int &i3)
{
    constexpr int Q = N / 4, M = N / 2;
    if (n1 < 4) {
        i0 = 3 * Q - 1 - 2 * n; i1 = 3 * Q + 2 * n; i2 = Q - 1 - 2 * n; i3 = Q + 2 * n;
    } else {
        const int m = 2 * n - Q;
        i0 = m; i1 = M - 1 - m; i2 = 2 * Q + m; i3 = 4 * Q - 1 - m;
    }
}

/* symmetric (sine) window, w[N-1-i] = w[i]: two table values in the first half of the table serve
   the four samples, wa = w[ia] = w[i0] = w[i3] and wb = w[ib] = w[i1] = w[i2] */
__device__ __forceinline__ void mdct_fold_sym_index(int n1, int i0, int i1, int i2, int i3, int &ia, int &ib)
{
    ia = n1 < 4 ? i3 : i0;
    ib = n1 < 4 ? i2 : i1;
}

/* One fold element from its four window values and codes.  The operand order of every fma and the
   place of every negation decide the last bit of a line: they are the contract between the kernels. */
__device__ __forceinline__ cplx mdct_fold_any(int n1, double w0, double w1, double w2, double w3, double c0, double c1,
                                              double c2, double c3)
{
    if (n1 < 4)
        return make_double2(-fma(w1, c1, w0 * c0), fma(w2, c2, -(w3 * c3)));
    return make_double2(fma(w0, c0, -(w1 * c1)), -fma(w2, c2, w3 * c3));
}
__device__ __forceinline__ cplx mdct_fold_sym(int n1, double wa, double wb, double c0, double c1, double c2, double c3)
{
    return mdct_fold_any(n1, wa, wb, wb, wa, c0, c1, c2, c3);
}

/* The four codes of a fold element from the staged int16 samples, and the running minimum that
   tells whether the frame holds the code -32768.  WIDEN keeps the loaded codes opaque 32-bit
   values (sign-extending loads, no 16-bit narrowing of the minimum). */
template <bool WIDEN>
__device__ __forceinline__ void mdct_fold_codes(const short *raw, int i0, int i1, int i2, int i3, double &d0, double &d1,
                                                double &d2, double &d3, int &lowest)
{
    int c0 = raw[i0], c1 = raw[i1], c2 = raw[i2], c3 = raw[i3];
    if (WIDEN)
        asm("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    lowest = min(lowest, min(min(c0, c1), min(c2, c3)));
    d0 = (double)c0; d1 = (double)c1; d2 = (double)c2; d3 = (double)c3;
}

/* The reference maps the code -32768 to 0 (coder/pcmfile.py:93-97 masks the magnitude with 32767).
   Rather than test every sample, a fold tracks the minimum and, only for a frame that has one,
   calls this on the frame's 4 KB of staged codes (between two wave_lds_fence()) and folds again. */
__device__ __forceinline__ void mdct_zero_min_codes(unsigned *rw, int lane)
{
    for (int j = 0; j < 16; ++j) {
        unsigned x = rw[lane + 64 * j];
        if ((x & 0xFFFFu) == 0x8000u) x &= 0xFFFF0000u;
        if ((x >> 16) == 0x8000u) x &= 0x0000FFFFu;
        rw[lane + 64 * j] = x;
    }
}

/* post-twiddle of y[lane + 64 k3] by d(k3) = tw_long[lane + 64 k3], and the lane's maximum */
template <class D>
__device__ __forceinline__ void mdct_long_post(const cplx *v, D d_of_k3, double (&a)[8], double (&b)[8], double &mx)
{
    mx = 0.0;
#pragma unroll
    for (int k3 = 0; k3 < 8; ++k3) {
        const cplx d = d_of_k3(k3);
        a[k3] = fma(v[k3].x, d.x, -(v[k3].y * d.y));      /* Re y = X[2k], k = lane + 64 k3 */
        b[k3] = -fma(v[k3].x, d.y, v[k3].y * d.x);        /* -Im y = X[1023 - 2k]           */
        mx = fmax(mx, fmax(fabs(a[k3]), fabs(b[k3])));
    }
}

/* X[2k+1] = X[1023 - 2(511-k)] is held by lane 63-lane, register 7-k3 */
__device__ __forceinline__ void mdct_long_reverse(const double (&b)[8], int lane, double (&odd)[8])
{
#pragma unroll
    for (int k3 = 0; k3 < 8; ++k3)
        odd[k3] = __shfl(b[7 - k3], 63 - lane, 64);
}

/* Overall scale: ScaleFactor is non-increasing in its argument, so the scale of the block maximum
   is the minimum of the lanes' own scales s -- a few-bit integer, found by bisection with one ballot
   per bit while the lane reversal is in flight (a 64-bit max over the wave would be six dependent
   LDS round trips). */
__device__ __forceinline__ int mdct_long_scale(const PacxTables &T, double mx, int &s)
{
    s = pacx_scale_factor(mx, T.n_scale_bits, 5);
    int lo = 0;
    for (int bit = T.n_scale_bits - 1; bit >= 0; --bit)
        if (!__builtin_amdgcn_ballot_w64(s < lo + (1 << bit)))
            lo += 1 << bit;
    return lo;
}

/* PACX_ST_GUARD: the lanes that decide the minimum hold a maximum within a factor two of the
   block's; theirs sitting at a boundary of ScaleFactor flags the frame (line error bound relative
   to the block maximum, pacx_exact.h) */
__device__ __forceinline__ bool mdct_long_guard(const PacxTables &T, double mx, int s, int lo)
{
    return s == lo && pacx_scale_guard(mx, T.n_scale_bits, 5, 2.0 * PACX_GUARD_LINE_ERR * mx);
}

/* 16-byte line stores per epilogue (1024 lines = 64 lanes x 8 stores x 2 doubles).  The counted
   wait of k_mdct_long_x2p is derived from it; tests/test_build_isa.py reads this constant and
   checks the compiled code against it. */
constexpr int EPI_STORES = 8;

template <class CF>
__device__ __forceinline__ void mdct_long_store(double *__restrict__ lines, CF cf, int lane, const double (&a)[8],
                                                const double (&odd)[8])
{
    double2 *__restrict__ out = (double2 *)(lines + (long long)cf * PACX_M_LONG);
    static_assert(EPI_STORES * 64 * 2 == PACX_M_LONG, "one epilogue = EPI_STORES 16-byte stores per lane");
#pragma unroll
    for (int k3 = 0; k3 < EPI_STORES; ++k3)
        out[lane + 64 * k3] = make_double2(a[k3], odd[k3]);
}

/* Everything after the FFT: lines, the overall scale (when scale_out is given) and, when status is
   given and the handle asks for it, PACX_ST_GUARD -- stored by lane 0 after the zero it stored into
   the same word when it initialised the frame's outputs. */
template <class D, class CF>
__device__ __forceinline__ void mdct_long_epilogue(const PacxTables &T, const cplx *v, D d_of_k3, CF cf, int lane,
                                                   double *__restrict__ lines, int32_t *__restrict__ scale_out,
                                                   int scale_stride, uint32_t *__restrict__ status)
{
    double a[8], b[8], odd[8], mx;
    mdct_long_post(v, d_of_k3, a, b, mx);
    mdct_long_reverse(b, lane, odd);
    int lo = 0;
    bool guard = false;
    if (scale_out) {
        int s;
        lo = mdct_long_scale(T, mx, s);
        guard = T.guard && status && mdct_long_guard(T, mx, s, lo);
    }
    mdct_long_store(lines, cf, lane, a, odd);
    if (scale_out && lane == 0)
        scale_out[(long long)cf * scale_stride] = lo;
    if (__builtin_amdgcn_ballot_w64(guard) && lane == 0)
        status[cf] = 16u;
}

/* A workgroup's LDS copies of the tables: pre/post twiddle, the scaled sine window's first half, and
   the per-lane FFT twiddles w1[64 (k-1)] = W512^(lane k), w2[8 (k-1)] = W64^((lane & 7) k), k = 1..7,
   as fft512n takes them.  stage() is followed by the caller's __syncthreads(). */
struct MdctLongTables {
    cplx twl[512];
    double wsin[1024];
    cplx w64[7][8];
    cplx w1s[7][64];
    template <int THREADS>
    __device__ __forceinline__ void stage(const PacxTables &T, int tid)
    {
        for (int i = tid; i < 512; i += THREADS)
            twl[i] = T.tw_long[i];
        for (int i = tid; i < 1024; i += THREADS)
            wsin[i] = T.win_long[i] * MDCT_LONG_KSCALE;
        if (tid < 56)
            w64[tid >> 3][tid & 7] = T.w512[8 * (tid & 7) * ((tid >> 3) + 1)];
        for (int i = tid; i < 7 * 64; i += THREADS)
            w1s[i >> 6][i & 63] = T.w512[(i & 63) * ((i >> 6) + 1)];
    }
    __device__ __forceinline__ const cplx *w1(int lane) const { return &w1s[0][lane]; }
    __device__ __forceinline__ const cplx *w2(int lane) const { return &w64[0][lane & 7]; }
};

#endif
