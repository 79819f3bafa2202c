/*
 * pacx_exact.h -- the order-sensitive scalar arithmetic of the encode path,
 * written once for device (hipcc) and host (g++, tests/hostcheck) builds.
 *
 * Everything here must be compiled with -ffp-contract=off: the reference does
 * these steps as individually rounded IEEE double operations and the integer
 * codes only match bit for bit if the same roundings happen.
 */
#ifndef PACX_EXACT_H
#define PACX_EXACT_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PACX_HD __host__ __device__ __forceinline__
#else
#define PACX_HD static inline
#endif

#define PACX_MAX_BANDS 32          /* bands of one (sub-)block; 25 critical bands at most */
#define PACX_ALLOC_MAX_PASSES 200  /* coder/bitalloc.py:116-119                    */
#define PACX_DB_PER_BIT 6.2        /* coder/bitalloc.py:61                         */
#define PACX_EPS 2.220446049250313e-16 /* np.finfo(float).eps, coder/psychoac.py:20 */
#define PACX_VQ_SPLIT_BITS 32      /* coder/gain_shape_quantize.py:27              */
#define PACX_VQ_THETA_TABLE_BITS 12 /* split angles of up to this many bits: log2(tan) tabulated */

/* A0 -- coder/pcmfile.py:89-99 + coder/quantize.py:82-95:
 * value = +-(2*(|c| & 32767)) / 65535 with a correctly rounded division
 * (one multiply by RN(1/65535) plus one FMA residual step; checked over all
 * 65536 codes against the reference's own conversion in tests). */
PACX_HD double pacx_pcm16_to_f64(int c)
{
    const int neg = c < 0;
    const int mag = (neg ? -c : c) & 32767;
    const double n = (double)(2 * mag);
    const double inv = 1.0 / 65535.0;
    double q = n * inv;
    const double e = fma(-q, 65535.0, n);
    q = fma(e, inv, q);
    return neg ? -q : q;
}

/* A5/A12 -- magnitude code of the R-bit midtread quantiser for |x| = ax
 * (coder/quantize.py:29-32 scalar, :73-74 vector): clip at 1, else
 * floor(((2^R - 1)*ax + 1) / 2). */
PACX_HD int64_t pacx_quant_mag(double ax, int r_bits)
{
    if (ax >= 1.0)
        return ((int64_t)1 << (r_bits - 1)) - 1;
    const double t = (double)(((int64_t)1 << r_bits) - 1) * ax + 1.0;
    return (int64_t)floor(t * 0.5);
}

/* PACX_ST_GUARD -- how close a quantiser input sits to a decision boundary.
 * The code floor(t/2), t = (2^R - 1) ax + 1 (coder/quantize.py:73), changes where t crosses
 * an even integer (and at ax = 1, the clip).  This build's MDCT lines differ from the
 * reference's by the rounding noise of two different FFT factorisations: measured ~2e-13 of the
 * block maximum, and the lines are scaled so that this maximum is below 1.  A line is "near a
 * boundary" when t lies within (2^R - 1) * PACX_GUARD_LINE_ERR of one: its code could be the
 * neighbouring one in the reference's arithmetic.  (Not an error: the codes written are the
 * exact codes of THIS arithmetic; the flag marks frames a bit-exactness harness may want to
 * recompute on the CPU.) */
#define PACX_GUARD_LINE_ERR 5e-13       /* absolute, on lines scaled by 2^overallScale */
#define PACX_GUARD_ALLOC_ERR 1e-9       /* on Ropt - level (SMRs agree with the reference to 1e-9 dB) */

PACX_HD int pacx_quant_guard(double ax, int r_bits, double err)
{

    const double s = (double)(((int64_t)1 << r_bits) - 1);
    if (ax >= 1.0 - err)
        return ax <= 1.0 + err;                   /* at the clip (beyond it the code is constant) */
    const double half = (s * ax + 1.0) * 0.5;
    return fabs(half - rint(half)) * 2.0 <= s * err;
}

/* the same for ScaleFactor (coder/quantize.py:99-125): the leading-zero count of the magnitude
   code changes where the code crosses a power of two */
PACX_HD int pacx_scale_guard(double ax, int n_scale_bits, int n_mant_bits, double err)
{
    const int r_bits = (1 << n_scale_bits) - 1 + n_mant_bits;
    if (!pacx_quant_guard(ax, r_bits, err))
        return 0;
    const double s = (double)(((int64_t)1 << r_bits) - 1);
    const double half = (s * ax + 1.0) * 0.5;     /* near an integer n: does n have one bit set? */
    const int64_t n = (int64_t)rint(half);
    return ax >= 1.0 - err || (n > 0 && (n & (n - 1)) == 0);
}

PACX_HD int pacx_clz64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

/* A5 -- ScaleFactor(aNum, nScaleBits, nMantBits), coder/quantize.py:107-125:
 * zeros above the first set bit of the (R-1)-bit magnitude, capped. */
PACX_HD int pacx_scale_factor(double ax, int n_scale_bits, int n_mant_bits)
{
    const int r_bits = (1 << n_scale_bits) - 1 + n_mant_bits;
    const int64_t mag = pacx_quant_mag(ax, r_bits) & (((int64_t)1 << (r_bits - 1)) - 1);
    int zeros;
    if (mag == 0)
        zeros = r_bits - 1;
    else
        zeros = (r_bits - 2) - (63 - pacx_clz64((uint64_t)mag));
    const int cap = (1 << n_scale_bits) - 1;
    return zeros < cap ? zeros : cap;
}

/* A12 -- one block-floating-point mantissa, coder/quantize.py:238-250. */
PACX_HD int32_t pacx_mantissa(double x, int scale, int n_scale_bits, int n_mant_bits)
{
    const int r_bits = (1 << n_scale_bits) - 1 + n_mant_bits;
    const int64_t mag = pacx_quant_mag(fabs(x), r_bits);
    const int64_t keep = ((int64_t)1 << (n_mant_bits - 1)) - 1;
    const int64_t sign = (x < 0.0) ? ((int64_t)1 << (n_mant_bits - 1)) : 0;
    int64_t m;
    if (scale == (1 << n_scale_bits) - 1)
        m = mag & keep;
    else
        m = (mag >> (r_bits - scale - n_mant_bits)) & keep;
    return (int32_t)(sign + m);
}

/* Decode side of the quantisers (function-level mirrors and k_decode.hip).
 * vDequantizeUniform, coder/quantize.py:88-95: sign * 2 * code / (2^R - 1) -- integer product, then one
 * true division (the scalar DequantizeUniform, :46-57, divides Python ints, correctly rounded: the same
 * value while 2 * code and 2^R - 1 are exact doubles, R <= 53). */
PACX_HD double pacx_dequant_uniform(int64_t code_word, int r_bits)
{
    if (r_bits <= 0)
        return 0.0;
    const int64_t sign = (code_word & ((int64_t)1 << (r_bits - 1))) ? -1 : 1;
    const int64_t code = code_word & (((int64_t)1 << (r_bits - 1)) - 1);
    return (double)(sign * 2 * code) / (double)(((int64_t)1 << r_bits) - 1);
}

/* vDequantize / Dequantize, coder/quantize.py:260-274 (and :216-225): block-floating-point mantissa back to a
 * signed fraction -- sign to bit R-1, magnitude shifted up by R - scale - nMantBits, half a step added for a
 * non-zero magnitude unless the scale is the largest one. */
PACX_HD double pacx_dequantize(int64_t mant, int scale, int n_scale_bits, int n_mant_bits)
{
    const int r_bits = (1 << n_scale_bits) - 1 + n_mant_bits;
    const int64_t code = mant & (((int64_t)1 << (n_mant_bits - 1)) - 1);
    const int shift = r_bits - scale - n_mant_bits;
    int64_t a = (mant & ((int64_t)1 << (n_mant_bits - 1))) ? ((int64_t)1 << (r_bits - 1)) : 0;
    a += code << (shift > 0 ? shift : 0);
    if (scale < (1 << n_scale_bits) - 1 && code > 0)
        a += (int64_t)1 << (shift - 1);
    return pacx_dequant_uniform(a, r_bits);
}

/* MantissaFP / DequantizeFP, coder/quantize.py:130-175: the floating-point (not block-floating-point) pair of
 * the reference's quantiser module -- the leading one is implied, so one more bit of the magnitude is kept.  Not
 * used by the codec; mirrored so that a module swap of quantize.py and its self-test (:283-319) are complete. */
PACX_HD int32_t pacx_mantissa_fp(double x, int scale, int n_scale_bits, int n_mant_bits)
{
    const int r_bits = (1 << n_scale_bits) - 1 + n_mant_bits;
    const int64_t mag = pacx_quant_mag(fabs(x), r_bits);
    const int64_t keep = ((int64_t)1 << (n_mant_bits - 1)) - 1;
    const int64_t sign = (x < 0.0) ? ((int64_t)1 << (n_mant_bits - 1)) : 0;
    if (scale == (1 << n_scale_bits) - 1)
        return (int32_t)(sign + (mag & keep));
    return (int32_t)(sign + ((mag >> (r_bits - scale - n_mant_bits - 1)) & keep));
}

PACX_HD double pacx_dequantize_fp(int64_t mant, int scale, int n_scale_bits, int n_mant_bits)
{
    const int r_bits = (1 << n_scale_bits) - 1 + n_mant_bits;
    const int64_t code = mant & (((int64_t)1 << (n_mant_bits - 1)) - 1);
    int64_t a = (mant & ((int64_t)1 << (n_mant_bits - 1))) ? ((int64_t)1 << (r_bits - 1)) : 0;
    const int up = r_bits - scale - n_mant_bits - 1;
    a += code << (up > 0 ? up : 0);
    if (scale != (1 << n_scale_bits) - 1)
        a += (int64_t)1 << (r_bits - scale - 2);
    const int shift = r_bits - scale - n_mant_bits - 2;
    if (shift > 0)
        a += (int64_t)1 << shift;
    return pacx_dequant_uniform(a, r_bits);
}

/* np.sum of a contiguous float64 vector (NumPy pairwise_sum: plain loop below
 * 8 elements, else 8 running accumulators folded as ((0+1)+(2+3))+((4+5)+(6+7))
 * and a scalar tail; n <= 128 here so no recursive split). */
PACX_HD double pacx_np_sum(const double *a, int n)
{
    if (n < 8) {
        double r = -0.0;
        for (int i = 0; i < n; ++i)
            r = r + a[i];
        return r;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 = r0 + a[i + 0]; r1 = r1 + a[i + 1]; r2 = r2 + a[i + 2]; r3 = r3 + a[i + 3];
        r4 = r4 + a[i + 4]; r5 = r5 + a[i + 5]; r6 = r6 + a[i + 6]; r7 = r7 + a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i)
        res = res + a[i];
    return res;
}

/* np.add.reduce / np.sum / np.mean of a contiguous float64 vector of ANY length, in NumPy's order.  The reduction
 * hands pairwise_sum runs of at most np.getbufsize() = 8192 elements and adds their sums left to right onto the
 * identity 0.0; inside a run: up to 128 elements summed as pacx_np_sum sums them, longer runs cut at n/2
 * rounded down to a multiple of 8, the two halves summed and added.  The recursion runs on an explicit stack
 * that the caller supplies (the kernels keep it in LDS: a local array indexed at run time would go to scratch).
 * Element i is at(i), so the caller decides the layout.
 *
 * Stack depth: the larger half of a run of n is at most floor(n/2) + 8 elements, a bound that grows with n, so
 * iterating it from the longest run bounds the index of every entry pushed for any shorter run too.  Runs
 * never exceed PACX_NP_BUFSIZE, whatever the length of the vector. */
#define PACX_NP_BUFSIZE 8192               /* numpy's default ufunc buffer size (np.getbufsize()) */
#define PACX_NP_SUM_MAX_N 0x7fffffff       /* int element indices; pacx_transient_detect_f64's size limit */
#define PACX_PAIRWISE_STACK 8

struct PacxPairwiseStack {
    int lo[PACX_PAIRWISE_STACK], n[PACX_PAIRWISE_STACK], state[PACX_PAIRWISE_STACK];
    double left[PACX_PAIRWISE_STACK];
};

static constexpr int pacx_pairwise_depth_bound(long long n)
{
    int d = 0;
    while (n > 128) {
        n = n / 2 + 8;
        ++d;
    }
    return d;
}
static_assert(pacx_pairwise_depth_bound(PACX_NP_BUFSIZE) < PACX_PAIRWISE_STACK,
              "the pairwise-sum stack must hold the deepest split of the longest run");

/* numpy's pairwise_sum of elements lo .. lo + n_el - 1, n_el <= PACX_NP_BUFSIZE */
template <typename At>
PACX_HD double pacx_np_pairwise_sum(int lo0, int n_el, At at, PacxPairwiseStack *st)
{
    auto leaf = [&](int lo, int n) {
        if (n < 8) {
            double r = -0.0;
            for (int i = lo; i < lo + n; ++i)
                r = r + at(i);
            return r;
        }
        double r0 = at(lo), r1 = at(lo + 1), r2 = at(lo + 2), r3 = at(lo + 3);
        double r4 = at(lo + 4), r5 = at(lo + 5), r6 = at(lo + 6), r7 = at(lo + 7);
        const int n8 = n - (n & 7);
        for (int i = lo + 8; i < lo + n8; i += 8) {
            r0 = r0 + at(i + 0); r1 = r1 + at(i + 1); r2 = r2 + at(i + 2); r3 = r3 + at(i + 3);
            r4 = r4 + at(i + 4); r5 = r5 + at(i + 5); r6 = r6 + at(i + 6); r7 = r7 + at(i + 7);
        }
        double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (int i = lo + n8; i < lo + n; ++i)
            s = s + at(i);
        return s;
    };
    int top = 0;
    st->lo[0] = lo0;
    st->n[0] = n_el;
    st->state[0] = 0;
    double result = 0.0;
    while (top >= 0) {
        const int lo = st->lo[top], n = st->n[top], state = st->state[top];
        int cut = n / 2;
        cut -= cut % 8;
        if (n <= 128) {
            result = leaf(lo, n);
            --top;
        } else if (state == 0) {
            st->state[top] = 1;
            ++top;
            st->lo[top] = lo;
            st->n[top] = cut;
            st->state[top] = 0;
        } else if (state == 1) {
            st->left[top] = result;
            st->state[top] = 2;
            ++top;
            st->lo[top] = lo + cut;
            st->n[top] = n - cut;
            st->state[top] = 0;
        } else {
            result = st->left[top] + result;
            --top;
        }
    }
    return result;
}

template <typename At>
PACX_HD double pacx_np_add_reduce(int n_el, At at, PacxPairwiseStack *st)
{
    double r = 0.0;
    for (int done = 0; done < n_el;) {
        const int n = n_el - done < PACX_NP_BUFSIZE ? n_el - done : PACX_NP_BUFSIZE;
        r = r + pacx_np_pairwise_sum(done, n, at, st);
        done += n;
    }
    return r;
}

/* Budget rule of coder/codec.py:288-299.  use_vq: only the overall scale
 * factor is charged (:292-294).  sbr_long: a long block of an SBR file is
 * budgeted from the full halfN whatever its flags (EncodeSingleChannel_SBR,
 * coder/codec.py:446-453). */
PACX_HD double pacx_bit_budget(double target_bits_per_sample, int half_n, int is_short,
                               int last_or_next, int n_scale_bits, int n_mant_size_bits,
                               int n_bands, int use_vq, int sbr_long)
{
    int n_eff = is_short ? (int)(1.45 * half_n) : half_n;
    if (last_or_next && !sbr_long)
        n_eff = (int)(0.85 * n_eff);
    double budget = target_bits_per_sample * (double)n_eff;
    if (use_vq)
        budget = budget - (double)n_scale_bits;
    else
        budget = budget - (double)(n_scale_bits * (n_bands + 1));
    budget = budget - (double)(n_mant_size_bits * n_bands);
    return budget;
}

/* J of a unit of the rate search and the rate curve (include/pacx.h): the scalar budget rule with the cap rate, in
 * steps of PACX_RATE_STEP = 32 bits. */
PACX_HD int pacx_rate_steps(double max_bits_per_sample, int half_n, int is_short, int last_or_next, int n_scale_bits,
                            int n_mant_size_bits, int n_bands)
{
    const double cap = pacx_bit_budget(max_bits_per_sample, half_n, is_short, last_or_next, n_scale_bits,
                                       n_mant_size_bits, n_bands, 0, 0);
    const double jf = floor(cap / 32.0);
    return jf > 0.0 ? (jf < 2047.0 ? (int)jf : 2047) : 0;
}

/* A11 -- BitAlloc, coder/bitalloc.py:77-121.  Returns the number of passes;
 * *hit_cap is set when the loop left through its 200-pass guard. */
PACX_HD int pacx_bit_alloc(double budget, int max_mant_bits, int n_bands,
                           const int32_t *n_lines, const double *smr,
                           int32_t *bits, int *hit_cap)
{
    unsigned dropped = 0;          /* bit b set: band b flagged (gets no bits) */
    int n_flip = 0;
    int passes = 0;
    if (max_mant_bits > 16)
        max_mant_bits = 16;
    for (int b = 0; b < n_bands; ++b)
        bits[b] = 0;
    *hit_cap = 0;
    for (;;) {
        double prod[PACX_MAX_BANDS];
        double want[PACX_MAX_BANDS];
        double ladder[PACX_MAX_BANDS];
        int idx[PACX_MAX_BANDS];
        int nv = 0;
        int64_t total_i = 0;
        for (int b = 0; b < n_bands; ++b) {
            if (!((dropped >> b) & 1u)) {
                idx[nv] = b;
                prod[nv] = (double)n_lines[b] * smr[b];
                total_i += n_lines[b];
                ++nv;
            }
        }
        double total = (double)total_i;
        if (total_i == 0)
            total = total + 1e-12;
        const double mean = pacx_np_sum(prod, nv) / total;
        const double base = budget / total;
        const double per_db = 1.0 / PACX_DB_PER_BIT;
        int nd = 0;
        for (int i = 0; i < nv; ++i) {
            want[i] = base + per_db * (smr[idx[i]] - mean);
            const double frac = (want[i] - floor(want[i])) - 0.5;
            if (frac > 0.0) {              /* insertion into the ascending ladder */
                int j = nd++;
                while (j > 0 && ladder[j - 1] > frac) {
                    ladder[j] = ladder[j - 1];
                    --j;
                }
                ladder[j] = frac;
            }
        }
        if (n_flip > nd) {
            n_flip -= 1;                   /* bits keep their previous values */
        } else {
            const double level = (n_flip == 0) ? 0.0 : ladder[n_flip - 1];
            for (int i = 0; i < nv; ++i)
                bits[idx[i]] = (int32_t)rint(want[i] - level);   /* np.round: half to even */
        }
        unsigned now_dropped = 0;
        int64_t spent = 0;
        for (int b = 0; b < n_bands; ++b) {
            if (bits[b] > max_mant_bits)
                bits[b] = max_mant_bits;
            if (bits[b] < 2) {
                now_dropped |= 1u << b;
                bits[b] = 0;
            }
            spent += (int64_t)bits[b] * n_lines[b];
        }
        const int stable = (now_dropped == dropped);
        dropped = now_dropped;
        if (stable && (double)spent <= budget)
            break;
        if (stable && (double)spent > budget)
            n_flip += 1;
        ++passes;
        if (passes > PACX_ALLOC_MAX_PASSES) {
            *hit_cap = 1;
            break;
        }
    }
    return passes;
}

/* log10 of a positive normal double, for the mask kernel's per-line SPL (its argument is
 * 4 v^2 + eps with |v| < 8).  The classic argument reduction x = 2^k (1 + f),
 * sqrt(1/2) < 1 + f < sqrt(2), s = f / (2 + f), a degree-14 odd series in s, and the
 * head/tail assembly of k log10(2) + log(1 + f) / ln(10) (as in the BSD libm's log10);
 * error below one ulp.  A third of the instructions of the device library's log10,
 * which carries the whole evaluation in double-double -- and this kernel is bound by
 * VALU issue.  NumPy's own log10 is the host libm's (< 1-2 ulp, platform dependent), so
 * the reference's value is defined to that precision only; the integer codes, checked
 * against the reference's .pac files, do not depend on the last bit here. */
PACX_HD double pacx_log10_pos(double x)
{
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const double ivln10hi = 4.34294481878168880939e-01, ivln10lo = 2.50829467116452752298e-11,
                 log10_2hi = 3.01029995663611771306e-01, log10_2lo = 3.69423907715893078616e-13;
    uint64_t bits;
    memcpy(&bits, &x, 8);
    int hx = (int)(bits >> 32);
    int k = (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int i = (hx + 0x95f64) & 0x100000;                 /* mantissa >= sqrt(2): use x/2 */
    bits = ((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xFFFFFFFFull);
    memcpy(&x, &bits, 8);
    k += i >> 20;
    const double f = x - 1.0, dk = (double)k;
    const double hfsq = (0.5 * f) * f;
    /* s = f / (2 + f): reciprocal refined twice, then one correction of the quotient */
    const double d = 2.0 + f;
#if defined(__HIP_DEVICE_COMPILE__)
    double rc = __builtin_amdgcn_rcp(d);
#else
    double rc = 1.0 / d;
#endif
    rc = fma(fma(-d, rc, 1.0), rc, rc);
    rc = fma(fma(-d, rc, 1.0), rc, rc);
    double sq = f * rc;
    sq = fma(fma(-d, sq, f), rc, sq);
    const double z = sq * sq, w = z * z;
    /* Horner steps with the addend in scalar registers (three-address v_fma_f64): from a
       vector register the compiler takes the two-address v_fmac_f64 and copies the constant
       into the accumulator first, every step of every line */
#if defined(__HIP_DEVICE_COMPILE__)
#define PACX_FMA_SC(r, a, b, c) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c))
#else
#define PACX_FMA_SC(r, a, b, c) (r) = fma((a), (b), (c))
#endif
    double h1, h2;
    PACX_FMA_SC(h1, w, Lg6, Lg4);
    PACX_FMA_SC(h1, w, h1, Lg2);
    PACX_FMA_SC(h2, w, Lg7, Lg5);
    PACX_FMA_SC(h2, w, h2, Lg3);
    PACX_FMA_SC(h2, w, h2, Lg1);
#undef PACX_FMA_SC
    const double t1 = w * h1;
    const double t2 = z * h2;
    const double r = sq * (hfsq + (t2 + t1));
    double hi = f - hfsq;
    memcpy(&bits, &hi, 8);
    bits &= 0xFFFFFFFF00000000ull;
    memcpy(&hi, &bits, 8);
    const double lo = ((f - hi) - hfsq) + r;
    double val_hi = hi * ivln10hi;
    const double y2 = dk * log10_2hi;
    double val_lo = fma(dk, log10_2lo, fma(lo + hi, ivln10lo, lo * ivln10hi));
    const double wv = y2 + val_hi;
    val_lo += (y2 - wv) + val_hi;
    return val_lo + wv;
}

/* coder/psychoac.py:10-25, array flavour: exact zero -> 1e-8, floor at -30. */
PACX_HD double pacx_spl_array(double intensity)
{
    if (intensity == 0.0)
        intensity = 1e-8;
    double spl = 96.0 + 10.0 * log10(fabs(intensity) + PACX_EPS);
    if (spl < -30.0)
        spl = -30.0;
    return spl;
}

/* SPL(Intensity(x)) -- the round trip the reference applies to every masker
 * curve (coder/psychoac.py:96 then :192): 96 + 10 log10(10^((x-96)/10) + eps),
 * floored at -30.  Algebraically x + (10/ln 10) log1p(t) with
 * t = eps * 10^((96-x)/10); t < 1e-3 whenever the result is above the floor
 * (t >= 1e-3 means the intensity is <= 2.2e-13, i.e. SPL <= -30.57 + 0.004), so
 * a 5-term log1p series is exact to double rounding and one exp2 replaces
 * pow + log10.  Differs from the reference's own evaluation by rounding noise
 * only (~1e-14 dB); the threshold is compared at 1e-9 dB in the tests. */
/* 2^y to a relative 3e-13, for the round trip below (which needs t = eps 2^y to ~1e-11 only:
 * t < 1e-3 enters the result as 4.34 log1p(t) dB).  y = n + f, |f| <= 1/2, degree-10 series
 * of 2^f in Horner form with the coefficients as scalar-register operands, 2^n by ldexp:
 * 16 instructions against 39 for the device library's exp2 -- inside the mask kernel's
 * per-line loop, sixteen lines per lane and frame. */
PACX_HD double pacx_exp2_lean(double y)
{
    const double n = rint(y), f = y - n;
    const double c1 = 6.931471805599453094e-01, c2 = 2.402265069591007123e-01, c3 = 5.550410866482157995e-02,
                 c4 = 9.618129107628477162e-03, c5 = 1.333355814642844343e-03, c6 = 1.540353039338160995e-04,
                 c7 = 1.525273380405984028e-05, c8 = 1.321548679014430949e-06, c9 = 1.017808600923969973e-07,
                 c10 = 7.054911620801123330e-09;
#if defined(__HIP_DEVICE_COMPILE__)
#define PACX_FMA_SC(r, a, b, c) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c))
#else
#define PACX_FMA_SC(r, a, b, c) (r) = fma((a), (b), (c))
#endif
    double p;
    PACX_FMA_SC(p, f, c10, c9);
    PACX_FMA_SC(p, f, p, c8);
    PACX_FMA_SC(p, f, p, c7);
    PACX_FMA_SC(p, f, p, c6);
    PACX_FMA_SC(p, f, p, c5);
    PACX_FMA_SC(p, f, p, c4);
    PACX_FMA_SC(p, f, p, c3);
    PACX_FMA_SC(p, f, p, c2);
    PACX_FMA_SC(p, f, p, c1);
#undef PACX_FMA_SC
    p = fma(f, p, 1.0);
    int e = (int)n;                                  /* |y| < 1100 here; ldexp saturates beyond */
    return ldexp(p, e);
}

PACX_HD double pacx_spl_of_intensity_of(double x)
{
    double y = (96.0 - x) * 0.33219280948873623;     /* log2(10)/10 */
    if (y > 1000.0)
        y = 1000.0;                                  /* t is far above 1e-3 long before: the floor */
    const double t = PACX_EPS * pacx_exp2_lean(y);
    if (!(t < 1e-3))
        return -30.0;
    const double p = t * (1.0 + t * (-0.5 + t * (1.0 / 3.0 + t * (-0.25 + t * 0.2))));
    const double r = x + 4.3429448190325182765 * p;                       /* 10/ln(10) */
    return r < -30.0 ? -30.0 : r;
}

/* coder/psychoac.py:10-25, scalar flavour: exact zero -> -30. */
PACX_HD double pacx_spl_scalar(double intensity)
{
    if (intensity == 0.0)
        return -30.0;
    double spl = 96.0 + 10.0 * log10(fabs(intensity) + PACX_EPS);
    if (spl < -30.0)
        spl = -30.0;
    return spl;
}

/* coder/psychoac.py:45-46 */
PACX_HD double pacx_bark(double f)
{
    const double t = f / 7500.0;
    return 13.0 * atan(0.76 * f / 1000.0) + 3.5 * atan(t * t);
}

/* coder/psychoac.py:37-40 */
PACX_HD double pacx_thresh_quiet(double f)
{
    if (f < 10.0)
        f = 10.0;
    const double k = f / 1000.0;
    const double d = k - 3.3;
    return 3.64 * pow(k, -0.8) - 6.5 * exp(-0.6 * (d * d)) + 0.001 * (k * k * k * k);
}

/* codec.getCorrectWindow, coder/codec.py:30-44 */
PACX_HD int pacx_window_kind(unsigned flags)
{
    const int last_t = flags & 1u, cur_t = (flags >> 1) & 1u, next_t = (flags >> 2) & 1u;
    if (cur_t) return 0;
    if (last_t && next_t) return 3;
    if (last_t) return 2;
    if (next_t) return 1;
    return 0;
}

#endif /* PACX_EXACT_H */
