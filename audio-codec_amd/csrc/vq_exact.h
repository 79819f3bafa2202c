/*
 * vq_exact.h -- the scalar rule that the gain-shape coder (k_vq.hip) and its decoder
 * (k_vq_dec.hip) evaluate at every node of a band's split tree, written once for device
 * (hipcc) and host (g++, tests/hostcheck) builds: the bits of the first field (a split's
 * angle, a band's gain), the angle's quantiser and dequantiser in 64- and in 32-bit integers,
 * the mid/side bit split, and the wide uniform quantiser of the mu-law gain.
 *
 * Coder and decoder agree on a stream only if every walker evaluates these expressions with
 * the same roundings (-ffp-contract=off, see pacx_exact.h); tests/test_host_exact.py holds them
 * against the oracle on the CPU.  No LDS, no kernels and no table pointers here: table values
 * are arguments, and each walker keeps its own way of fetching them.
 */
#ifndef PACX_VQ_EXACT_H
#define PACX_VQ_EXACT_H

#include "pacx_exact.h"

#define vq_half_pi 1.5707963267948966      /* np.pi / 2 */

/* gain_shape_alloc(bits, l)[0] (coder/gain_shape_quantize.py:57-62): what the first field takes,
   floor(bits / l + 0.5 log2(l)) -- a split's angle (l = its half) and a band's gain (l = its lines).
   The rest, max(bits - first, 0), stays with the caller. */
PACX_HD int vq_first_bits(int bits, int l, double half_log2_l)
{
    return (int)floor((double)bits / (double)l + half_log2_l);
}

/* QuantizeUniform(tn, a_theta) of tn = theta / (pi/2) >= 0 (coder/quantize.py:22-36) the way Python
   evaluates it: the factor 2^a - 1 becomes a float64 (exact up to 53 bits, 2^a beyond), one multiply,
   +1, floor-divide by 2.  1 <= a_theta <= 62. */
PACX_HD unsigned long long vq_angle_code(double tn, int a_theta)
{
    if (tn >= 1.0)
        return (1ull << (a_theta - 1)) - 1ull;
    const double factor = (a_theta <= 53) ? (double)((1ull << a_theta) - 1ull) : ldexp(1.0, a_theta);
    return (unsigned long long)floor((factor * tn + 1.0) * 0.5);
}

/* DequantizeUniform(code, a_theta) (coder/quantize.py:46-57) times pi/2: the angle both sides go on with */
PACX_HD double vq_angle_value(unsigned long long code, int a_theta)
{
    const unsigned long long mag = code & ((1ull << (a_theta - 1)) - 1ull);
    const double den = (a_theta <= 53) ? (double)((1ull << a_theta) - 1ull) : ldexp(1.0, a_theta);
    double dq = (double)(2ull * mag) / den;
    if (code >> (a_theta - 1))
        dq = -dq;
    return dq * vq_half_pi;
}

/* The same two values for 1 <= a_theta <= 31 in 32-bit integers: one conversion instruction on the
   device where the 64-bit ones take a dozen. */
PACX_HD unsigned vq_angle_code32(double tn, int a_theta)
{
    const double factor = (double)((1u << a_theta) - 1u);
    if (tn >= 1.0)
        return (1u << (a_theta - 1)) - 1u;
    return (unsigned)floor((factor * tn + 1.0) * 0.5);
}

PACX_HD double vq_angle_value32(unsigned code, int a_theta)
{
    const double den = (double)((1u << a_theta) - 1u);
    const unsigned mag = code & ((1u << (a_theta - 1)) - 1u);
    double dq = (double)(2u * mag) / den;
    if (code >> (a_theta - 1))
        dq = -dq;
    return dq * vq_half_pi;
}

/* log2(tan(theta_q) + eps) of the positive angles of up to PACX_VQ_THETA_TABLE_BITS bits is
   tabulated (pacx_config): whether a node's angle is in the table, and where */
PACX_HD bool vq_log2_tan_tabled(int a_theta, double theta_q)
{
    return a_theta <= PACX_VQ_THETA_TABLE_BITS && theta_q > 0.0;
}

PACX_HD int vq_log2_tan_slot(int a_theta, unsigned long long code)
{
    return ((1 << (a_theta - 1)) - 1) + (int)code;
}

/* bit_allocation_ms (coder/gain_shape_quantize.py:302-312) for theta_q != 0: the mid half's share of
   a_rest bits, lt = log2(tan(|theta_q|) + eps); the side half takes a_rest - mid.  theta_q == 0 (no
   bits for the mid half) is the caller's case. */
PACX_HD int vq_mid_bits(int a_rest, int half, double lt)
{
    const double v = ((double)a_rest - (double)(half - 1) * lt) / 2.0;
    const double f = floor(v);
    return (f < 0.0) ? 0 : ((f > (double)a_rest) ? a_rest : (int)f);
}

/* QuantizeUniform(x, n_bits) for x >= 0 and 1 <= n_bits <= 128, evaluated as vq_angle_code evaluates
   it: the code's two words (beyond 64 bits the float64 code is cut in two exactly). */
PACX_HD void vq_quantize_wide(double x, int n_bits, unsigned long long &hi, unsigned long long &lo)
{
    hi = 0;
    lo = 0;
    if (x >= 1.0) {                           /* code = 2^(n-1) - 1 */
        const int ones = n_bits - 1;
        if (ones >= 64) {
            lo = ~0ull;
            hi = (ones - 64 >= 64) ? ~0ull : ((1ull << (ones - 64)) - 1ull);
        } else {
            lo = (ones == 0) ? 0ull : ((~0ull) >> (64 - ones));
        }
    } else {
        const double factor = (n_bits <= 53) ? (double)((1ull << n_bits) - 1ull) : ldexp(1.0, n_bits);
        const double code = floor((factor * x + 1.0) * 0.5);
        if (n_bits <= 64) {
            lo = (unsigned long long)code;
        } else {
            const double top = floor(ldexp(code, -64));
            hi = (unsigned long long)top;
            lo = (unsigned long long)(code - ldexp(top, 64));
        }
    }
}

#endif
