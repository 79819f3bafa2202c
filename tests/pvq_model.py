"""Exact pyramid-VQ arithmetic that does not walk K: the reference for leaves the oracle cannot reach.

oracle.pac_oracle_vq restates the reference's codebook layer as the reference wrote it: `codebook_size` grows rows of
N(l, k) one k at a time, `pulses_for_bits` counts K up from 1 and `pvq_decode` tries the magnitudes of a component one
after the other -- all linear in K.  A 2-line leaf with 32 bits has K = 2^30, leaves of 3 and 4 lines reach K of some
10^4 and 10^3; the oracle does not get there.  This module computes the same quantities in closed form and by
bisection, in Python integers only (no floats, no NumPy), so that nothing in it can overflow or round:

    n_vectors(l, k)          N(l, k) = sum_i 2^i C(l, i) C(k-1, i-1)       (i non-zero components: their places, their
                             signs, k pulses split into i positive parts); 1 at k = 0
    n_up_to(l, k)            P(l, k) = sum_{j <= k} N(l, j) = 1 + sum_i 2^i C(l, i) C(k, i)
    pulses_for_bits(l, bits) the largest K with N(l, K) <= 2^bits and the index width ceil(log2(N + eps)): 1 at K = 0
    pvq_decode(b, l, k)      index -> vector, the reference's five-step machine with the magnitude found by bisection
    pvq_index(y, k)          vector -> index, its inverse

tests/test_pvq_model.py pins every function to the oracle wherever the oracle is usable.  CPU only, no tests here.
"""
import functools
from math import comb


@functools.lru_cache(maxsize=None)
def n_vectors(l, k):
    """N(l, k): integer vectors of l components with sum |y_i| = k.  N(l, 0) = 1, N(0, k >= 1) = 0, 0 for k < 0."""
    if k < 0:
        return 0
    if k == 0:
        return 1
    return sum((1 << i) * comb(l, i) * comb(k - 1, i - 1) for i in range(1, min(l, k) + 1))


@functools.lru_cache(maxsize=None)
def n_up_to(l, k):
    """P(l, k) = N(l, 0) + ... + N(l, k) (sum_{j=1..k} C(j-1, i-1) = C(k, i)); 0 for k < 0."""
    if k < 0:
        return 0
    return 1 + sum((1 << i) * comb(l, i) * comb(k, i) for i in range(1, min(l, k) + 1))


def index_width(n):
    """ceil(log2(n + eps)) of the reference's width rule, for an integer n >= 1: a codebook of ONE vector (K = 0) still
    takes a bit, log2(1 + eps) being a little above 0"""
    return 1 if n == 1 else (n - 1).bit_length()


@functools.lru_cache(maxsize=None)
def pulses_for_bits(l, bits):
    """-> (K, width): the largest K with N(l, K) <= 2^bits, by bisection (N grows with K for l >= 2, and
    N(l, K) >= 4 K there, so K < 2^bits), and the width of an index of that codebook.  l = 1 has N = 2 for every
    K >= 1: the reference's count never ends, and this raises."""
    if l < 2:
        raise ValueError("N(1, k) = 2 for every k: no largest K")
    cap = 1 << bits
    lo, hi = 0, cap                                      # N(l, lo) <= cap < N(l, hi)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if n_vectors(l, mid) <= cap:
            lo = mid
        else:
            hi = mid
    return lo, index_width(n_vectors(l, lo))


def _pairs_below(l, k, j):
    """vectors of l + 1 components and k pulses whose first component has magnitude 1..j, either sign:
    sum_{m=1..j} 2 N(l, k - m)"""
    return 2 * (n_up_to(l, k - 1) - n_up_to(l, k - j - 1))


def pvq_decode(b, l_total, k_total):
    """Index -> vector (list of ints), oracle.pac_oracle_vq.pvq_decode's machine.  At component i with l components
    and k pulses left and xb the first index of the vectors that share the components so far:
      b == xb                     the walk ends: the LAST component takes the k pulses left, positive (step 1 -> 5);
      b <  xb + N(l-1, k)         this component is zero (step 2);
      else                        xb skips those, and the magnitude j is the first whose two sign groups reach past b
                                  (step 3; the reference tries j = 1, 2, ...; here j is bisected on P(l-1, .)).  The
                                  positive group of j comes first.  For a negative component the reference leaves xb at
                                  the positive group, walks through all of it at the next component and restarts that
                                  component at the negative group; adding N(l-1, k-j) to xb at once is the same walk.
    An index that is no member of the codebook (b >= N(l_total, k_total)) raises ValueError."""
    if not 0 <= b < n_vectors(l_total, k_total):
        raise ValueError(f"index {b} outside the codebook N({l_total}, {k_total})")
    y = [0] * l_total
    xb, k, l = 0, k_total, l_total
    for i in range(l_total):
        if k == 0:
            break
        if b == xb:
            y[l_total - 1] = k
            k = 0
            break
        zero = n_vectors(l - 1, k)
        if b - xb >= zero:
            xb += zero
            r = b - xb
            lo, hi = 1, k                                # smallest j with r < _pairs_below(l - 1, k, j)
            while lo < hi:
                mid = (lo + hi) >> 1
                if r < _pairs_below(l - 1, k, mid):
                    hi = mid
                else:
                    lo = mid + 1
            j = lo
            assert r < _pairs_below(l - 1, k, j)
            xb += _pairs_below(l - 1, k, j - 1)
            group = n_vectors(l - 1, k - j)
            if b - xb >= group:
                y[i] = -j
                xb += group
            else:
                y[i] = j
            k -= j
        l -= 1
    assert k == 0
    return y


def pvq_index(y, k_total=None):
    """Vector -> index (oracle.pac_oracle_vq.pvq_index with its inner sum over magnitudes in closed form)."""
    if k_total is None:
        k_total = sum(abs(int(v)) for v in y)
    assert sum(abs(int(v)) for v in y) == k_total
    b, k, l = 0, k_total, len(y)
    for v in y:
        a = abs(int(v))
        if a:
            b += n_vectors(l - 1, k) + _pairs_below(l - 1, k, a - 1)
            if v < 0:
                b += n_vectors(l - 1, k - a)
        k -= a
        l -= 1
        if k == 0:
            break
    return b
