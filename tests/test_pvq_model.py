"""tests/pvq_model.py against the oracle's codebook layer wherever the oracle is usable (its functions are linear in
K), and against itself beyond: the model is the reference for 2-, 3- and 4-line leaves with the largest K their 32 bits
allow, which tests/vq_code_streams.py draws and the GPU decoders have to decode."""
import numpy as np
import pytest

import pvq_model as pm
from oracle import pac_oracle_vq as pv


def test_sizes_and_running_sums():
    for l in range(0, 12):
        run = 0
        for k in range(0, 40):
            assert pm.n_vectors(l, k) == pv.codebook_size(l, k), (l, k)
            run += pm.n_vectors(l, k)
            assert pm.n_up_to(l, k) == run, (l, k)
    for l in (13, 38, 107, 182, 363):
        for k in (1, 2, 3, 5, 8):
            assert pm.n_vectors(l, k) == pv.codebook_size(l, k), (l, k)
    assert pm.n_vectors(5, -1) == 0 == pm.n_up_to(5, -1)
    # the closed forms the kernels use for l <= 2
    for k in (1, 2, 7, 1 << 30):
        assert pm.n_vectors(1, k) == 2 and pm.n_vectors(2, k) == 4 * k
        assert pm.n_up_to(1, k) == 1 + 2 * k and pm.n_up_to(2, k) == 1 + 2 * k * (k + 1)


@pytest.mark.parametrize("l", range(1, 7))
def test_every_index_of_the_small_codebooks(l):
    """l <= 6, k <= 10: decode of every index equals the oracle's, and the index of the vector is the index"""
    for k in range(0, 11):
        n = pm.n_vectors(l, k)
        assert n == pv.codebook_size(l, k)
        for b in range(n):
            y = pm.pvq_decode(b, l, k)
            assert y == pv.pvq_decode(b, l, k).tolist(), (l, k, b)
            assert sum(abs(v) for v in y) == k
            assert pm.pvq_index(y, k) == b == pv.pvq_index(y, k), (l, k, b)


def test_pulses_for_bits_where_the_oracle_finishes():
    """every l <= 64 and every bits <= 32 at which K stays <= 4096 (the model says which; the oracle counts K up from
    1 and does not come back from (2, 32))"""
    checked = 0
    for l in range(2, 65):
        for bits in range(0, 33):
            k, width = pm.pulses_for_bits(l, bits)
            assert pm.n_vectors(l, k) <= 1 << bits < pm.n_vectors(l, k + 1)
            assert 1 <= width <= max(bits, 1) and (k > 0 or width == 1)
            if k <= 4096:
                assert (k, width) == pv.pulses_for_bits(l, bits), (l, bits)
                checked += 1
    assert checked > 1900
    with pytest.raises(ValueError):
        pm.pulses_for_bits(1, 8)


def test_index_width_is_the_references_rule():
    for n in list(range(1, 70)) + [2 ** e + d for e in range(7, 33) for d in (-1, 0, 1)]:
        if n <= 1 << 32:
            assert pm.index_width(n) == int(np.ceil(np.log2(n + pv.EPS))), n


def test_random_indices_vs_oracle():
    """2 000 seeded (l, k, index): l <= 363 (the longest band), N < 2^32 (the widest leaf), K small enough for the
    oracle's walk.  The oracle's N(l, k) costs a loop over l per call, its decode some l^2: 1 900 draws have l <= 40,
    a hundred go up to 363."""
    rng = np.random.default_rng(20261019)
    seen_l = set()
    for i in range(2000):
        lo, hi = (2, 41) if i % 20 else (41, 364)
        l = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        k_top = min(pm.pulses_for_bits(l, 32)[0], 4096)
        while pm.n_vectors(l, k_top) >= 1 << 32:
            k_top -= 1
        k = int(rng.integers(1, k_top + 1))
        n = pm.n_vectors(l, k)
        assert n < 1 << 32
        b = int(rng.integers(0, n))
        y = pm.pvq_decode(b, l, k)
        assert y == pv.pvq_decode(b, l, k).tolist(), (l, k, b)
        assert pm.pvq_index(y, k) == b
        seen_l.add(l)
    assert min(seen_l) == 2 and max(seen_l) >= 300


def _draw_vector(rng, l, k):
    """a vector of the pyramid with pulses spread over random places"""
    cuts = np.sort(rng.integers(0, k + 1, l - 1)).tolist()
    mags = [b - a for a, b in zip([0] + cuts, cuts + [k])]
    order = rng.permutation(l).tolist()
    return [int(mags[order[i]]) * (1 if rng.integers(0, 2) else -1) for i in range(l)]


@pytest.mark.parametrize("l", [2, 3, 4])
def test_the_largest_leaves_round_trip(l):
    """beyond the oracle's reach the model is checked against itself: K of 32 bits, drawn vectors and drawn indices,
    the codebook's ends and the vectors with all pulses on one component"""
    k, width = pm.pulses_for_bits(l, 32)
    n = pm.n_vectors(l, k)
    assert width == 32 and n <= 1 << 32 < pm.n_vectors(l, k + 1)
    assert (l, k) in ((2, 1 << 30), (3, 32767), (4, 1172))
    rng = np.random.default_rng(l)
    for _ in range(300):
        y = _draw_vector(rng, l, k)
        b = pm.pvq_index(y, k)
        assert 0 <= b < n and pm.pvq_decode(b, l, k) == y
        b = int(rng.integers(0, n))
        y = pm.pvq_decode(b, l, k)
        assert sum(abs(v) for v in y) == k and pm.pvq_index(y, k) == b
    assert pm.pvq_decode(0, l, k) == [0] * (l - 1) + [k]
    assert pm.pvq_decode(1, l, k) == [0] * (l - 1) + [-k]
    assert pm.pvq_decode(n - 1, l, k) == [-k] + [0] * (l - 1)
    assert pm.pvq_index([k] + [0] * (l - 1), k) == n - 2 and pm.pvq_decode(n - 2, l, k) == [k] + [0] * (l - 1)
    with pytest.raises(ValueError):
        pm.pvq_decode(n, l, k)
