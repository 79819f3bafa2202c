"""tests/mixed_batches.py on the CPU: the patterns are what their names say for every size the GPU tests run, and
every item (atom, flag byte) goes through the oracle with the scalar coder and both gain-shape configurations, for
1, 2 and 3 channels -- with the property that makes each atom worth having asserted on the oracle's own output."""
import numpy as np
import pytest

import mixed_batches as mb
from oracle import pac_oracle as po

ALL_SIZES = mb.SIZES_SMALL + mb.SIZES_LARGE


def test_atoms_are_what_they_claim():
    a = mb.atoms(3)
    assert a.shape == (mb.N_ATOMS, 3, mb.N) and a.dtype == np.int16 and mb.N_ATOMS == 11 and mb.N_ITEMS == 88
    assert mb.N_ITEMS <= 96                                            # one small batch holds every item
    for n_ch in (1, 2):
        assert np.array_equal(mb.atoms(n_ch), a[:, :n_ch])
    at = {name: a[i].astype(np.int64) for i, name in enumerate(mb.ATOMS)}
    assert not at["zeros"].any()
    for name in mb.ATOMS:
        if name != "zeros":
            assert all(at[name][ch].any() for ch in range(3)), name
            assert not np.array_equal(at[name][0], at[name][1]) and not np.array_equal(at[name][1], at[name][2]), name
    # the dropped hop: sub-blocks 0..2 (samples 448 + 128 j ... + 256) silent in channel 0 alone, sub-block 3 not
    sub = lambda x, j: x[448 + 128 * j:448 + 128 * j + 256]
    assert all(not sub(at["drop"][0], j).any() for j in range(3)) and sub(at["drop"][0], 3).any()
    assert all(sub(at["drop"][ch], j).any() for ch in (1, 2) for j in range(8))
    for name in mb.ATOMS:
        if name not in ("drop", "zeros"):
            assert all(sub(at[name][ch], j).any() for ch in range(3) for j in range(8)), name
    assert (at["low_code"][:, list(mb.LOW_CODE_AT)] == -32768).all() and (at["low_code"] == -32768).sum() == 15
    assert np.abs(at["attack"][:, :1500]).max() <= 40 and np.abs(at["attack"][:, 1500:]).max() > 15000
    assert np.abs(at["step"][:, :mb.HOP]).max() <= 25 and np.abs(at["step"][:, mb.HOP:]).max() > 7000
    assert at["full_noise"].min() < -32000 and at["full_noise"].max() > 32000
    assert np.abs(at["tone"]).max() in range(9990, 10001)
    # the castanet frame holds a real transient: the reference's detector fires on its second hop, not on its first
    frac = po.pcm16_to_fraction(a[mb.ATOMS.index("castanet"), :2])
    look = lambda h: np.concatenate((frac[:, h * mb.HOP:(h + 1) * mb.HOP], np.zeros((2, mb.HOP))), axis=1)
    assert po.transient_detect(look(1)) is True and not po.transient_detect(look(0))
    frames, flags = mb.item_frames(2)
    assert frames.shape == (mb.N_ITEMS, 2, mb.N) and flags.tolist() == [i % 8 for i in range(mb.N_ITEMS)]
    assert np.array_equal(frames[8 * mb.DROP + 3], a[mb.DROP, :2])


@pytest.mark.parametrize("name", mb.PATTERNS)
def test_patterns_meet_their_names(name):
    """every pattern, every size: the count and the places of the short frames; flags = item % 8; the same draw from
    the same seed and another from another"""
    counts = {}
    for n in ALL_SIZES:
        item, flags = mb.pattern(name, n)
        assert item.shape == flags.shape == (n,) and item.dtype == np.int32 and flags.dtype == np.uint8
        assert item.min() >= 0 and item.max() < mb.N_ITEMS and np.array_equal(item % 8, flags)
        again = mb.pattern(name, n)
        assert np.array_equal(again[0], item) and np.array_equal(again[1], flags)
        if n >= 63:
            assert not np.array_equal(mb.pattern(name, n, seed=1)[0], item)
        cur = (flags & 2) != 0
        f = np.arange(n)
        n_short = counts[n] = int(cur.sum())
        if name == "flags_all_long":
            assert n_short == 0
            if n >= 63:
                assert set(flags.tolist()) == set(mb.LONG_FLAGS)                  # the other bits are varied
        elif name == "all_short":
            assert n_short == n
            if n >= 63:
                assert set(flags.tolist()) == set(mb.SHORT_FLAGS)
        elif name == "alternate":
            assert np.array_equal(cur, f % 2 == 0) and n_short == (n + 1) // 2
        elif name == "short_first_only":
            assert n_short == 1 and cur[0]
        elif name == "short_last_only":
            assert n_short == 1 and cur[n - 1]
        elif name == "runs64":
            assert np.array_equal(cur, (f // 64) % 2 == 0)
            if n > mb.LISTS_SMALL_MAX:                 # whole waves of k_frame_lists with a full and an empty ballot
                waves = cur[:n // 64 * 64].reshape(-1, 64)
                assert waves.all(axis=1).sum() >= 128 and (~waves).all(axis=1).sum() >= 127
                assert (waves.all(axis=1) | (~waves).all(axis=1)).all()
        elif name == "owner_edges":
            per, first, last = mb.owner_range(n)
            assert per == -(-n // 256) and first[0] == 0 and last[-1] == n - 1 and len(first) <= 256
            assert (last - first <= per - 1).all() and (first[1:] == last[:-1] + 1).all()
            want = np.zeros(n, bool)
            want[first] = want[last] = True
            assert np.array_equal(cur, want)
            if per == 1:
                assert n_short == n
            elif per > 2:
                assert n_short < n and n_short >= 2 * len(first) - 1
        else:
            share = {"random01": 0.01, "random50": 0.5, "random99": 0.99, "dropped_mix": 0.5}[name]
            # a binomial draw, five standard deviations, and the eight planted flag bytes
            assert abs(n_short - share * n) <= 5 * np.sqrt(n * share * (1 - share)) + 8, (n, n_short)
            if n >= 257:
                assert set(flags.tolist()) == set(range(8)), n
                assert 4 <= n_short <= n - 4
            if name == "dropped_mix":
                atom = item[cur] // 8
                assert int((atom == mb.DROP).sum()) == -(-n_short // 4) and not (atom == mb.ZEROS).any()
                if n >= 257:
                    assert (item[~cur] // 8 == mb.DROP).any()              # and coded long the same atom is kept
        if n >= 1023 and name != "dropped_mix":
            assert len(set((item // 8).tolist())) == mb.N_ATOMS
    print(f"{name}: short frames of {len(ALL_SIZES)} sizes: " + ", ".join(f"{n}: {c}" for n, c in counts.items()))


def test_sizes():
    assert mb.sizes_for(1) == mb.sizes_for(2) == ALL_SIZES and max(mb.sizes_for(3)) == 16385
    assert 16384 in ALL_SIZES and 16385 in ALL_SIZES and mb.LISTS_SMALL_MAX == 16384      # both list kernels
    assert [-(-n // mb.LISTS_THREADS) for n in (256, 257, 16384)] == [1, 2, 64]


def _kinds(parts_of_items):
    """window kinds among the coded items: the oracle's window_kind of every flag byte"""
    return {po.window_kind(*mb.flag_tuple(i % 8)) for i, q in enumerate(parts_of_items) if q is not None}


def _check_items(handle, n_ch, alloc_of):
    parts, records = mb.oracle_items(handle, n_ch)
    assert len(parts) == len(records) == mb.N_ITEMS
    n_coded = 0
    for i, (q, recs) in enumerate(zip(parts, records)):
        atom, flag = divmod(i, 8)
        short = bool(flag & 2)
        if atom in (mb.DROP, mb.ZEROS):
            # the dropped-hop rule: None exactly when the cur bit is set -- whatever the other channels hold
            assert (q is None) == short, (handle, n_ch, mb.ATOMS[atom], flag)
        else:
            assert q is not None, (handle, n_ch, mb.ATOMS[atom], flag)
        if q is None:
            assert recs is None
            continue
        n_coded += 1
        assert len(q) == len(recs) == n_ch and all(len(ch) == (8 if short else 1) for ch in q)
        for ch in range(n_ch):
            assert 5 <= len(recs[ch]) and recs[ch][0] >> 5 == (flag & 1) << 2 | (flag & 2) | (flag & 4) >> 2
    assert n_coded == mb.N_ITEMS - 8
    # each of the four window kinds (sine, start, stop, start-stop) occurs with every atom, the sine window both
    # over a long block and over short sub-blocks
    assert len({po.window_kind(*mb.flag_tuple(fl)) for fl in range(8)}) == 4
    for atom in range(mb.N_ATOMS):
        if atom not in (mb.DROP, mb.ZEROS):
            assert len(_kinds([parts[atom * 8 + fl] for fl in range(8)])) == 4
    top = max(int(np.max(alloc_of(b))) for fl in mb.SHORT_FLAGS for ch in parts[mb.CAP * 8 + fl] for b in ch)
    noise = max(int(np.max(alloc_of(b))) for fl in range(8) for ch in parts[(mb.N_ATOMS - 1) * 8 + fl] for b in ch)
    return n_coded, top, noise


@pytest.mark.parametrize("n_ch", [1, 2, 3])
def test_oracle_on_every_item_scalar(n_ch):
    n_coded, top, noise = _check_items("scalar", n_ch, lambda b: b[1])
    print(f"scalar 128 kb/s, {n_ch} ch: {mb.N_ITEMS} items, {n_coded} coded, 8 dropped; largest allocation of the cap "
          f"atom {top} bits, of full-scale noise {noise}")
    assert top == 16                                       # the cap atom reaches maxMantBits in some band
    assert noise < 16


@pytest.mark.parametrize("n_ch", [1, 2, 3])
@pytest.mark.parametrize("handle", ["vq128", "vq96"])
def test_oracle_on_every_item_gain_shape(handle, n_ch):
    """gain-shape PVQ at 128 kb/s without SBR and at 96 kb/s with it.  At 96 kb/s a short sub-block has 294 bits to
    give instead of 417 and the cap atom's lowest band ends at 14 bits a line, so the cap is asserted at 128 only."""
    n_coded, top, noise = _check_items(handle, n_ch, lambda b: b[0])
    print(f"{handle}, {n_ch} ch: {mb.N_ITEMS} items, {n_coded} coded, 8 dropped; largest allocation of the cap atom "
          f"{top} bits, of full-scale noise {noise}")
    p = mb.oracle_params(handle, n_ch)
    assert bool(p.useSBR) == (handle == "vq96") and p.useVQ
    if handle == "vq128":
        assert top == 16
