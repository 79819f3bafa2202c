"""tests/pcm_layouts.py on the CPU: every layout, evaluated as the kernels address it, is the planar stream view."""
import numpy as np
import pytest

import pcm_layouts as pl


def material(n_ch, n_hops, seed):
    rng = np.random.default_rng(seed)
    planar = rng.integers(-32768, 32768, (n_ch, (n_hops + 1) * 1024)).astype(np.int16)
    planar[:, 5] = -32768
    return planar


@pytest.mark.parametrize("n_ch,n_hops", [(1, 1), (2, 4), (3, 3)])
@pytest.mark.parametrize("kind", pl.KINDS)
def test_layout_addresses_the_planar_samples(kind, n_ch, n_hops):
    planar = material(n_ch, n_hops, 7 * n_ch + n_hops)
    buf, dtype, c, F, fs, cs, ss, off = pl.make(planar, kind)
    assert (c, F) == (n_ch, n_hops) and buf.dtype == dtype and buf.ndim == 1
    assert dtype == (np.float64 if kind.startswith("f64") else np.int16)
    at = pl.addresses(c, F, fs, cs, ss, off)
    assert at.min() >= 0 and at.max() == off + pl.last_index(c, F, fs, cs, ss) < len(buf)
    got, want = buf[at], pl.expected(planar, kind)
    assert got.dtype == want.dtype
    if dtype == np.float64:          # bit for bit: the sign of the zero that -32768 becomes included
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
        assert np.array_equal(want, pl.po.pcm16_to_fraction(pl.expected(planar, "broadcast" if kind == "broadcast"
                                                                            else "planar")))
    else:
        assert np.array_equal(got, want)
    # everything the view does not address is poison
    rest = np.ones(len(buf), bool)
    rest[at.ravel()] = False
    if kind not in pl.NO_POISON:
        assert rest.any()
    if kind != "broadcast" or n_ch == 1:
        assert kind not in pl.NO_POISON or not rest.any()
    if dtype == np.float64:
        assert np.isnan(buf[rest]).all() and not np.isnan(buf[~rest]).any()
    else:
        assert (np.abs(buf[rest].astype(np.int32)) == 32767).all()
        if rest.sum() > 1:
            assert (buf[rest] > 0).any() and (buf[rest] < 0).any()
    # check_pcm's choice: only planar and broadcast are views the fast kernels take
    assert pl.fast(dtype, off, fs, cs, ss) == (kind in ("planar", "broadcast"))
    # a smaller sample stride or a dropped channel term reach lower addresses only: still inside the buffer
    assert pl.addresses(c, F, fs, cs, 1, off).max() < len(buf) and pl.addresses(c, F, fs, 0, ss, off).max() < len(buf)


def test_generic_kinds_are_what_the_table_says():
    planar = material(2, 3, 1)
    _, _, _, _, fs, cs, ss, off = pl.make(planar, "interleaved")
    assert (cs, ss) == (1, 2)
    _, _, _, _, fs, cs, ss, off = pl.make(planar, "shifted")
    assert off == 1 and fs % 8 == 0 and cs % 8 == 0 and ss == 1
    _, _, _, _, fs, cs, ss, off = pl.make(planar, "odd_rows")
    assert off == 0 and cs % 8 == 3 and fs % 8 == 0
    _, _, _, _, fs, cs, ss, off = pl.make(planar, "odd_frames")
    assert fs == 2 * 1024 + 4
    _, _, _, _, fs, cs, ss, off = pl.make(planar, "every_third")
    assert ss == 3
    _, _, _, _, fs, cs, ss, off = pl.make(planar, "broadcast")
    assert cs == 0
