"""The masked-threshold kernels on the blocks of tests/mask_cases.py: spectra that sit ON the inequalities by which
side_long_one prunes maskers and k_mask skips batches and chunks (csrc/k_psy.hip).  tests/test_mask_cases.py shows on
the CPU that each block is what it claims and that a wrong skip moves the oracle's own threshold by 1e-5 dB and more.

Bars (the project's): peak counts equal; every line of the masked threshold and every band's SMR
within DB_TOL = 1e-9 dB of the oracle; codes of the whole encode equal unit by unit; reorderings bit for bit.
"""
import numpy as np
import pytest

import mask_cases as mc
from oracle import pac_oracle as po
from test_gpu_parity import DB_TOL, A, enc_for, frames_view, torch          # noqa: F401  (A, torch are fixtures)
from test_gpu_round3 import fresh_handles                                    # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

CASES = mc.cases()
WORST = {}                       # largest |delta| seen, by (quantity, entry point): printed, and quoted in DESIGN.md


def groups(short, dtype, coded=False):
    """[(rate, cases)]: what goes into one batch -- one block kind, one sample type, one rate"""
    sel = [c for c in CASES if c.short == short and (dtype == "f64" or c.i16) and not (coded and c.family == "e")]
    return [(sr, [c for c in sel if c.sr == sr]) for sr in sorted({c.sr for c in sel})]


def samples(cases, dtype):
    return np.stack([mc.as_int16(c.x) if dtype == "i16" else c.x for c in cases])


def fractions(case, dtype):
    return mc.rendered(case) if dtype == "i16" else case.x


def gpu_smr(A, torch, enc, x, short):
    """x [n, 2048] or [n, n_ch, 2048] -> lines from Encoder.mdct, then Encoder.smr: host arrays per channel-frame"""
    t = torch.as_tensor(np.ascontiguousarray(x), device=enc.device)
    view = A.engine.PcmView.frames(t if t.dim() == 3 else t.view(x.shape[0], 1, x.shape[1]))
    lines = enc.mdct(view, None, short=short).reshape(view.n_cf, 1024)
    smr, thr, npk = enc.smr(view, lines, short=short, want_threshold=True, want_peaks=True)
    return {"lines": lines.cpu().numpy(), "smr": smr.cpu().numpy(), "thr": thr.cpu().numpy(),
            "npk": npk.cpu().numpy().reshape(view.n_cf, -1)}


def oracle_units(case, dtype, lines, p):
    """[(sub-block, line offset, band offset, peak count, threshold, SMRs)] of one case from the oracle, its SMRs on
    the lines the GPU's MDCT gave (lines are compared elsewhere, to 2e-12 of the block maximum)"""
    out = []
    x = fractions(case, dtype)
    bands = p.sfBandsShort if case.short else p.sfBands
    m = 128 if case.short else 1024
    for sb, blk in enumerate(mc.blocks_of(case, x)):
        n_peaks = len(po.find_peaks(po.sidechain_intensity(blk), np.fft.rfftfreq(len(blk), d=1 / case.sr))[0])
        thr = po.masked_threshold(blk.copy(), m, case.sr)
        smr = po.calc_smrs(blk.copy(), lines[sb * m:(sb + 1) * m].copy(), 0, case.sr, bands)
        out.append((sb, sb * m, sb * bands.nBands, n_peaks, thr, smr))
    return out


@pytest.fixture(scope="module")
def batches(A, torch):
    """Every case through Encoder.mdct + Encoder.smr once per sample type, with the oracle's answers: computed once,
    shared by the tests below and left unchanged."""
    out = {}
    for short in (False, True):
        for dtype in ("f64", "i16"):
            for sr, cases in groups(short, dtype):
                enc, p = enc_for(A, sr), po.make_params(sr, 1, 128)
                got = gpu_smr(A, torch, enc, samples(cases, dtype), short)
                ref = [oracle_units(c, dtype, got["lines"][i], p) for i, c in enumerate(cases)]
                out[(short, dtype, sr)] = (cases, got, ref)
    return out


def compare(tag, cases, ref, npk, thr, smr):
    """npk / thr / smr: callables (i, unit) -> what the GPU gave for unit `unit` of case i"""
    worst_thr = worst_smr = 0.0
    for i, case in enumerate(cases):
        for unit in ref[i]:
            sb, _, _, n_peaks, want_thr, want_smr = unit
            where = f"{tag} {case.name}" + (f" sub-block {sb}" if case.short else "")
            assert int(npk(i, unit)) == n_peaks, f"{where}: peak count; built for {case.prop}"
            d_thr = np.abs(thr(i, unit) - want_thr)
            worst_thr = max(worst_thr, float(d_thr.max()))
            print(f"{where}: |d thr| {d_thr.max():.3e}  |d smr| {np.abs(smr(i, unit) - want_smr).max():.3e}")
            bad = np.nonzero(~(d_thr < DB_TOL))[0]
            assert len(bad) == 0, (f"{where}: threshold off by {d_thr[bad[0]]:.3e} dB at " +
                                   mc.nearest_planted(case, int(bad[0])) + f" ({len(bad)} lines in all)")
            d_smr = np.abs(smr(i, unit) - want_smr)
            worst_smr = max(worst_smr, float(d_smr.max()))
            bad = np.nonzero(~(d_smr < DB_TOL))[0]
            assert len(bad) == 0, f"{where}: SMR of band {bad[0]} off by {d_smr[bad[0]]:.3e} dB; built for {case.prop}"
    WORST[("thr", tag)] = max(WORST.get(("thr", tag), 0.0), worst_thr)
    WORST[("smr", tag)] = max(WORST.get(("smr", tag), 0.0), worst_smr)
    print(f"largest |d threshold| {worst_thr:.3e} dB, |d SMR| {worst_smr:.3e} dB ({tag})")


@pytest.mark.parametrize("dtype", ["f64", "i16"])
@pytest.mark.parametrize("kind", ["long", "short"])
def test_smr_on_constructed_spectra(batches, kind, dtype):
    """Encoder.smr (k_side_long / k_side_short + k_mask): peak counts, every line of the threshold, every band's SMR"""
    short = kind == "short"
    seen = 0
    for (sh, dt, sr), (cases, got, ref) in batches.items():
        if (sh, dt) != (short, dtype):
            continue
        nb = len(ref[0][0][5])
        compare(f"smr {kind} {dtype} {sr}", cases, ref,
                lambda i, u: got["npk"][i, u[0]],
                lambda i, u: got["thr"][i, u[1]:u[1] + len(u[4])],
                lambda i, u: got["smr"][i, u[2]:u[2] + nb])
        seen += len(cases)
    assert seen == sum(len(cs) for _, cs in groups(short, dtype)) > 0


@pytest.mark.parametrize("kind", ["long", "short"])
def test_generic_kernel_on_constructed_spectra(A, torch, batches, kind):
    """k_smr_generic takes every masker at every line -- no pruning, no screen: an independent statement on the GPU,
    held to the same bars on the same blocks (both renderings, as float64 blocks)"""
    short = kind == "short"
    n, m = (256, 128) if short else (2048, 1024)
    for (sh, dtype, sr), (cases, got, ref) in batches.items():
        if sh != short:
            continue
        enc = enc_for(A, sr)
        bands = enc.sfBandsShort if short else enc.sfBands
        t = A.psychoac._generic_tables(n, sr, bands, enc.device)
        data = np.stack([blk for c in cases for blk in mc.blocks_of(c, fractions(c, dtype))])
        lines = got["lines"].reshape(len(data), m)
        g_smr, g_thr, g_npk = enc.smr_generic(torch.as_tensor(data, device=enc.device),
                                              torch.as_tensor(lines, device=enc.device), t,
                                              want_threshold=True, want_peaks=True)
        g_smr, g_thr, g_npk = g_smr.cpu().numpy(), g_thr.cpu().numpy(), g_npk.cpu().numpy()
        per = 8 if short else 1
        compare(f"generic {kind} {dtype} {sr}", cases, ref,
                lambda i, u: g_npk[i * per + u[0]], lambda i, u: g_thr[i * per + u[0]],
                lambda i, u: g_smr[i * per + u[0]])


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("kind", ["long", "short"])
def test_order_of_the_batch_does_not_matter(A, torch, batches, kind):
    """The batch reversed, with a silent frame between every two cases, and as two interleaved channels (one in the
    given order, one reversed) against the planar runs: thresholds, SMRs and peak counts bit for bit, case by case.
    k_mask is persistent: what a wave keeps from one unit to the next (running maxima in registers and LDS, the
    masker table, the band keys, the prefetched batch) would show here."""
    short = kind == "short"
    rates = set()
    for (sh, dtype, sr), (cases, got, _) in batches.items():
        if sh != short or dtype != "f64":
            continue
        rates.add(sr)
        enc = enc_for(A, sr)
        x = samples(cases, "f64")
        n = len(cases)

        def check(run, at, tag):
            for i, case in enumerate(cases):
                for key in ("thr", "smr"):
                    assert same_bits(run[key][at(i)], got[key][i]), (tag, case.name, key, case.prop)
                assert np.array_equal(run["npk"][at(i)], got["npk"][i]), (tag, case.name, "peak count")

        check(gpu_smr(A, torch, enc, x[::-1], short), lambda i: n - 1 - i, "reversed")
        spaced = np.zeros((2 * n + 1, 2048))
        spaced[1::2] = x
        run = gpu_smr(A, torch, enc, spaced, short)
        check(run, lambda i: 2 * i + 1, "silent frames between")
        quiet = mc.line_tables(128 if short else 1024, sr)[1]
        for f in range(0, 2 * n + 1, 2):
            assert not run["npk"][f].any()
            assert np.max(np.abs(run["thr"][f].reshape(-1, len(quiet)) - quiet)) < DB_TOL
        run = gpu_smr(A, torch, enc, np.stack((x, x[::-1]), axis=1), short)
        check(run, lambda i: 2 * i, "two channels, channel 0")
        check(run, lambda i: 2 * (n - 1 - i) + 1, "two channels, channel 1")
    assert rates == {sr for sr, _ in groups(short, "f64")}


def test_second_and_third_unit_of_a_persistent_wave(A, torch, batches):
    """A wave of k_mask<1024> takes a second unit only in a batch of more channel-frames than the grid has waves
    (16 a compute unit): the long cases repeated over 2 x 4096 + 37 channel-frames, so that every wave runs two or
    three DIFFERENT cases one after the other; each frame's threshold and SMRs are the bits of its case alone."""
    (cases, got, _) = batches[(False, "f64", mc.SR)]
    enc = enc_for(A, mc.SR)
    x = samples(cases, "f64")
    n = len(cases)
    assert 4096 % n != 0                          # the case a wave meets next is never the one it just had
    which = np.arange(2 * 4096 + 37) % n
    run = gpu_smr(A, torch, enc, x[which], False)
    for key in ("thr", "smr", "npk"):
        want = got[key][which]
        same = np.all(run[key].reshape(len(which), -1) == want.reshape(len(which), -1), axis=1)
        bad = np.nonzero(~same)[0]
        assert len(bad) == 0, (key, f"frame {bad[0]}", cases[which[bad[0]]].name, f"{len(bad)} frames differ")


# ------------------------------------------------------------------ the whole encode path
_codes = {}


def oracle_codes(case, dtype, p):
    """po.encode_channel of a long case, or of each sub-block of a short one that is not digital silence (the
    reference drops a hop with a silent sub-block, coder/pacfile.py:530-533; the kernels flag it)"""
    key = (case.name, dtype)
    if key not in _codes:
        x = fractions(case, dtype)
        if case.short:
            p.nMDCTLines = p.nSamplesPerBlock = 128
            try:
                _codes[key] = {sb: po.encode_channel(blk.copy(), p, False, True, False)
                               for sb, blk in enumerate(mc.blocks_of(case, x)) if blk.any()}
            finally:
                p.nMDCTLines = p.nSamplesPerBlock = 1024
        else:
            _codes[key] = {0: po.encode_channel(x.copy(), p)}
    return _codes[key]


@pytest.mark.parametrize("env", [None, ("PACX_FUSE_TAIL", "0"), ("PACX_FUSE_FRONT", "0")],
                         ids=["default", "FUSE_TAIL=0", "FUSE_FRONT=0"])
def test_encode_on_constructed_spectra(A, torch, monkeypatch, fresh_handles, env):
    """Encoder.encode: int16 batches take k_front_long + k_mask<1024, true>, float64 batches k_side_long; overall
    scale, allocation, scale factors and mantissas equal the oracle's unit by unit, by default and with the tail
    and the front end as separate kernels; the short frames with flags that mark them short.  (The loud family is
    left out: it is made for the threshold.)"""
    for k in ("PACX_FUSE_TAIL", "PACX_FUSE_FRONT", "PACX_SPLIT_SHORT"):
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(*env)
    A.context.clear()                              # the overrides are read when a handle is created
    n_units = 0
    for short in (False, True):
        for dtype in ("i16", "f64"):
            for sr, cases in groups(short, dtype, coded=True):
                enc, p = enc_for(A, sr), po.make_params(sr, 1, 128)
                flags = np.full(len(cases), 2, np.uint8) if short else None
                out = enc.encode(frames_view(A, torch, enc, samples(cases, dtype)), flags)
                host = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
                for i, case in enumerate(cases):
                    for sb, want in oracle_codes(case, dtype, p).items():
                        got = A.codec.unpack_short(enc, host, i, sb) if short else A.codec.unpack_long(enc, host, i)
                        where = (env, dtype, case.name, sb, case.prop)
                        assert got[3] == want[3], ("overall scale",) + where
                        assert got[1].tolist() == want[1].tolist(), ("allocation",) + where
                        assert got[0].tolist() == want[0].tolist(), ("scale factors",) + where
                        assert got[2].tolist() == want[2].tolist(), ("mantissas",) + where
                        n_units += 1
    assert n_units > len(CASES)


def test_zz_margins_seen(batches):
    """the record of the margin (DESIGN.md section 2 quotes it): the bar is the project's, these are what was seen"""
    for (quantity, tag), v in sorted(WORST.items()):
        print(f"measured: largest |d {quantity}| {v:.3e} dB ({tag})")
        assert v < DB_TOL
