"""Block-switched batches of any size assembled from a handful of frames (test infrastructure, NumPy only).

In a batch given as PcmView.frames(blocks) every output row of a frame depends on that frame's own 2048 samples per
channel, on its flag byte (bit 1 = last, 2 = cur, 4 = next, as k_stream_flags writes them) and, for the dropped-hop
rule alone, on the other channels of the same frame.  So a batch of 40 000 frames put together from a small set of
ATOMS must reproduce the atoms' rows exactly, wherever a frame lands in the long or the short list, whichever wave
walks it and however often that wave loops.  The atoms' rows are held to the oracle; everything else is equality.

ATOMS: eleven frames of int16 PCM at 48 kHz for up to three channels, made with integer arithmetic alone (PCG64 integers,
the committed sine table of tests/soak_programmes.py), so that they are the same samples on every machine.  An ITEM
is (atom, flag byte): item = 8 * atom + flag.  pattern(name, n_frames, seed) draws the items of a batch.
"""
import functools
import os

import numpy as np

import soak_programmes as sp

HERE = os.path.dirname(os.path.abspath(__file__))
HOP, N = 1024, 2048
SR = 48000
MAX_CH = 3

ATOMS = ("tone", "noise_low", "noise_mid", "attack", "drop", "zeros", "low_code", "cap", "castanet", "step",
         "full_noise")
N_ATOMS = len(ATOMS)
N_ITEMS = 8 * N_ATOMS
DROP, ZEROS, CAP = ATOMS.index("drop"), ATOMS.index("zeros"), ATOMS.index("cap")
LOW_CODE_AT = (0, 511, 512, 1023, 2047)
CASTANET_HOP = 12                      # hops 12 and 13 of the committed excerpt: quiet, then a stroke

PATTERNS = ("flags_all_long", "all_short", "alternate", "short_first_only", "short_last_only", "runs64", "owner_edges",
            "random01", "random50", "random99", "dropped_mix")
SIZES_SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
SIZES_LARGE = (16383, 16384, 16385, 40000)
MAX_FRAMES_3CH = 16385                 # three channels only up to here: memory for the frames view
LISTS_THREADS = 256                    # k_frame_lists_small: one workgroup, a thread owns ceil(n / 256) frames
LISTS_SMALL_MAX = 16384                # above: k_frame_lists (ballots and atomics)
LONG_FLAGS, SHORT_FLAGS = (0, 1, 4, 5), (2, 3, 6, 7)


def _noise(rng, lo, hi, n=N):
    return rng.integers(lo, hi, n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _master():
    """int16 [N_ATOMS, MAX_CH, 2048], read-only; atoms(n_ch) are its first n_ch channels"""
    a = np.zeros((N_ATOMS, MAX_CH, N), np.int64)
    castanet = np.load(os.path.join(HERE, "golden", "excerpt_castanet.npz"))["pcm"].astype(np.int64)
    cast = castanet[CASTANET_HOP * HOP:(CASTANET_HOP + 2) * HOP]
    cast = np.stack((cast[:, 0], cast[:, 1], (cast[:, 0] - cast[:, 1]) >> 1))
    for ch in range(MAX_CH):
        rng = np.random.default_rng(7100 + ch)
        # a steady tone: 440, 1320, 3520 Hz at about -10 dB
        f_mhz = (440_000, 1_320_000, 3_520_000)[ch]
        inc = np.full(N, (f_mhz << 32) // (1000 * SR), np.int64)
        a[0, ch] = (sp._osc(int(rng.integers(0, 1 << 32)), inc) * 10000) >> 15
        a[1, ch] = _noise(rng, -300, 301)
        a[2, ch] = _noise(rng, -6000, 6001)
        # an attack in the second half: a low bed, a burst from sample 1500 on
        x = _noise(rng, -40, 41)
        x[1500:] += _noise(rng, -20000, 20001, N - 1500)
        a[3, ch] = x
        # the dropped hop: channel 0 is digital silence up to sample 960, that is all of sub-blocks 0..2 (samples
        # 448 + 128 j ... + 256) -- coded short the WHOLE hop is dropped, in every channel; coded long it is an
        # ordinary frame with an attack
        x = _noise(rng, -40, 41)
        x[960:] += _noise(rng, -15000, 15001, N - 960)
        if ch == 0:
            x[:960] = 0
        a[4, ch] = x
        # a[5] stays zeros
        x = _noise(rng, -6000, 6001)
        x[list(LOW_CODE_AT)] = -32768
        a[6, ch] = x
        # allocations at their cap of 16 bits: a full-scale 123 Hz tone under a raised-cosine envelope over samples
        # 256 ... 1791.  Coded short, every band but the lowest of a sub-block falls out of BitAlloc and the 14 lines
        # left share the whole budget.  (Full-scale noise, the next atom, spreads its bits evenly: 4 bits a line in
        # a long block, 12 at most in a short one.)
        w = 1536
        inc = np.full(w, (123_000 << 32) // (1000 * SR), np.int64)
        env = 32767 - sp.sine_table()[(np.arange(w) * 4096 // w + 1024) % 4096]          # 1 - cos, 0 ... 65534
        a[7, ch, 256:256 + w] = (sp._osc(ch << 30, inc) * env) >> 16
        a[8, ch] = cast[ch]
        # a level step at the hop boundary: the prior hop 50 dB below the hop
        x = _noise(rng, -25, 26)
        x[HOP:] = _noise(rng, -8000, 8001, HOP)
        a[9, ch] = x
        a[10, ch] = _noise(rng, -32768, 32768)
    out = np.clip(a, -32768, 32767).astype(np.int16)
    out.setflags(write=False)
    return out


def atoms(n_ch):
    """int16 [N_ATOMS, n_ch, 2048]"""
    assert 1 <= n_ch <= MAX_CH
    return _master()[:, :n_ch]


def item_frames(n_ch):
    """the atom batch: int16 [N_ITEMS, n_ch, 2048] and uint8 flags [N_ITEMS], item i = (atom i // 8, flag i % 8)"""
    items = np.arange(N_ITEMS)
    return np.ascontiguousarray(atoms(n_ch)[items // 8]), (items % 8).astype(np.uint8)


def flag_tuple(flag):
    return (flag & 1, (flag >> 1) & 1, (flag >> 2) & 1)


# ------------------------------------------------------------------------------------------------- patterns
def owner_range(n_frames):
    """per = ceil(n / 256) and, for every thread of k_frame_lists_small that owns a frame, its first and last one"""
    per = -(-n_frames // LISTS_THREADS)
    first = np.arange(0, n_frames, per)
    last = np.minimum(first + per, n_frames) - 1
    return per, first, last


def _cur_of(name, n, rng):
    f = np.arange(n)
    if name == "flags_all_long":
        return np.zeros(n, bool)
    if name == "all_short":
        return np.ones(n, bool)
    if name == "alternate":
        return f % 2 == 0
    if name == "short_first_only":
        return f == 0
    if name == "short_last_only":
        return f == n - 1
    if name == "runs64":
        return (f // 64) % 2 == 0
    if name == "owner_edges":
        cur = np.zeros(n, bool)
        _, first, last = owner_range(n)
        cur[first] = True
        cur[last] = True
        return cur
    share = {"random01": 1, "random50": 50, "random99": 99, "dropped_mix": 50}[name]
    return rng.integers(0, 100, n) < share


def pattern(name, n_frames, seed=0):
    """-> (item_index int32 [n_frames], flags uint8 [n_frames]); flags = item_index % 8.  The cur bits are what the
    name says; the last / next bits and the atoms are drawn.  The random* patterns and dropped_mix carry every one of
    the eight flag bytes from 8 frames on (they are planted at eight drawn places, so the share of short frames is
    the named one to within 4 frames of the draw)."""
    assert name in PATTERNS and n_frames >= 1
    n = int(n_frames)
    rng = np.random.default_rng([PATTERNS.index(name), n, int(seed)])
    cur = _cur_of(name, n, rng)
    other = rng.integers(0, 4, n)                          # bit 0: last, bit 1: next
    flags = (other & 1) | (cur.astype(np.int64) << 1) | ((other >> 1) << 2)
    if name.startswith("random") or name == "dropped_mix":
        if n >= 8:
            flags[rng.permutation(n)[:8]] = np.arange(8)
    atom = rng.integers(0, N_ATOMS, n)
    if name == "dropped_mix":
        # of the short frames every fourth is the dropped-hop atom, the others are neither that one nor silence
        # (which is dropped as well when it is coded short): a quarter of the short frames, rounded up, is dropped
        short = np.flatnonzero(flags & 2)
        others = np.array([k for k in range(N_ATOMS) if k not in (DROP, ZEROS)])
        atom[short] = others[rng.integers(0, len(others), len(short))]
        atom[short[::4]] = DROP
    item = (atom * 8 + flags).astype(np.int32)
    return item, flags.astype(np.uint8)


def sizes_for(n_ch):
    return tuple(n for n in SIZES_SMALL + SIZES_LARGE if n_ch < 3 or n <= MAX_FRAMES_3CH)


# ------------------------------------------------------------------------------------------------- the oracle
HANDLES = {"scalar": dict(kbps=128, use_vq=False, use_sbr=False), "vq128": dict(kbps=128, use_vq=True, use_sbr=False),
           "vq96": dict(kbps=96, use_vq=True, use_sbr=True)}


def oracle_params(handle, n_ch):
    from oracle import pac_oracle as po, pac_oracle_vq as pv
    h = HANDLES[handle]
    p = pv.make_params_vq(SR, n_ch, h["kbps"]) if h["use_vq"] else po.make_params(SR, n_ch, h["kbps"])
    assert bool(p.useSBR) == h["use_sbr"]
    return p


def oracle_item(handle, n_ch, item, p=None):
    """the oracle's run of one item: (parts, records) -- parts [ch] = the list of one (long) or eight (short) coded
    blocks as encode_hop / encode_hop_vq return them, records [ch] = payload bytes; (None, None) for a dropped hop"""
    from oracle import pac_oracle as po, pac_oracle_vq as pv
    p = p or oracle_params(handle, n_ch)
    frac = po.pcm16_to_fraction(atoms(n_ch)[item // 8])
    flags = flag_tuple(item % 8)
    prior, hop = [frac[ch, :HOP] for ch in range(n_ch)], [frac[ch, HOP:] for ch in range(n_ch)]
    if HANDLES[handle]["use_vq"]:
        parts = pv.encode_hop_vq(p, prior, hop, flags)
        pack = pv.pack_channel_block_vq
    else:
        parts = po.encode_hop(p, prior, hop, flags)
        pack = po.pack_channel_block
    if parts is None:
        return None, None
    records = []
    for ch in range(n_ch):
        n_bytes, payload = pack(p, flags, parts[ch])
        assert len(payload) == n_bytes
        records.append(payload)
    return parts, records


@functools.lru_cache(maxsize=None)
def oracle_items(handle, n_ch):
    """oracle_item of every item, computed once per process: ([parts], [records])"""
    p = oracle_params(handle, n_ch)
    got = [oracle_item(handle, n_ch, i, p) for i in range(N_ITEMS)]
    return [g[0] for g in got], [g[1] for g in got]
