"""Hand-written gain-shape records as .pac streams: the counterpart of tests/code_streams.py for the PVQ / SBR coder.

A gain-shape record is a pure function of its bits.  The allocations fix every band's position; inside a band the
decoder walks a tree (oracle.pac_oracle_vq.split_decode) whose every field is free within its width (split angles,
gains) or within a codebook (leaf indices).  The suite's decode tests only ever saw what an encoder wrote from audio.
This module DRAWS the records instead: flags, overall scales and allocations per band (0 or 2..max_alloc), then, band
by band, it walks the tree with the oracle's own gain_shape_alloc / mid_side_alloc and pvq_model.pulses_for_bits and
draws a value at every field -- an angle index below 2^width, a leaf index BELOW N(l, K) (indices in [N, 2^width) are
outside the codebook; what the reference does there is not pinned, they stay out), a gain index below 2^width.  The
record is written with the oracle's write_block_body_vq / pack_channel_block_vq, the header with pac_header.

    case(name) -> Case          the file, the records, the drawn header codes, every node of every tree (see Case)
    decode_float_vq(pac)        the oracle's decode_stream_vq / decode_block_vq with its three leaf functions that are
                                linear in K (pulses_for_bits, codebook_size, pvq_decode) replaced by pvq_model's for
                                the duration of the call (unittest.mock.patch.object; oracle/ itself is unchanged)

Well-formed records only: every case is a file the oracle's decoder takes.  Two things a drawn tree could reach are
kept out by the walk, which redraws the angle of the split above, or, where no angle helps, lowers the band's
allocation (the final allocations are the Case's):
  * a leaf of ONE line, where the reference's pulses_for_bits never returns.  No walk reaches one: a 2-line node with
    more than 32 bits is a split whose angle takes ALL its bits (half = 1: a_theta = bits, a_rest = 0), both halves are
    zeros and the node decodes to a zero vector; theta_32_33 and theta_max hold such nodes and the census counts them;
  * an angle of more than 62 bits (a_theta = floor(bits / half + log2(half) / 2) of a node that got nearly all bits of
    a wide band): the oracle decodes it, the kernels flag the block PACX_ST_VQ_UNDEFINED.  `theta_wide` alone draws
    such nodes ON PURPOSE and says which channel-frames hold them (Case.undefined);
  * a gain of more than 64 bits (never met: the census records the widest gain seen).
One more thing stays out, for the comparison's sake: an angle at which the argument of floor() in mid_side_alloc lies
within 1e-9 of a whole number.  There the split of the bits hangs on the last place of log2(tan()), which differs between
maths libraries (the reference's own result follows its NumPy build), not on the decoder.  Drawn angles keep a margin
of 1e-5 or more; a SEARCHED angle (theta_32_33, tiny_leaves) would sit on such an edge if the first magnitude that
gives the wanted bits were taken, so the middle one is (_mag_for_mid).  census()["floor_margin"] is the case's
smallest margin and the CPU tests assert it.

The two decoders.  k_vq_dec_frame, the default, takes a channel-frame whose trees fit its store: at most NODE_CAP
nodes (every split, leaf and half without bits of every band of every sub-block) and at most BUF_CAP doubles (pow2ceil of
the lines of every band that has a shape); the rest goes to k_vq_dec, which PACX_VQ_DEC_FRAME=0 gives every frame.  A
record drawn freely at 2..16 bits a line has 400 to 800 nodes, so in all recipes but those of HEAVY every other frame is
light: its bands are drawn in a drawn order and a band that would take the frame past the store is left uncoded.
Case.fits says which frames fit (Case.n_nodes, Case.buf), and the census is asserted on both sides: what a case's name
says must occur in frames that fit (the frame decoder sees it) and, where the recipe can, in frames beyond.

CPU only, seeded, no tests in it (tests/test_vq_code_streams.py, tests/test_gpu_vq_code_streams.py).

Seeds, as in code_streams.py: SEEDS holds, per case, the first seed from 0 at which no sample of the reference output
lies within 1e-10 * max(1, peak) of a step of the 16-bit quantiser (a hundred times the 1e-12 line bar) and at which
the case's census holds (census_ok); find_seed is how it was filled.
"""
import contextlib
import functools
import struct
from unittest import mock

import numpy as np

import pvq_model as pm
from code_streams import max_alloc, tie_exceptions
from oracle import pac_oracle as po
from oracle import pac_oracle_vq as pv

HOP, SUB, SHORT = 1024, 8, po.SHORT_LINES
THETA_LIMIT = 62                  # bits of a split angle the kernels take
GAIN_LIMIT = 64                   # bits of a gain the decoders take
NODE_CAP, BUF_CAP = 304, 1536     # k_vq_dec_frame's node store and vector buffer (VQDF_NCAP, VQDF_BUF)
# recipes whose frames are all drawn as they come: every band at one allocation, and theta_wide's few bands.  In every
# other recipe every other channel-frame is LIGHT, drawn to fit the store; in the recipes of BOTH_SIDES the frames drawn
# freely all lie beyond it, so that what the case's name says can be asked of either side
HEAVY = ("max_long", "max_short", "low_long", "node_edge", "theta_wide")
BOTH_SIDES = ("mixed", "theta_32_33", "leaf_edges", "gain_edges", "odd_bands", "random")

# name -> (hops, channels, sample rate, (nScaleBits, nMantSizeBits), use_sbr, recipe)
SPECS = {
    "mixed":            (6, 2, 48000, (4, 12), False, "mixed"),
    "max_long":         (2, 1, 48000, (4, 12), False, "max_long"),
    "max_short":        (2, 1, 48000, (4, 12), False, "max_short"),
    "max_long_sr32":    (2, 1, 32000, (4, 12), False, "max_long"),
    "max_short_sr32":   (2, 1, 32000, (4, 12), False, "max_short"),
    "low_long":         (4, 1, 48000, (4, 12), False, "low_long"),
    "node_edge":        (6, 3, 48000, (4, 12), False, "node_edge"),
    "theta_zero":       (3, 2, 48000, (4, 12), False, "theta_zero"),
    "theta_max":        (3, 2, 48000, (4, 12), False, "theta_max"),
    "theta_32_33":      (3, 2, 48000, (4, 12), False, "theta_32_33"),
    "theta_wide":       (2, 2, 48000, (4, 12), False, "theta_wide"),
    "leaf_edges":       (3, 2, 48000, (4, 12), False, "leaf_edges"),
    "tiny_leaves":      (4, 2, 48000, (4, 12), False, "tiny_leaves"),
    "tiny_leaves_sr32": (2, 2, 32000, (4, 12), False, "tiny_leaves"),
    "gain_edges":       (4, 2, 48000, (4, 12), False, "gain_edges"),
    "odd_bands":        (3, 2, 48000, (4, 12), False, "odd_bands"),
    "sbr_partial":      (3, 2, 48000, (4, 12), True, "sbr_partial"),
    "sbr_zero_env":     (3, 2, 48000, (4, 12), True, "sbr_zero_env"),
    "sbr_negative":     (3, 2, 48000, (4, 12), True, "sbr_negative"),
    "sbr_empty_low":    (3, 2, 48000, (4, 12), True, "sbr_empty_low"),
    "sbr_sparse_dense": (3, 2, 48000, (4, 12), True, "sbr_sparse_dense"),
    "sbr_sr441":        (3, 2, 44100, (4, 12), True, "sbr_some"),
    "sbr_sr32":         (3, 2, 32000, (4, 12), True, "sbr_some"),
    "ch1":              (3, 1, 48000, (4, 12), False, "random"),
    "ch3":              (3, 3, 48000, (4, 12), False, "random"),
    "one_hop":          (1, 2, 48000, (4, 12), False, "random"),
    "no_hops":          (0, 2, 48000, (4, 12), False, "random"),
    "w3_4":             (3, 2, 48000, (3, 4), False, "random"),
}
NAMES = tuple(SPECS)

SEEDS = {name: 0 for name in SPECS}
SEEDS.update({"ch3": 4, "gain_edges": 1, "leaf_edges": 1, "max_long_sr32": 1, "max_short_sr32": 1, "node_edge": 1,
              "odd_bands": 2, "sbr_negative": 1, "sbr_sparse_dense": 2, "sbr_sr32": 1, "tiny_leaves": 8,
              "tiny_leaves_sr32": 81, "w3_4": 4})                        # find_seed(name) of every case

# which omitted bands the four long blocks of an SBR case code, how their gains are drawn, what the bands below the
# cut get: (subset, gain rule of the omitted bands, allocations below the cut)
SBR_PLANS = {
    "sbr_partial":      (("first", "random", "random"), ("last", "random", "random"),
                         ("all", "random", "random"), ("none", "random", "random")),
    "sbr_zero_env":     (("all", "zero", "random"), ("first", "zero", "random"),
                         ("all", "zero_first", "random"), ("all", "zero", "random")),
    "sbr_negative":     (("all", "neg", "random"), ("first", "neg", "random"),
                         ("last", "neg", "random"), ("all", "neg", "random")),
    "sbr_empty_low":    (("all", "random", "empty"), ("first", "random", "empty"),
                         ("all", "zero", "empty"), ("last", "neg", "empty")),
    "sbr_sparse_dense": (("first", "nonzero", "random"), ("all", "nonzero", "random"),
                         ("all", "zero_first", "random"), ("last", "nonzero", "random")),
    "sbr_some":         (("some", "random", "random"), ("all", "random", "random"),
                         ("some", "random", "random"), ("none", "random", "random")),
}


NODE_EDGE_ROW = (2, 16, 3, 15, 4, 14, 5, 13, 6, 12, 7, 11, 8, 10, 9)


class Case:
    """One stream.  n_cf = hops * channels channel-frames in stream order (hop major).
      pac, header_len     the file and where its body starts
      p                   the oracle's params of the header (useVQ, useSBR, omittedBands set)
      records, sizes      payload bytes of every record and their lengths (int32 [n_cf])
      flags               uint8 [n_cf]: last | cur << 1 | next << 2 of every channel-frame
      overall             int32 [n_cf, 8], zero beyond entry 0 for a long block
      bit_alloc           int32 [n_cf, band_stride]: a long block's bands, or eight rows of nb_short
      units               per channel-frame, per (sub-)block: dict(alloc, sbr, bands=[(band, n, [node, ...])]) with nodes
                          ('split', depth, n, bits, a_theta, code, a_mid, a_side), ('zero', depth, n),
                          ('leaf', depth, n, bits, K, width, index, N) and, last, ('gain', n, width, code)
      undefined           bool [n_cf]: the record holds an angle wider than THETA_LIMIT (`theta_wide` alone)
      light               bool [n_cf]: drawn to fit the frame decoder's store
      n_nodes, buf        int [n_cf]: the frame's nodes and buffer doubles as k_vq_dec_frame counts them
      fits                bool [n_cf]: n_nodes <= NODE_CAP and buf <= BUF_CAP
    """


class Unreachable(Exception):
    """the walk met a node no well-formed record holds; the caller redraws"""


# ------------------------------------------------------------------------------------------------- the tree walk
def _theta_of(code, a_theta):
    return po.dequantize_uniform(code, a_theta) * (np.pi / 2)


def _mag_for_mid(a_theta, a_rest, half, target):
    """an angle magnitude >= 1 that leaves the mid child at most `target` bits (mid_side_alloc falls with the angle),
    or None.  Of the magnitudes that give the same mid bits as the smallest such one, the MIDDLE one is taken: at the
    first or the last of them floor() in mid_side_alloc sits, for an angle of 50 or 60 bits, within an ulp of a whole
    number, and which side log2(tan()) of another maths library falls on is rounding noise, not the decoder's doing
    (the reference's own result there hangs on its NumPy build)"""
    top = (1 << (a_theta - 1)) - 1 if a_theta >= 1 else 0
    if top < 1:
        return None

    def mid(mag):
        return pv.mid_side_alloc(a_rest, _theta_of(mag, a_theta), half)[0]

    def first_at_most(t):
        """the smallest magnitude in 1..top with mid <= t, top + 1 where there is none"""
        if mid(top) > t:
            return top + 1
        lo, hi = 1, top
        while lo < hi:
            m = (lo + hi) >> 1
            if mid(m) <= t:
                hi = m
            else:
                lo = m + 1
        return lo
    first = first_at_most(target)
    if first > top:
        return None
    return (first + first_at_most(mid(first) - 1) - 1) >> 1


class Walk:
    """the draws of one channel-frame: rng and the three rules (angle, leaf index, gain index)"""

    def __init__(self, rng, theta="random", leaf="random", gain="random", theta_limit=THETA_LIMIT, k_limit=None):
        self.rng, self.theta, self.leaf, self.gain, self.theta_limit = rng, theta, leaf, gain, theta_limit
        self.k_limit = k_limit                           # leaves of more pulses are redrawn (the reference's reach)
        self.turn = 0                                    # cycles through the targets / edge kinds of a rule

    def _below(self, n):
        return int(self.rng.integers(0, n)) if n < 1 << 62 else int(self.rng.integers(0, 1 << 62))

    # ---- angles
    def theta_code(self, a_theta, a_rest, half, attempt):
        """an angle index below 2^a_theta, or None when the rule has no other to offer"""
        rule = self.theta
        if a_theta <= 0:
            return 0 if attempt == 0 else None
        sign = int(self.rng.integers(0, 2)) << (a_theta - 1)
        top = (1 << (a_theta - 1)) - 1
        if rule == "zero":
            return 0 if attempt == 0 else None
        if rule == "max":
            return (sign | top) if attempt == 0 else None
        if rule == "search" and attempt < 5:
            # a child of exactly 32 / 33 bits (the leaf / split boundary), a side child of exactly 0 bits
            self.turn += 1
            kind, want = (("mid", 32), ("mid", 33), ("side", 32), ("side", 33), ("side", 0))[self.turn % 5]
            target = want if kind == "mid" else a_rest - want
            if 0 <= target <= a_rest:
                mag = _mag_for_mid(a_theta, a_rest, half, target)
                if mag is not None and pv.mid_side_alloc(a_rest, _theta_of(mag, a_theta), half)[0] == target:
                    return sign | mag
        if rule == "tiny" and attempt < 6:
            # leaves of 2..4 lines with all of their 32 bits: a child of `half` <= 4 lines gets exactly 32 where the
            # node can spare them; above, the bits are pushed to one side so that small nodes stay rich
            self.turn += 1
            if half <= 4 and a_rest >= 32 and (half == 2 or self.turn % 3):
                target = 32 if self.turn % 2 else a_rest - 32
                exact = True
            else:
                target = int(a_rest * (0.1, 0.3, 0.5, 0.7, 0.9)[int(self.rng.integers(0, 5))])
                exact = False
            mag = _mag_for_mid(a_theta, a_rest, half, target)
            if mag is not None and (not exact or
                                    pv.mid_side_alloc(a_rest, _theta_of(mag, a_theta), half)[0] == target):
                return sign | mag
        if attempt >= 12:
            return None
        return self._below(1 << a_theta)

    # ---- leaves
    def leaf_index(self, l, k, n):
        if k == 0:
            return 0
        rule = self.leaf
        if rule == "edges":
            self.turn += 1
            kind = self.turn % 6
            if kind == 0:
                return 0                                             # (0, ..., 0, +K)
            if kind == 1:
                return n - 1                                         # (-K, 0, ...): the last index
            if kind == 2:
                return pm.pvq_index([k] + [0] * (l - 1), k)          # (+K, 0, ...)
            if kind == 3:
                return pm.pvq_index([0] * (l - 1) + [-k], k)         # (0, ..., 0, -K)
            if kind == 4 and k >= 2 and l >= 3:
                # a vector that ends through b == xb: some pulses in front, zeros, the rest on the last component
                y = [0] * l
                a = int(self.rng.integers(1, k))
                y[int(self.rng.integers(0, l - 2))] = a if self.rng.integers(0, 2) else -a
                y[l - 1] = k - a
                return pm.pvq_index(y, k)
        if rule == "tiny" and l <= 4:
            self.turn += 1
            if self.turn % 4 == 0:
                return 0
            if self.turn % 4 == 1:
                return n - 1
        return self._below(n)

    # ---- gains
    def gain_code(self, width, rule=None):
        rule = rule or self.gain
        if width <= 0:
            return 0
        top = (1 << (width - 1)) - 1
        sign = 1 << (width - 1)
        if rule == "zero":
            return 0
        if rule == "ones":
            return sign | top
        if rule == "neg":
            return sign | self._below(top + 1)
        if rule == "nonzero":
            return (int(self.rng.integers(0, 2)) << (width - 1)) | (1 + self._below(top))
        if rule == "alternate":
            self.turn += 1
            return (0, sign | top)[self.turn % 2]
        return self._below(1 << width)


def _leaf(w, n, bits, depth):
    assert n >= 2                 # a node of one line gets no bits (see the module's header)
    k, width = pm.pulses_for_bits(n, min(32, bits))
    if w.k_limit is not None and k > w.k_limit:
        raise Unreachable("a leaf of %d pulses" % k)
    size = pm.n_vectors(n, k)
    idx = w.leaf_index(n, k, size)
    assert 0 <= idx < size <= 1 << width
    return ("leaf", depth, n, bits, k, width, idx, size)


def _shape(w, bits, n, depth):
    """oracle.split_decode with every br.get replaced by a draw -> the nodes in the order their fields are read"""
    if bits <= pv.SPLIT_BITS:
        return [_leaf(w, n, bits, depth)]
    half = -(-n // 2)
    a_theta, a_rest = pv.gain_shape_alloc(bits, half)
    if a_theta > w.theta_limit:
        raise Unreachable("an angle of %d bits" % a_theta)
    for attempt in range(16):
        code = w.theta_code(a_theta, a_rest, half, attempt)
        if code is None:
            break
        a_mid, a_side = pv.mid_side_alloc(a_rest, _theta_of(code, a_theta), half)
        try:
            out = [("split", depth, n, bits, a_theta, code, a_mid, a_side)]
            for a in (a_mid, a_side):
                if a > pv.SPLIT_BITS:
                    out += _shape(w, a, half, depth + 1)
                elif a > 0:
                    out.append(_leaf(w, half, a, depth + 1))
                else:
                    out.append(("zero", depth + 1, half))
            return out
        except Unreachable:
            continue
    raise Unreachable("no angle gives a tree")


def _band(w, alloc, n, gain_rule=None):
    """oracle.dequantize_gain_shape, drawn -> nodes, the gain last"""
    bits_gain, bits_shape = pv.gain_shape_alloc(alloc * n, n)
    nodes = _shape(w, bits_shape, n, 0) if bits_shape else []
    bits_gain += bits_shape - sum(fields(nodes)[1])
    if bits_gain > GAIN_LIMIT:
        raise Unreachable("a gain of %d bits" % bits_gain)
    nodes.append(("gain", n, bits_gain, w.gain_code(bits_gain, gain_rule)))
    assert sum(fields(nodes)[1]) == alloc * n
    return nodes


def fields(nodes):
    """(indices, widths) of a band's nodes as the writer takes them"""
    idx, wid = [], []
    for nd in nodes:
        if nd[0] == "split":
            idx.append(nd[5]), wid.append(nd[4])
        elif nd[0] == "leaf":
            idx.append(nd[6]), wid.append(nd[5])
        elif nd[0] == "gain":
            idx.append(nd[3]), wid.append(nd[2])
    return idx, wid


def _draw_band(w, alloc, n, gain_rule=None):
    """the band at `alloc`, or at the nearest lower allocation at which the rules give a tree -> (alloc, nodes);
    (0, None) where they give none at any (angle index 0 throughout sends all bits of a wide band down one path)"""
    for a in range(alloc, 1, -1):
        try:
            return a, _band(w, a, n, gain_rule)
        except Unreachable:
            continue
    return 0, None


# ------------------------------------------------------------------------------------------------- the cases
def _hop_flags(rng, recipe, hops, n_ch):
    """uint8 [hops, n_ch]"""
    if recipe == "mixed":
        fl = rng.integers(0, 8, (hops, n_ch))
        fl[0] = (0, 2)                                   # a long and a short block side by side
        return fl.astype(np.uint8)
    if recipe in ("max_long", "low_long"):
        one = rng.integers(0, 8, hops) & ~2
    elif recipe == "max_short":
        one = rng.integers(0, 8, hops) | 2
    elif recipe == "node_edge":
        fl = (rng.integers(0, 8, (hops, n_ch)) & ~2)
        fl[hops - 1, 1] |= 2                             # one short frame among the blocks of the last hop
        return fl.astype(np.uint8)
    elif recipe.startswith("sbr_"):
        one = np.array([0, 2, 4])                        # a short frame between the SBR long blocks
        one[0] |= int(rng.integers(0, 2))
        one[1] |= int(rng.integers(0, 2)) | int(rng.integers(0, 2)) << 2
    else:
        one = rng.integers(0, 8, hops)
        if hops >= 2:
            one[0] &= ~2                                 # a long and a short frame in every stream of two hops or more
            one[1] |= 2
        if recipe == "gain_edges":
            one[2] |= 2                                  # either gain rule (hop parity) on a long and on a short frame
            one[3] &= ~2
    return np.repeat(np.asarray(one)[:hops, None], n_ch, axis=1).astype(np.uint8)


def _rules(recipe, cf, n_ch):
    """(angle rule, leaf rule, gain rule, angle limit) of a channel-frame"""
    if recipe in ("theta_zero", "theta_wide"):
        return "zero", "random", "random", (1 << 30 if recipe == "theta_wide" else THETA_LIMIT)
    if recipe == "theta_max":
        return "max", "random", "random", THETA_LIMIT
    if recipe == "theta_32_33":
        return "search", "random", "random", THETA_LIMIT
    if recipe == "leaf_edges":
        return "random", "edges", "random", THETA_LIMIT
    if recipe == "tiny_leaves":
        return "tiny", "tiny", "random", THETA_LIMIT
    if recipe == "gain_edges":
        # hop 0: the sign bit on every gain; hop 1 (short): index 0 and all ones in turn; hop 2: sign bits; hop 3: in turn
        return "random", "random", ("neg", "alternate")[(cf // n_ch) % 2], THETA_LIMIT
    return "random", "random", "random", THETA_LIMIT


def _allocs(rng, recipe, cf, n_ch, cur, bands, top):
    nb = bands.nBands
    alloc = rng.choice(np.concatenate(([0], np.arange(2, top + 1))), nb)
    if recipe in ("max_long", "max_short"):
        alloc[:] = top
    elif recipe == "low_long":
        alloc[:] = (2, 3)[cf % 2]
    elif recipe == "node_edge":
        # 15 long blocks with one allocation for all bands, 2..16 from both ends inwards (so that a hop of three
        # channels holds blocks of either side), then a block far inside the node store, a short frame, a small block
        if not cur:
            alloc[:] = NODE_EDGE_ROW[cf] if cf < 15 else (2, 0, 3)[cf - 15]
    elif recipe in ("theta_zero", "theta_max", "theta_32_33", "leaf_edges", "gain_edges"):
        alloc = rng.integers(2, top + 1, nb)             # every band coded
    elif recipe == "theta_wide":
        alloc[:] = 0
        if not cur:
            alloc[-1] = top                              # the widest band with every bit on one side, again and again
            alloc[: nb // 2] = rng.integers(2, 6, nb // 2)
    elif recipe == "tiny_leaves":
        small = np.asarray(bands.nLines) <= 60
        alloc = np.where(small, rng.integers(12, top + 1, nb), rng.choice([0, 2, 3], nb))
    elif recipe == "odd_bands":
        odd = np.asarray(bands.nLines) % 2 == 1
        alloc = np.where(odd, rng.integers(4, top + 1, nb), alloc)
        if not cur:
            alloc[int(np.argmax(bands.nLines))] = top    # 363 lines at 16 bits at 48 kHz
    return alloc.astype(int)


def _build(name, seed, k_limit=None):
    hops, n_ch, sr, (n_scale, n_msb), use_sbr, recipe = SPECS[name]
    rng = np.random.default_rng([seed, NAMES.index(name), 7])
    p = po.make_params(sr, n_ch, 128, HOP, n_scale, n_msb)
    p.useVQ, p.useSBR = True, use_sbr
    p.omittedBands = [int(b) for b in po.omitted_bands(p.sfBands)] if use_sbr else []
    top = max_alloc(n_msb)
    nb_l, nb_s = p.sfBands.nBands, p.sfBandsShort.nBands
    stride = max(nb_l, SUB * nb_s)
    n_cf = hops * n_ch
    c = Case()
    c.name, c.seed, c.p, c.hops, c.n_ch, c.sample_rate, c.widths = name, seed, p, hops, n_ch, sr, (n_scale, n_msb)
    c.band_stride, c.use_sbr = stride, use_sbr
    hop_flags = _hop_flags(rng, recipe, hops, n_ch)
    c.flags = hop_flags.reshape(-1).copy()
    c.overall = np.zeros((n_cf, SUB), np.int32)
    c.bit_alloc = np.zeros((n_cf, stride), np.int32)
    c.undefined = np.zeros(n_cf, bool)
    c.light = np.zeros(n_cf, bool)
    c.n_nodes = np.zeros(n_cf, int)
    c.buf = np.zeros(n_cf, int)
    c.records, c.units = [], []
    out = [po.pac_header(p, hops * HOP)]
    c.header_len = len(out[0])
    n_long_seen = 0
    for cf in range(n_cf):
        fl = int(c.flags[cf])
        cur = (fl >> 1) & 1
        bands, nb = (p.sfBandsShort, nb_s) if cur else (p.sfBands, nb_l)
        th, lf, gn, limit = _rules(recipe, cf, n_ch)
        w = Walk(rng, th, lf, gn, limit, k_limit)
        parts, units = [], []
        c.light[cf] = recipe not in HEAVY and (cf % n_ch == 0 if n_ch > 1 else cf < 2)    # one channel: a long, a short
        room = NODE_CAP // (SUB if cur else 1)           # a light frame: the nodes a (sub-)block may take
        for s in range(SUB if cur else 1):
            overall = int(rng.integers(0, 1 << n_scale))
            alloc = _allocs(rng, recipe, cf, n_ch, cur, bands, top)
            omit_rule = None
            if use_sbr and not cur:
                subset, omit_rule, low = SBR_PLANS[recipe][n_long_seen % 4]
                n_long_seen += 1
                om = p.omittedBands
                alloc[om] = 0
                coded = {"first": om[:1], "last": om[-1:], "all": om, "none": [],
                         "some": [b for b in om if rng.integers(0, 2)] or om[-1:]}[subset]
                alloc[coded] = rng.integers(2, top + 1, len(coded))
                if low == "empty":
                    alloc[:om[0]] = 0
            elif use_sbr:
                pass                                     # a short frame of an SBR file is a plain gain-shape frame
            sbr = bool(use_sbr and not cur and any(alloc[b] for b in p.omittedBands))
            drawn = {}
            n_coded_omitted = 0
            order = [b for b in range(nb) if alloc[b]]
            if c.light[cf]:
                order = [order[i] for i in rng.permutation(len(order))]
            taken = 0
            for b in order:
                if sbr and b in p.omittedBands:
                    # ONE value: a gain of `alloc` bits and no shape
                    rule = omit_rule
                    if omit_rule == "zero_first":
                        rule = "zero" if n_coded_omitted == 0 else "nonzero"
                    n_coded_omitted += 1
                    a, nodes = int(alloc[b]), _band(w, int(alloc[b]), 1, rule)
                else:
                    a, nodes = _draw_band(w, int(alloc[b]), int(bands.nLines[b]))
                if a and c.light[cf] and taken + len(nodes) - 1 > room:
                    a = 0                                # would take the frame past the frame decoder's store
                alloc[b] = a
                if not a:
                    continue
                taken += len(nodes) - 1
                drawn[b] = (1 if (sbr and b in p.omittedBands) else int(bands.nLines[b]), nodes)
            unit_bands, indices, widths = [], [], []
            for b in sorted(drawn):
                n, nodes = drawn[b]
                i, wd = fields(nodes)
                indices.append(i), widths.append(wd)
                unit_bands.append((b, n, nodes))
                c.n_nodes[cf] += len(nodes) - 1
                if len(nodes) > 1:
                    c.buf[cf] += 1 << (n - 1).bit_length()
                if any(nd[0] == "split" and nd[4] > THETA_LIMIT for nd in nodes):
                    c.undefined[cf] = True
            c.overall[cf, s] = overall
            c.bit_alloc[cf, s * nb:(s + 1) * nb] = alloc
            parts.append((alloc, indices, widths, overall))
            units.append({"alloc": alloc, "sbr": sbr, "bands": unit_bands})
        n_bytes, payload = pv.pack_channel_block_vq(p, (fl & 1, cur, (fl >> 2) & 1), parts)
        assert n_bytes == len(payload)
        c.records.append(payload)
        c.units.append(units)
        out += [struct.pack("<L", n_bytes), payload]
    c.sizes = np.array([len(r) for r in c.records], np.int32)
    c.fits = (c.n_nodes <= NODE_CAP) & (c.buf <= BUF_CAP)
    c.pac = b"".join(out)
    return c


@functools.lru_cache(maxsize=None)
def case(name, seed=None, k_limit=None):
    """the case `name` at its fixed seed (SEEDS); another seed only for the search that fixed them.  k_limit: no leaf
    of more pulses (the angle above is redrawn): the variants the reference itself decodes in seconds, FIXTURE_CASES"""
    return _build(name, SEEDS[name] if seed is None else seed, k_limit)


# the cases tests/golden/make_vq_code_streams.py feeds to the reference's own reader and decoder, drawn with k_limit
FIXTURE_CASES = ("mixed", "gain_edges", "theta_zero", "sbr_partial")
FIXTURE_K_LIMIT = 4096


def fixture_case(name):
    return case(name, None, FIXTURE_K_LIMIT)


def longest_record_vq(sample_rate, widths=(4, 12), short=False):
    """bytes of the gain-shape record with every band at the largest allocation, by oracle.block_bits_vq and the size
    rule of oracle.pack_channel_block_vq"""
    p = po.make_params(sample_rate, 1, 128, HOP, *widths)
    bands = p.sfBandsShort if short else p.sfBands
    bits = pv.block_bits_vq(p, [max_alloc(widths[1])] * bands.nBands, short)
    return int(((SUB if short else 1) * bits + 4 + 7) // 8)


# ------------------------------------------------------------------------------ the oracle's decoder, restated
@contextlib.contextmanager
def model_leaves():
    """the oracle's three functions that are linear in K, replaced by the model's for the duration of a `with`"""
    with mock.patch.object(pv, "pulses_for_bits", pm.pulses_for_bits), \
            mock.patch.object(pv, "codebook_size", pm.n_vectors), \
            mock.patch.object(pv, "pvq_decode", lambda b, l, k: np.array(pm.pvq_decode(int(b), l, k), dtype=int)):
        yield


def decode_stream_vq(data):
    """oracle.decode_stream_vq itself, with the model's leaves -> int16 [n, nCh]"""
    with model_leaves():
        return pv.decode_stream_vq(data)


def _decode_unit(br, p, last_t, cur_t, next_t, info):
    """oracle.decode_block_vq, statement by statement, keeping the lines after sbr_reconstruct (before the division by
    2^overall) and where the reader stood after every band"""
    bands = p.sfBandsShort if cur_t else p.sfBands
    overall = br.get(p.nScaleBits)
    alloc = []
    for b in range(bands.nBands):
        a = br.get(p.nMantSizeBits)
        alloc.append(a + 1 if a else 0)
    sbr = bool(p.useSBR and not cur_t and
               np.any(np.array(alloc)[np.array(p.omittedBands, dtype=int)] != 0))
    lines = np.zeros(p.nMDCTLines, dtype=np.float64)     # oracle.decode_lines_vq with the reader's position kept
    at = 0
    ends = []
    for b in range(bands.nBands):
        n = bands.nLines[b]
        if sbr and b in p.omittedBands:
            n = 1
        if alloc[b]:
            start = br.pos
            lines[at:at + n] = pv.dequantize_gain_shape(br, int(alloc[b] * n), n)
            ends.append((b, int(alloc[b] * n), br.pos - start))
        at += n
    env_nonzero = None
    if sbr:
        cut = bands.lowerLine[p.omittedBands[0]]
        env_nonzero = int(np.count_nonzero(lines[cut:]))
        lines = pv.sbr_reconstruct(lines, p)
    info.append({"overall": overall, "alloc": alloc, "sbr": sbr, "env_nonzero": env_nonzero, "ends": ends})
    kept = lines.copy()
    lines = lines / (1. * (1 << overall))
    half_n = p.nMDCTLines
    win = po.window_table(po.window_kind(last_t, cur_t, next_t), 2 * half_n)
    return win * po.mdct_inverse(lines, half_n, half_n), kept


def decode_float_vq(data):
    """oracle.decode_stream_vq (coder/pacfile.py:231-298) up to, not including, the PCM conversion, with the model's
    leaves.  -> samples float64 [n, nCh] (fraction_to_pcm16 of them is decode_stream_vq's array), peak float64
    [n, nCh]: the larger max |block| of the two blocks that overlap at the sample, blocks float64 [n_cf, 2048], lines
    float64 [n_cf, 1024] (after SBR reconstruction where it applies, before / 2^overall; a short frame: eight rows
    of 128), info: per channel-frame the list of its (sub-)blocks' dicts and the bit at which the reader ended."""
    (sr, n_ch, _, n_lines, n_scale, n_msb, use_sbr, use_vq) = struct.unpack(
        "<LHLLHHHH", data[4:4 + struct.calcsize("<LHLLHHHH")])
    assert data[:4] == b"PAC " and use_vq and n_lines == HOP
    pos = 4 + struct.calcsize("<LHLLHHHH")
    n_bands = struct.unpack("<L", data[pos:pos + 4])[0]
    pos += 4 + 2 * n_bands
    p = po.make_params(sr, n_ch, 128, n_lines, n_scale, n_msb)
    p.useVQ, p.useSBR = True, bool(use_sbr)
    p.omittedBands = list(po.omitted_bands(p.sfBands)) if p.useSBR else []
    hop = HOP
    ola = [np.zeros(hop) for _ in range(n_ch)]
    last_peak = [0.0] * n_ch
    samples, peaks, blocks, all_lines, infos = [], [], [], [], []
    with model_leaves():
        while pos < len(data):
            hop_out, hop_peak = [], []
            for ch in range(n_ch):
                n_bytes = struct.unpack("<L", data[pos:pos + 4])[0]
                br = po.BitReader(data[pos + 4:pos + 4 + n_bytes] + b"\0" * 8)
                pos += 4 + n_bytes
                last_t, cur_t, next_t = br.get(1), br.get(1), br.get(1)
                info = []
                if not cur_t:
                    block, lines = _decode_unit(br, p, last_t, cur_t, next_t, info)
                else:
                    block = np.zeros(2 * hop)
                    lines = np.zeros(hop)
                    p.nMDCTLines = p.nSamplesPerBlock = SHORT
                    try:
                        pad = hop // 2 - SHORT // 2
                        for s, n in enumerate(range(pad, 2 * hop - SHORT - pad, SHORT)):
                            sub, ln = _decode_unit(br, p, last_t, cur_t, next_t, info)
                            block[n:n + 2 * SHORT] += sub
                            lines[s * SHORT:(s + 1) * SHORT] = ln
                    finally:
                        p.nMDCTLines = p.nSamplesPerBlock = hop
                infos.append({"units": info, "end_bit": br.pos, "n_bytes": n_bytes})
                blocks.append(block)
                all_lines.append(lines)
                pk = float(np.max(np.abs(block)))
                hop_out.append(np.add(ola[ch], block[:hop]))
                hop_peak.append(np.full(hop, max(last_peak[ch], pk)))
                ola[ch], last_peak[ch] = block[hop:], pk
            samples.append(np.stack(hop_out, axis=1))
            peaks.append(np.stack(hop_peak, axis=1))
    samples.append(np.stack(ola, axis=1))
    peaks.append(np.stack([np.full(hop, v) for v in last_peak], axis=1))
    return (np.concatenate(samples), np.concatenate(peaks), np.array(blocks).reshape(-1, 2 * hop),
            np.array(all_lines).reshape(-1, hop), infos)


# ------------------------------------------------------------------------------------------------------ census
def nodes_of(c, kind=None, cfs=None):
    """(cf, sub, band, node) of every node of a case, or of the nodes of one kind, or of some channel-frames"""
    for cf, units in enumerate(c.units):
        if cfs is not None and cf not in cfs:
            continue
        for s, u in enumerate(units):
            for (b, n, nodes) in u["bands"]:
                for nd in nodes:
                    if kind is None or nd[0] == kind:
                        yield cf, s, b, nd


def sides(c):
    """(channel-frames that fit the frame decoder's store, channel-frames beyond it)"""
    return [cf for cf in range(len(c.flags)) if c.fits[cf]], [cf for cf in range(len(c.flags)) if not c.fits[cf]]


def _floor_margin(nd):
    """how far the argument of floor() in mid_side_alloc lies from a whole number at a split (0.5 where nothing hangs
    on it: angle 0, no bits to share, or an argument outside [0, a_rest + 1], which the clamp decides)"""
    _, _, n, _, a_theta, code, a_mid, a_side = nd
    half, a_rest = -(-n // 2), a_mid + a_side
    theta = _theta_of(code, a_theta) if a_theta > 0 else 0
    if theta == 0 or a_rest == 0 or half == 1:
        return 0.5
    v = (a_rest - (half - 1) * np.log2(np.tan(abs(theta)) + pv.EPS)) / 2
    return abs(v - round(v)) if -1 <= v <= a_rest + 1 else 0.5


def leaf_kinds(c, cfs=None):
    """how many leaves with pulses hold each edge `leaf_edges` draws"""
    got = {"first": 0, "last": 0, "+K first": 0, "-K first": 0, "+K last": 0, "-K last": 0, "b == xb": 0}
    for _, _, _, (_, _, n, _, k, _, idx, size) in nodes_of(c, "leaf", cfs):
        if not k:
            continue
        y = pm.pvq_decode(idx, n, k)
        got["first"] += idx == 0
        got["last"] += idx == size - 1
        got["+K first"] += y[0] == k
        got["-K first"] += y[0] == -k
        got["+K last"] += y[-1] == k
        got["-K last"] += y[-1] == -k
        front = [v for v in y[:-1] if v]
        got["b == xb"] += len(front) == 1 and y[-1] > 0 and y[-2] == 0     # pulses in front, zeros, the rest at the end
    return got


def census(c, cfs=None):
    """what a case's records hold, or those of the channel-frames `cfs`"""
    leaves = [nd for _, _, _, nd in nodes_of(c, "leaf", cfs)]
    splits = [nd for _, _, _, nd in nodes_of(c, "split", cfs)]
    gains = [nd for _, _, _, nd in nodes_of(c, "gain", cfs)]
    units = [u for cf, units in enumerate(c.units) if cfs is None or cf in cfs for u in units]
    top = {l: pm.pulses_for_bits(l, 32)[0] for l in (2, 3, 4)}
    return {
        "flags": set(int(f) for cf, f in enumerate(c.flags) if cfs is None or cf in cfs),
        "alloc": set(int(a) for u in units for a in u["alloc"]),
        "overall": set(int(c.overall[cf, s]) for cf, us in enumerate(c.units) for s in range(len(us))),
        "mod4": set(int(n) % 4 for n in c.sizes),
        "k0_leaves": sum(1 for nd in leaves if nd[4] == 0),
        "zero_children": sum(1 for _ in nodes_of(c, "zero", cfs)),
        "mid_bits": [nd[6] for nd in splits],
        "side_bits": [nd[7] for nd in splits],
        "all_angle_nodes": sum(1 for nd in splits if nd[2] == 2),           # 2 lines, > 32 bits: the angle takes them all
        "theta_bits": set(nd[4] for nd in splits),
        "split_depths_odd": set(nd[1] for nd in splits if nd[2] % 2),
        "full_tiny_tables": set((nd[2], "short" if c.flags[cf] & 2 else "long")
                                for cf, _, _, nd in nodes_of(c, "leaf", cfs) if nd[2] <= 4 and nd[4] == top[nd[2]]),
        "tiny_ends": set((nd[2], "first" if nd[6] == 0 else "last") for nd in leaves
                         if nd[2] <= 4 and nd[4] == top[nd[2]] and nd[6] in (0, nd[7] - 1)),
        "gain_bits": set(nd[2] for nd in gains),
        "gain_negative": sum(1 for nd in gains if nd[2] and nd[3] >> (nd[2] - 1)),
        "gain_zero": sum(1 for nd in gains if nd[3] == 0),
        "gain_ones": sum(1 for nd in gains if nd[2] and nd[3] == (1 << nd[2]) - 1),
        "gains": len(gains),
        "sbr_blocks": sum(1 for u in units if u["sbr"]),
        "floor_margin": min([_floor_margin(nd) for nd in splits], default=0.5),
    }


def searched(got):
    """how often each child `theta_32_33` searches for occurs in a census"""
    return {"mid 32": got["mid_bits"].count(32), "mid 33": got["mid_bits"].count(33),
            "side 32": got["side_bits"].count(32), "side 33": got["side_bits"].count(33),
            "side 0": sum(1 for m, sd in zip(got["mid_bits"], got["side_bits"]) if sd == 0 and m > 0)}


def census_ok(c):
    """what find_seed asks of a seed besides the tie condition (tests/test_vq_code_streams.py asserts the same, and
    more, case by case): no angle on a rounding edge, and what the case's name says on both sides of the frame
    decoder's store"""
    got = census(c)
    if got["floor_margin"] < 1e-9:
        return False
    fit, beyond = sides(c)
    recipe = SPECS[c.name][5]
    both = recipe in BOTH_SIDES and len(c.flags) >= 2
    if recipe not in HEAVY and len(c.flags):
        if not c.fits[c.light].all() or (both and c.fits[~c.light].any()):
            return False
        for side in ([fit, beyond] if both and c.n_ch > 1 else [fit]):
            if c.hops >= 2 and not {0, 2} <= set(int(c.flags[cf]) & 2 for cf in side):
                return False                             # long and short frames on the side
    if c.name == "mixed":
        differ = any(len(set(c.flags[h * c.n_ch:(h + 1) * c.n_ch].tolist())) > 1 for h in range(c.hops))
        return got["flags"] == set(range(8)) and differ and got["mod4"] == {0, 1, 2, 3} and \
            got["alloc"] == {0} | set(range(2, max_alloc(c.widths[1]) + 1))
    if c.name == "theta_32_33":
        return all(min(searched(census(c, side)).values()) >= 2 for side in (fit, beyond))
    if c.name == "leaf_edges":
        return all(min(leaf_kinds(c, side).values()) >= 10 for side in (fit, beyond))
    if c.name == "odd_bands":
        return census(c, fit)["split_depths_odd"] >= set(range(5))
    if c.name.startswith("tiny_leaves"):
        return len(census(c, fit)["full_tiny_tables"]) == 6 and len(census(c, fit)["tiny_ends"]) == 6 and \
            len(got["full_tiny_tables"]) == 6
    return True


def find_seed(name, limit=1000):
    """how SEEDS was filled: the first seed without a tie and with the case's census"""
    for seed in range(limit):
        c = _build(name, seed)
        if not census_ok(c):
            continue
        samples, peak = decode_float_vq(c.pac)[:2]
        if tie_exceptions(samples, peak) == 0:
            return seed
    raise RuntimeError(f"{name}: no clean seed below {limit}")
