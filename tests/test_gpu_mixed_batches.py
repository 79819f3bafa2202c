"""Block-switched batches at the sizes where the frame lists and the persistent walks loop (tests/mixed_batches.py).

In a batch given as PcmView.frames(blocks) a frame's output rows depend on its own samples and its flag byte alone (and,
for the dropped-hop rule, on the other channels of the same frame).  So:

  (a) the ATOM BATCH -- every item (atom, flag byte), 88 frames in one call -- is held to the oracle: payload bytes of
      the scalar coder and of both gain-shape configurations, the scalar coder's integer codes as well;
  (b..h) batches of 1 to 40 000 frames drawn from the items must reproduce the atom batch's rows, gathered on the
      device and compared with torch.equal.  Integers, bytes, and doubles the same kernel made from the same input:
      there is no tolerance anywhere in this file.

Every call writes into buffers filled with 0xFF, so a row no kernel wrote -- a frame missing from both lists, a list
walked short -- shows as a mismatch.  What (b..h) catch is a defect of list building (k_frame_lists_small: one thread
owns ceil(n / 256) frames; k_frame_lists above 16 384 frames: ballots and atomics), of a walk through cf_list /
cf_count (k_mdct_long_v2, k_mask<1024> / k_mask<128>, k_tail_short, the gain-shape coders) or of the ordering of the
long and the short chain on their two streams -- not of the arithmetic, which (a) and the rest of the suite pin.
"""
import os

import numpy as np
import pytest

import mixed_batches as mb
from oracle import pac_oracle as po

pytestmark = pytest.mark.gpu

SCALAR_OUT = ("overall", "scale_factor", "bit_alloc", "mantissa", "status", "n_bytes", "payload")
VQ_OUT = ("overall", "bit_alloc", "status", "n_bytes", "payload")
CAP_RATE = 128 / 48.0
MAX_CH = mb.MAX_CH
ENV = ("PACX_SPLIT_SHORT", "PACX_FUSE_TAIL", "PACX_VQ_FUSE_ALLOC", "PACX_VQ_FRAME")


@pytest.fixture(scope="module")
def A():
    import audio_codec_amd as a
    a.load()
    return a


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture
def fresh_handles(A):
    A.context.clear()
    yield
    A.context.clear()


# ------------------------------------------------------------------------------------------------ handles and calls
def handle(A, name):
    h = mb.HANDLES[name]
    return A.context.encoder(mb.SR, h["kbps"] / 48.0, use_vq=h["use_vq"], use_sbr=h["use_sbr"])


def new_handle(A, name):
    h = mb.HANDLES[name]
    return A.engine.Encoder(mb.SR, h["kbps"] / 48.0, use_vq=h["use_vq"], use_sbr=h["use_sbr"])


def filled(torch, out):
    """every buffer of an output dict set to 0xFF bytes"""
    for t in out.values():
        if hasattr(t, "view"):
            t.view(torch.uint8).fill_(0xFF)
    return out


def finish(torch, out, keys):
    """the outputs named, as integers (doubles by their bits), payload bytes past n_bytes zeroed"""
    torch.cuda.synchronize()
    res = {}
    for k in keys:
        t = out[k]
        if k == "payload":
            used = torch.arange(t.shape[1], device=t.device)[None, :] < out["n_bytes"][:, None]
            t = torch.where(used, t, torch.zeros_like(t))
        res[k] = t.view(torch.int64) if t.dtype == torch.float64 else t
    return res


def encode_pack(torch, enc, view, flags):
    out = filled(torch, enc.alloc_outputs(view.n_cf, with_payload=True))
    return finish(torch, enc.encode_pack(view, flags, out, want_mantissa=True), SCALAR_OUT)


def encode_vq(torch, enc, view, flags):
    out = filled(torch, enc.alloc_vq_outputs(view.n_cf))
    return finish(torch, enc.encode_vq(view, flags, out), VQ_OUT)


ENCODE = {"scalar": encode_pack, "vq128": encode_vq, "vq96": encode_vq}


# --------------------------------------------------------------------------------------------------- batches
_DEV = {}


def atoms_on(torch, device, n_ch):
    key = ("atoms", n_ch)
    if key not in _DEV:
        _DEV[key] = torch.as_tensor(mb.atoms(n_ch).copy(), device=device)
    return _DEV[key]


def batch(A, torch, device, n_ch, item):
    """(frames view of the items, flags tensor, rows [n_cf] of the atom batch to expect)"""
    it = torch.as_tensor(item.astype(np.int64), device=device)
    blocks = atoms_on(torch, device, n_ch)[it // 8].contiguous()
    flags = (it % 8).to(torch.uint8)
    rows = (it[:, None] * n_ch + torch.arange(n_ch, device=device)[None, :]).reshape(-1)
    return A.engine.PcmView.frames(blocks), flags, rows


def atom_rows(A, torch, name, n_ch):
    """the atom batch through the default handle of this name, once per module: the expectation of (b..h)"""
    key = ("rows", name, n_ch)
    if key not in _DEV:
        enc = handle(A, name)
        view, flags, _ = batch(A, torch, enc.device, n_ch, np.arange(mb.N_ITEMS))
        _DEV[key] = ENCODE[name](torch, enc, view, flags)
    return _DEV[key]


def assert_rows(torch, got, want, rows, item, n_ch, what):
    """got[k] == want[k][rows] for every output; the failure names the first frame that differs"""
    for k in got:
        exp = want[k][rows]
        assert got[k].shape == exp.shape and got[k].dtype == exp.dtype, (what, k)
        if not torch.equal(got[k], exp):
            bad = (got[k] != exp).reshape(len(rows), -1).any(dim=1).nonzero().flatten()
            r = int(bad[0])
            f, i = r // n_ch, int(item[r // n_ch])
            raise AssertionError(f"{what}: {k}: {len(bad)} of {len(rows)} rows differ from the atom batch; the first is "
                                 f"frame {f} channel {r % n_ch}: atom {mb.ATOMS[i // 8]}, flag byte {i % 8}")


def assert_same(torch, a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, "a second run gave other bits")


# ------------------------------------------------------------------------------------- (a) the atoms and the oracle
def zero_subblock(n_ch):
    """bool [N_ITEMS, n_ch]: the channel holds an all-zero sub-block (samples 448 + 128 j ... + 256) and is coded short"""
    a = mb.atoms(n_ch)
    zero = np.array([[any(not a[k, ch, 448 + 128 * j:448 + 128 * j + 256].any() for j in range(8)) for ch in range(n_ch)]
                     for k in range(mb.N_ATOMS)])
    return np.repeat(zero, 8, axis=0) & ((np.arange(mb.N_ITEMS) & 2) != 0)[:, None]


def check_records(A, got, records, n_ch, what):
    """payload bytes against the oracle's records.  A dropped hop: n_bytes 0 and PACX_ST_ZERO_SUBBLOCK in every
    channel, whichever channel holds the all-zero sub-block"""
    n_bytes, payload, status = (got[k].cpu().numpy() for k in ("n_bytes", "payload", "status"))
    assert len(n_bytes) == mb.N_ITEMS * n_ch
    zero = zero_subblock(n_ch)
    for i, recs in enumerate(records):
        assert (recs is None) == bool(zero[i].any()), (what, i)
        for ch in range(n_ch):
            r = i * n_ch + ch
            st = int(status[r]) & 0xFFFFFFFF
            assert (st & A._lib.ST_SHORT != 0) == bool(i & 2), (what, i, ch, st)
            assert bool(st & A._lib.ST_ZERO_SUBBLOCK) == (recs is None), (what, i, ch, st)
            if recs is None:
                assert n_bytes[r] == 0, (what, "dropped hop", i, ch, st)
            else:
                assert payload[r, :n_bytes[r]].tobytes() == recs[ch], (what, mb.ATOMS[i // 8], i % 8, ch)


@pytest.mark.parametrize("n_ch", [1, 2, 3])
@pytest.mark.parametrize("name", list(mb.HANDLES))
def test_dropped_hop_status_in_every_channel(A, torch, name, n_ch):
    """(a) a dropped hop has n_bytes == 0 AND PACX_ST_ZERO_SUBBLOCK in EVERY channel: the dropped-hop atom is silent
    in channel 0 alone.  This test found k_mdct_short setting the bit per channel-frame (status 3, 1 for the stereo
    atom, 3, 1, 1 for three channels, n_bytes 0 throughout); it now looks at the sibling channels as well."""
    _, records = mb.oracle_items(name, n_ch)
    got = atom_rows(A, torch, name, n_ch)
    n_bytes, status = got["n_bytes"].cpu().numpy(), got["status"].cpu().numpy()
    silent_elsewhere = 0
    for i, recs in enumerate(records):
        if recs is None:
            for ch in range(n_ch):
                r = i * n_ch + ch
                assert n_bytes[r] == 0 and int(status[r]) & A._lib.ST_ZERO_SUBBLOCK, (name, mb.ATOMS[i // 8], i % 8, ch)
                silent_elsewhere += not zero_subblock(n_ch)[i, ch]
    assert silent_elsewhere == (4 * (n_ch - 1))                # the four short flag bytes of the dropped-hop atom


@pytest.mark.parametrize("n_ch", [1, 2, 3])
@pytest.mark.parametrize("name", list(mb.HANDLES))
def test_atom_batch_against_the_oracle(A, torch, name, n_ch):
    """(a) every item in one batch of 88 frames: the payload bytes up to n_bytes are the oracle's record; a dropped
    hop has n_bytes 0 and PACX_ST_ZERO_SUBBLOCK in every channel.  Scalar handle: the codes of encode() as well."""
    parts, records = mb.oracle_items(name, n_ch)
    got = atom_rows(A, torch, name, n_ch)
    check_records(A, got, records, n_ch, f"{name} {n_ch} ch")
    assert sum(r is None for r in records) == 8
    if name != "scalar":
        return
    enc = handle(A, name)
    view, flags, _ = batch(A, torch, enc.device, n_ch, np.arange(mb.N_ITEMS))
    out = enc.encode(view, flags, filled(torch, enc.alloc_outputs(view.n_cf)))
    torch.cuda.synchronize()
    for label, res in (("encode", out), ("encode_pack", got)):
        host = {k: res[k].cpu().numpy() for k in ("overall", "scale_factor", "bit_alloc", "mantissa", "status")}
        for i, q in enumerate(parts):
            for ch in range(n_ch):
                r = i * n_ch + ch
                assert bool(int(host["status"][r]) & A._lib.ST_ZERO_SUBBLOCK) == (q is None), (label, i, ch)
                if q is None:
                    continue
                for j, (sf, alloc, mant, overall) in enumerate(q[ch]):
                    c = A.codec.unpack_short(enc, host, r, j) if i & 2 else A.codec.unpack_long(enc, host, r)
                    assert c[3] == overall and c[1].tolist() == list(alloc), (label, mb.ATOMS[i // 8], i % 8, ch, j)
                    assert c[0].tolist() == sf.tolist() and c[2].tolist() == mant.tolist(), \
                        (label, mb.ATOMS[i // 8], i % 8, ch, j)


# ------------------------------------------------------------------------- (b) every pattern, every size, twice
def check_pattern(A, torch, name, n, n_ch, handles=tuple(mb.HANDLES), encs=None):
    item, _ = mb.pattern(name, n)
    for h in handles:
        enc = encs[h] if encs else handle(A, h)
        want = atom_rows(A, torch, h, n_ch) if not encs else _DEV[("rows", h, n_ch)]
        view, flags, rows = batch(A, torch, enc.device, n_ch, item)
        first = ENCODE[h](torch, enc, view, flags)
        assert_rows(torch, first, want, rows, item, n_ch, f"{h} {name} {n} frames x {n_ch} ch")
        second = ENCODE[h](torch, enc, view, flags)
        assert_same(torch, first, second, f"{h} {name} {n} frames x {n_ch} ch")
        del first, second, view, rows


@pytest.mark.parametrize("n_ch", [1, 2])
@pytest.mark.parametrize("name", mb.PATTERNS)
def test_small_list_kernel_sizes(A, torch, name, n_ch):
    """(b) 1 to 4097 frames (k_frame_lists_small: per = 1 up to 256 frames, then 2, 4, 5, 17 frames per thread)"""
    for n in mb.SIZES_SMALL:
        check_pattern(A, torch, name, n, n_ch)


@pytest.mark.parametrize("n_ch", [1, 2])
@pytest.mark.parametrize("n", mb.SIZES_LARGE)
@pytest.mark.parametrize("name", mb.PATTERNS)
def test_both_list_kernels_at_their_border(A, torch, name, n, n_ch):
    """(b) 16 383 and 16 384 frames (k_frame_lists_small with 64 frames per thread), 16 385 and 40 000 (k_frame_lists);
    every persistent kernel loops"""
    check_pattern(A, torch, name, n, n_ch)


@pytest.mark.parametrize("n", [257, 16385])
@pytest.mark.parametrize("name", mb.PATTERNS)
def test_three_channels(A, torch, name, n):
    check_pattern(A, torch, name, n, 3)


# ------------------------------------------------------------------------------------------ (c) degenerate lists
@pytest.mark.parametrize("n", [257, 16385])
@pytest.mark.parametrize("name", list(mb.HANDLES))
def test_flags_without_a_short_frame(A, torch, name, n):
    """(c) counts[1] == 0: a flags array whose cur bits are all 0 against the same batch with flags=None, in every
    output, on the frames whose flag byte is 0 (the others take a start or stop window)"""
    enc = handle(A, name)
    item, fl = mb.pattern("flags_all_long", n)
    view, flags, rows = batch(A, torch, enc.device, 2, item)
    with_flags = ENCODE[name](torch, enc, view, flags)
    without = ENCODE[name](torch, enc, view, None)
    sel = torch.as_tensor(np.repeat(fl == 0, 2), device=enc.device)
    assert int(sel.sum()) >= n // 4
    for k in with_flags:
        assert torch.equal(with_flags[k][sel], without[k][sel]), (name, n, k)
    assert_rows(torch, with_flags, atom_rows(A, torch, name, 2), rows, item, 2, f"{name} flags_all_long {n}")


@pytest.mark.parametrize("n", [257, 16385])
def test_no_long_frame(A, torch, n):
    """(c) counts[0] == 0: every frame short-coded, the rows of (a)"""
    check_pattern(A, torch, "all_short", n, 2)
    item, fl = mb.pattern("all_short", n)
    assert (fl & 2).all()


# ------------------------------------------------------------------------------------------ (d) routing overrides
@pytest.mark.parametrize("n", [257, 16385])
@pytest.mark.parametrize("env", ENV)
def test_routing_overrides(A, torch, monkeypatch, fresh_handles, env, n):
    """(d) one stream instead of two, the long tail as a kernel of its own, BitAlloc behind the gain-shape mask kernel,
    k_vq over every unit: the rows of the default handles' atom batch.  The overrides are read when a handle is made."""
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    for h in mb.HANDLES:
        _DEV.pop(("rows", h, 2), None)
        atom_rows(A, torch, h, 2)                  # default handles, made before the override is set
    monkeypatch.setenv(env, "0")
    encs = {h: new_handle(A, h) for h in mb.HANDLES}
    try:
        for name in ("random50", "dropped_mix"):
            check_pattern(A, torch, name, n, 2, encs=encs)
    finally:
        for e in encs.values():
            e.close()


# ------------------------------------------------------------------------------------ (e) paths that are not fast
@pytest.mark.parametrize("kind", ["float64", "offset_by_one_sample"])
@pytest.mark.parametrize("name", ["random50", "dropped_mix"])
def test_generic_views(A, torch, name, kind):
    """(e) 257 stereo frames as float64 fractions (the oracle's own pcm16_to_fraction values) and as int16 one sample
    off the 16-byte alignment: check_pcm keeps `fast` false, the chain runs unsplit on the generic kernels"""
    n, n_ch = 257, 2
    item, fl = mb.pattern(name, n)
    frames = mb.atoms(n_ch)[item // 8]
    for h in mb.HANDLES:
        enc = handle(A, h)
        _, flags, rows = batch(A, torch, enc.device, n_ch, item)
        if kind == "float64":
            blocks = torch.as_tensor(po.pcm16_to_fraction(frames), device=enc.device)
            assert blocks.dtype == torch.float64
            view = A.engine.PcmView.frames(blocks)
        else:
            flat = torch.zeros(frames.size + 8, dtype=torch.int16, device=enc.device)
            flat[1:1 + frames.size] = torch.as_tensor(frames.reshape(-1).copy(), device=enc.device)
            assert flat.data_ptr() % 16 == 0
            view = A.engine.PcmView(flat[1:], n_ch, n, n_ch * mb.N, mb.N, 1)
            assert view.c.data % 16 == 2
        got = ENCODE[h](torch, enc, view, flags)
        assert_rows(torch, got, atom_rows(A, torch, h, n_ch), rows, item, n_ch, f"{h} {name} {kind}")


# ------------------------------------------------------------------------------------ (f) the stream layout at scale
PERIOD, STREAM_HOPS = 24, 16385 + 1


def test_stream_layout_at_scale(A, torch):
    """(f) 24 stereo hops of the castanet excerpt, tiled to 16 386 hops in pacfile.device_stream's layout: the
    detector's transients are periodic and are detect_transients.hop_transients' of one period, and every frame's rows
    are those of the same frame one period in"""
    pcm = np.load(os.path.join(mb.HERE, "golden", "excerpt_castanet.npz"))["pcm"][:PERIOD * mb.HOP]
    assert pcm.shape == (PERIOD * mb.HOP, 2)
    hops = pcm.reshape(PERIOD, mb.HOP, 2).transpose(0, 2, 1)
    one = A.detect_transients.hop_transients(po.pcm16_to_fraction(hops))
    look = np.concatenate((po.pcm16_to_fraction(hops), np.zeros(hops.shape)), axis=2)
    assert one.tolist() == [bool(po.transient_detect(b)) for b in look]
    switches = int(np.sum(one & ~np.roll(one, 1)))                     # 0 -> 1 in the wrapped period
    assert switches >= 4, switches
    enc = handle(A, "scalar")
    n_hops = STREAM_HOPS
    planar = torch.zeros((2, (n_hops + 3) * mb.HOP), dtype=torch.int16, device=enc.device)
    period = torch.as_tensor(np.ascontiguousarray(pcm.T), device=enc.device)
    tiled = period.repeat(1, -(-n_hops // PERIOD))[:, :n_hops * mb.HOP]
    planar[:, mb.HOP:(n_hops + 1) * mb.HOP] = tiled
    planar[:, (n_hops + 1) * mb.HOP:(n_hops + 2) * mb.HOP] = tiled[:, -mb.HOP:]
    tr, fl = enc.transient_flags(planar, n_hops)
    tr_h, fl_h = tr.cpu().numpy(), fl.cpu().numpy()
    assert tr_h.shape == (n_hops,) and fl_h.shape == (n_hops + 2,)
    assert np.array_equal(tr_h[2 * PERIOD:], tr_h[PERIOD:-PERIOD])              # periodic from the third period on
    assert np.array_equal(tr_h != 0, one[np.arange(n_hops) % PERIOD])
    t = np.concatenate(([0, 0], tr_h != 0, [0])).astype(np.uint8)               # k_stream_flags: T[f-2], T[f-1], T[f]
    assert np.array_equal(fl_h[:n_hops + 1], t[:n_hops + 1] | t[1:n_hops + 2] << 1 | t[2:n_hops + 3] << 2)
    assert fl_h[n_hops + 1] == 0
    view = A.engine.PcmView.stream(planar)
    assert view.n_frames == n_hops + 2
    f = torch.arange(PERIOD, n_hops, device=enc.device)
    src = PERIOD + f % PERIOD
    cf, cf_src = [(x[:, None] * 2 + torch.arange(2, device=enc.device)[None, :]).reshape(-1) for x in (f, src)]
    assert torch.equal(fl[f], fl[src])
    for h in mb.HANDLES:
        got = ENCODE[h](torch, handle(A, h), view, fl)
        assert int((got["status"] & A._lib.ST_SHORT != 0).sum()) >= 2 * 4 * (n_hops // PERIOD)
        for k in got:
            assert torch.equal(got[k][cf], got[k][cf_src]), (h, k)


# ------------------------------------------------------------------------------- (g) the second passes and curves
def second_passes(A, torch, enc, view, flags, given_rows):
    """encode_pack_budget / _alloc with the budgets and allocations of `given_rows` (drawn per atom-batch row),
    encode_pack_nmr at -3 dB, band_curve and rate_curve at the 128 kb/s cap -> {what: outputs}"""
    n_cf = view.n_cf
    rng = np.random.default_rng(5)
    budget = torch.as_tensor(rng.integers(0, 3000, (mb.N_ITEMS * MAX_CH, 8)).astype(np.int32), device=enc.device)
    alloc = torch.as_tensor(rng.integers(0, 13, (mb.N_ITEMS * MAX_CH, enc.band_stride)).astype(np.int32),
                            device=enc.device)
    res = {}
    out = filled(torch, enc.alloc_outputs(n_cf, with_payload=True))
    res["budget"] = finish(torch, enc.encode_pack_budget(view, flags, budget[given_rows], out, want_mantissa=True),
                           SCALAR_OUT)
    out = filled(torch, enc.alloc_outputs(n_cf, with_payload=True))
    res["alloc"] = finish(torch, enc.encode_pack_alloc(view, flags, alloc[given_rows], out, want_mantissa=True),
                          SCALAR_OUT)
    out = filled(torch, enc.alloc_outputs(n_cf, with_payload=True))
    out["budget"] = torch.full((n_cf, 8), -1, dtype=torch.int32, device=enc.device)
    res["nmr"] = finish(torch, enc.encode_pack_nmr(view, flags, -3.0, CAP_RATE, out, want_mantissa=True),
                        SCALAR_OUT + ("budget",))
    shapes = {"nmr": (n_cf, enc.band_stride, A._lib.BAND_CAND), "cap": (n_cf, 8), "cap_alloc": (n_cf, enc.band_stride)}
    out = filled(torch, {"nmr": torch.empty(shapes["nmr"], dtype=torch.float64, device=enc.device),
                         "cap": torch.empty(shapes["cap"], dtype=torch.int32, device=enc.device),
                         "cap_alloc": torch.empty(shapes["cap_alloc"], dtype=torch.int32, device=enc.device)})
    res["band_curve"] = finish(torch, enc.band_curve(view, flags, CAP_RATE, out), ("nmr", "cap", "cap_alloc"))
    row, _ = enc.rate_curve_layout(CAP_RATE)
    out = filled(torch, {"worst": torch.empty((n_cf, row), dtype=torch.float64, device=enc.device),
                         "bits": torch.empty((n_cf, row), dtype=torch.int32, device=enc.device),
                         "steps": torch.empty((n_cf, 8), dtype=torch.int32, device=enc.device)})
    res["rate_curve"] = finish(torch, enc.rate_curve(view, flags, CAP_RATE, out), ("worst", "bits", "steps"))
    return res


@pytest.mark.parametrize("n", [257, 16385])
def test_second_passes_and_curves(A, torch, n):
    """(g) random50, stereo: every row of the five calls equals the item's row of the same call on the atom batch"""
    enc = handle(A, "scalar")
    n_ch = 2
    key = ("second", n_ch)
    if key not in _DEV:
        view, flags, rows = batch(A, torch, enc.device, n_ch, np.arange(mb.N_ITEMS))
        _DEV[key] = second_passes(A, torch, enc, view, flags, rows)
    want = _DEV[key]
    item, _ = mb.pattern("random50", n)
    view, flags, rows = batch(A, torch, enc.device, n_ch, item)
    got = second_passes(A, torch, enc, view, flags, rows)
    for what in got:
        assert_rows(torch, got[what], want[what], rows, item, n_ch, f"{what} random50 {n}")
    # the calls are worth comparing: budgets were found, curves have steps, the drawn allocations were coded
    assert (want["nmr"]["budget"] > 0).any() and (want["rate_curve"]["steps"] > 0).any()
    assert (want["band_curve"]["cap"] > 0).any() and (want["alloc"]["n_bytes"] > 0).any()


# -------------------------------------------------------------------------------------------------- (h) the way back
def way_back(A, torch, name, enc, view, flags, n_ch):
    """encode -> gather_body -> index_body -> unpack / decode (want_blocks); scalar: NMR of every row as well"""
    got = ENCODE[name](torch, enc, view, flags)
    out = filled(torch, enc.alloc_vq_outputs(view.n_cf) if name != "scalar" else
                 enc.alloc_outputs(view.n_cf, with_payload=True))
    out = enc.encode_vq(view, flags, out) if name != "scalar" else enc.encode_pack(view, flags, out)
    body, total = enc.gather_body(out["payload"], out["n_bytes"])
    total = int(total.item())
    offsets, n_bytes, result = enc.index_body(body[:total], n_ch)
    n_rec, used, broke = (int(x) for x in result.cpu().numpy())
    res = {"got": got, "n_rec": n_rec, "total": total, "used": used, "broke": broke,
           "offsets": offsets[:n_rec], "rec_bytes": n_bytes[:n_rec]}
    if name == "scalar":
        codes = enc.unpack(body[:total], n_bytes[:n_rec], offsets[:n_rec])
        res["flags"] = codes["flags"]
        res["blocks"] = enc.decode(codes, n_ch, want_blocks=True, want_pcm=False).view(torch.int64)
        slot = enc.unpack(out["payload"], out["n_bytes"])
        extra = {}
        enc.decode(slot, n_ch, want_pcm=False, extra=extra)
        status = (out["status"] | slot["status"] | extra["status"]) & A.quality._NO_PAYLOAD
        status = torch.where(out["n_bytes"] > 0, status, torch.full_like(status, A._lib.ST_ZERO_SUBBLOCK))
        nmr = enc.nmr(view, flags, extra["lines"], slot["overall"], status)
        res["nmr"] = {k: nmr[k].view(torch.int64) for k in ("noise", "mask", "nmr_db")}
        res["nan"] = torch.isnan(nmr["nmr_db"])
    else:
        dec = enc.decode_vq(body[:total], n_bytes[:n_rec], n_ch, offsets=offsets[:n_rec], want_blocks=True,
                            want_pcm=False)
        res["flags"] = dec["flags"]
        res["blocks"] = dec["blocks"].view(torch.int64)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", list(mb.HANDLES))
def test_the_way_back(A, torch, name):
    """(h) dropped_mix, 16 385 stereo frames: index_body finds exactly the records of the hops that were not dropped,
    unpack / decode_vq return the flags given, every decoded block is the atom batch's bit for bit, and the NMR rows
    are the atom batch's, NaN placement included"""
    n, n_ch = 16385, 2
    enc = handle(A, name)
    key = ("back", name)
    if key not in _DEV:
        view, flags, _ = batch(A, torch, enc.device, n_ch, np.arange(mb.N_ITEMS))
        _DEV[key] = way_back(A, torch, name, enc, view, flags, n_ch)
    want = _DEV[key]
    dropped_item = np.array([(i // 8 in (mb.DROP, mb.ZEROS)) and bool(i & 2) for i in range(mb.N_ITEMS)])
    assert want["n_rec"] == n_ch * int((~dropped_item).sum()) and want["broke"] == -1
    item, fl = mb.pattern("dropped_mix", n)
    view, flags, rows = batch(A, torch, enc.device, n_ch, item)
    got = way_back(A, torch, name, enc, view, flags, n_ch)
    assert_rows(torch, got["got"], want["got"], rows, item, n_ch, f"{name} dropped_mix {n}")
    kept_frames = ~dropped_item[item]
    assert 0.8 * n < kept_frames.sum() < 0.9 * n                       # an eighth of the hops is dropped
    kept = torch.as_tensor(np.repeat(kept_frames, n_ch), device=enc.device)
    assert torch.equal(got["got"]["n_bytes"] > 0, kept)
    # the record index: the kept channel-frames in order, nothing else
    assert got["n_rec"] == int(kept.sum()) and got["broke"] == -1 and got["used"] == got["total"]
    want_bytes = got["got"]["n_bytes"][kept]
    assert torch.equal(got["rec_bytes"], want_bytes)
    assert torch.equal(got["offsets"], torch.cumsum(want_bytes.to(torch.int64) + 4, 0) - want_bytes)
    assert torch.equal(got["flags"], flags.repeat_interleave(n_ch)[kept])
    # decoded blocks: record j of the batch is row rows[kept][j] of the atom batch, which is that batch's record
    # number (kept rows before it)
    kept_atom = torch.as_tensor(np.repeat(~dropped_item, n_ch), device=enc.device)
    record_of_row = torch.cumsum(kept_atom.to(torch.int64), 0) - 1
    src = record_of_row[rows[kept]]
    assert got["blocks"].shape == (got["n_rec"], 2 * mb.HOP)
    assert torch.equal(got["blocks"], want["blocks"][src])
    if name == "scalar":
        for k in got["nmr"]:
            assert torch.equal(got["nmr"][k], want["nmr"][k][rows]), k
        assert torch.equal(got["nan"], want["nan"][rows])
        assert torch.equal(got["nan"].all(dim=1), ~kept)               # a dropped hop has no NMR, a kept one has
