"""The transcript of the twenty Encoder methods on a rate curve or a band curve ({rate,band}_{solve, solve_segments,
solve_peak, profile, profile_segments, pick, pick_segments, thresholds, pick_thresholds, pick_thresholds_segments}):
what each hands to the C library and what it returns, and what each refuses, taken on the CPU with a library that only
records.  tests/golden/make_curve_calls.py writes it to tests/golden/curve_calls.json, tests/test_curve_calls.py
compares the methods of the tree with that file.

An argument is recorded as [ctypes type of include/pacx.h's prototype (_lib.SIGNATURES), value]; every argument has to
convert to that type as ctypes would convert it.  A pointer's value is "null", "<array>+<byte offset>" with the array
an input of the call ("curve.worst", "out", ...) or an array the method returned ("ret.budget"), or, where it is
neither, "internal" with type, shape and contents of the largest tensor alive that holds it and the offset in it.  The
two host arrays of a segmented solve are recorded by value.  A return value is recorded key by key: a tensor as
"= <input>" where it is one, else with type, shape and contents (no contents for the kept arrays a *_thresholds call
makes itself, which are uninitialised); NumPy arrays and numbers by value.
"""
import ctypes
import gc

import numpy as np
import torch

N_CF, ROW, SUB_STRIDE, BAND_STRIDE = 3, 20, 2, 8
LO, HI = -1, 1
SEG_CF, FIRST_OFF = 2, 1                                   # local segments of the three frames: {0}, {1, 2}
SEG_FIRST, SEG_LIMIT = [0, 2, 3], [100, 200]
TARGETS = [3, -4]
HANDLE = 0x5000


class RecordingLib:
    """every pacx_* attribute records (name, args) and returns `rc`"""

    def __init__(self, signatures, rc=0):
        self.signatures, self.rc, self.calls, self.named, self.values = signatures, rc, [], {}, True

    def pacx_last_error(self, h):
        return b"not on this handle"

    def pacx_destroy(self, h):
        pass

    def __getattr__(self, name):
        if not name.startswith("pacx_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(self._record(name, args))
            return self.rc
        return call

    def _record(self, name, args):
        types = self.signatures[name][1]
        assert len(args) == len(types), (name, len(args), len(types))
        live = [o for o in gc.get_objects() if type(o) is torch.Tensor and o.numel() > 0]
        rec, n_seg = [], None
        for i, (t, a) in enumerate(zip(types, args)):
            t.from_param(a)                                # TypeError where ctypes would refuse the argument
            v = a.value if isinstance(a, ctypes._SimpleCData) else a
            if t is not ctypes.c_void_p:
                rec.append([t.__name__, v])
            elif i == 0:
                rec.append(["c_void_p", "handle" if v == HANDLE else v])
            elif not v:
                rec.append(["c_void_p", "null"])
            else:
                rec.append(["c_void_p", self._pointer(v, live)])
        # seg_first [n_seg + 1] and the limits [n_seg] of a segmented solve: host memory, behind n_seg
        if name.endswith(("_solve_segments", "_solve_peak")):
            at = 3 + (2 if "_rate_" in name else 0) + 2
            n_seg = rec[at][1]
            for j, n in ((at + 1, n_seg + 1), (at + 2, n_seg)):
                raw = ctypes.string_at(args[j], 8 * n)
                rec[j] = ["c_void_p", {"host int64": np.frombuffer(raw, np.int64).tolist()}]
        return {"name": name, "args": rec}

    def _pointer(self, p, live):
        for key, t in self.named.items():
            if t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                return f"{key}+{p - t.data_ptr()}"
        inside = [t for t in live if t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size()]
        if not inside:
            return {"unknown": True}
        t = max(inside, key=lambda t: t.numel() * t.element_size())
        return {"internal": _tensor(t, self.values), "offset": p - t.data_ptr(), "raw": p}


def _tensor(t, values=True):
    d = {"dtype": str(t.dtype), "shape": list(t.shape)}
    if values:
        d["values"] = _values((t.view(torch.int16) if t.dtype == torch.uint16 else t).reshape(-1).tolist())
    return d


def _values(v):
    """a long run of one value in short"""
    return {"all": v[0], "n": len(v)} if len(v) > 8 and all(x == v[0] for x in v) else v


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return {"numpy": str(v.dtype), "shape": list(v.shape), "values": _values(v.reshape(-1).tolist())}
    if isinstance(v, (bool, np.bool_)):
        return {"bool": bool(v)}
    if isinstance(v, (int, np.integer)):
        return {"int": int(v)}
    if isinstance(v, (float, np.floating)):
        return {"float": float(v)}
    raise TypeError(type(v))


def make_encoder(A, rc=0):
    enc = A.engine.Encoder.__new__(A.engine.Encoder)
    enc.device, enc.band_stride = "cpu", BAND_STRIDE
    enc.h = ctypes.c_void_p(HANDLE)
    enc._stream = lambda: ctypes.c_void_p(0)
    enc.lib = RecordingLib(A._lib.SIGNATURES, rc)
    return enc


def curve(kind, n_cf=N_CF):
    """a curve of the kind as its *_curve method returns it, any numbers"""
    g = torch.Generator().manual_seed(5)
    if kind == "rate":
        return {"worst": torch.rand((n_cf, ROW), dtype=torch.float64, generator=g),
                "bits": torch.randint(0, 900, (n_cf, ROW), dtype=torch.int32, generator=g),
                "steps": torch.randint(-1, 9, (n_cf, 8), dtype=torch.int32, generator=g), "row": ROW,
                "sub_stride": SUB_STRIDE}
    return {"nmr": torch.rand((n_cf, BAND_STRIDE, 16), dtype=torch.float64, generator=g),
            "cap": torch.randint(-1, 900, (n_cf, 8), dtype=torch.int32, generator=g),
            "cap_alloc": torch.randint(0, 16, (n_cf, BAND_STRIDE), dtype=torch.int32, generator=g)}


def kept(kind, n_cf=N_CF, lo=LO, hi=HI):
    """a kept curve of the kind as its *_thresholds method returns it"""
    wide = (n_cf, ROW) if kind == "rate" else (n_cf, BAND_STRIDE, 16)
    k = {"e": torch.arange(int(np.prod(wide)), dtype=torch.int32).to(torch.uint16).reshape(wide)}
    if kind == "rate":
        k.update(bits=torch.ones((n_cf, ROW), dtype=torch.int32), steps=torch.ones((n_cf, 8), dtype=torch.int32),
                 row=ROW, sub_stride=SUB_STRIDE)
    else:
        k.update(cap=torch.ones((n_cf, 8), dtype=torch.int32),
                 cap_alloc=torch.ones((n_cf, BAND_STRIDE), dtype=torch.uint8))
    k.update(nmr_lo_db=lo, nmr_hi_db=hi)
    return k


def kept_out(kind, n_cf=N_CF):
    return {k: torch.zeros_like(v) for k, v in kept(kind, n_cf).items() if isinstance(v, torch.Tensor)}


def _named(prefix, v, into):
    if isinstance(v, torch.Tensor):
        into[prefix] = v
    elif isinstance(v, dict):
        for k, t in v.items():
            if isinstance(t, torch.Tensor):
                into[f"{prefix}.{k}"] = t
    elif isinstance(v, tuple):
        for i, t in enumerate(v):
            _named(f"{prefix}[{i}]", t, into)


def transcript(A, method, inputs, rc=0):
    """one call of Encoder.<method>(**inputs) -> {"calls": [...], "returns": ...} or {"raises": [type, message]}"""
    enc = make_encoder(A, rc)
    named = {}
    for k, v in inputs.items():
        _named(k, v, named)
    enc.lib.named = {k: t for k, t in named.items() if t.numel() > 0}
    enc.lib.values = made = not method.endswith("_thresholds")      # the kept arrays such a call makes are uninitialised
    try:
        ret = getattr(enc, method)(**inputs)
    except Exception as e:                                 # what the method refuses, word for word
        return {"calls": _finish(enc.lib.calls, {}), "raises": [type(e).__name__, str(e)]}
    returned, out = {}, {}
    items = ret.items() if isinstance(ret, dict) else [("", ret)]
    for k, v in items:
        if isinstance(v, torch.Tensor):
            same = [n for n, t in named.items() if t is v]
            out[k] = "= " + same[0] if same else _tensor(v, made)
            if not same and v.numel() > 0:
                returned["ret." + k if k else "ret"] = v
        else:
            out[k] = _jsonable(v)
    return {"calls": _finish(enc.lib.calls, returned), "returns": {"dict": out} if isinstance(ret, dict) else out[""]}


def _finish(calls, returned):
    """pointers into what the method returned get that array's name; the raw addresses go"""
    for c in calls:
        for a in c["args"]:
            if isinstance(a[1], dict) and "raw" in a[1]:
                p = a[1].pop("raw")
                for key, t in returned.items():
                    if t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                        a[1] = f"{key}+{p - t.data_ptr()}"
    return calls


def cases(kind):
    """(label, method without the kind's prefix, inputs) of every call and every refusal recorded for a kind"""
    first = {"rate": "worst", "band": "nmr"}[kind]
    second = {"rate": "bits", "band": "cap"}[kind]
    flags = {"flags": None} if kind == "rate" else {}
    G = 64 * (HI - LO) + 1
    n_seg = -(-(FIRST_OFF + N_CF) // SEG_CF)
    rng = {"nmr_lo_db": LO, "nmr_hi_db": HI}
    seg = {"seg_cf": SEG_CF, "first_off": FIRST_OFF}
    c = lambda: curve(kind)                                # noqa: E731
    k = lambda: kept(kind)                                 # noqa: E731
    t_dev = lambda: torch.tensor(TARGETS, dtype=torch.int32)         # noqa: E731

    def bad(d, key, how):
        d = dict(d)
        t = d[key]
        d[key] = {"dtype": lambda: t.to(torch.float32 if t.dtype.is_floating_point else torch.int64),
                  "shape": lambda: t[:, :-1], "rows": lambda: t[:-1]}[how]()
        return d

    yield "solve", "solve", dict(curve=c(), **flags, limit_bytes=1000, **rng)
    yield "solve: default range", "solve", dict(curve=c(), **flags, limit_bytes=7)
    yield "solve_segments", "solve_segments", dict(curve=c(), seg_first=SEG_FIRST, limit_bytes=SEG_LIMIT, **rng)
    yield "solve_segments: arrays, default range", "solve_segments", \
        dict(curve=c(), seg_first=np.array(SEG_FIRST, np.int32), limit_bytes=np.array(SEG_LIMIT))
    yield "solve_peak", "solve_peak", dict(curve=c(), seg_first=SEG_FIRST, peak_bytes=SEG_LIMIT, limit_bytes=1000, **rng)
    yield "solve_peak: five segments", "solve_peak", \
        dict(curve=c(), seg_first=[0, 0, 1, 2, 2, 3], peak_bytes=[1, 2, 3, 4, 5], limit_bytes=0)
    yield "profile", "profile", dict(curve=c(), **rng)
    yield "profile: default range", "profile", dict(curve=c())
    yield "profile: out", "profile", dict(curve=c(), **rng, out=torch.arange(G, dtype=torch.int64))
    yield "profile_segments", "profile_segments", dict(curve=c(), **seg, **rng)
    yield "profile_segments: default first_off and range", "profile_segments", dict(curve=c(), seg_cf=SEG_CF)
    yield "profile_segments: out of more rows", "profile_segments", \
        dict(curve=c(), **seg, **rng, out=torch.ones((n_seg + 1, G), dtype=torch.int64))
    yield "profile_segments: no frame, no segment", "profile_segments", \
        dict(curve=curve(kind, 0), seg_cf=SEG_CF, first_off=0, **rng)
    yield "profile_segments: no frame, no segment, out", "profile_segments", \
        dict(curve=curve(kind, 0), seg_cf=SEG_CF, first_off=0, **rng, out=torch.ones((1, G), dtype=torch.int64))
    yield "pick", "pick", dict(curve=c(), target_nmr_db=0.5)
    yield "pick_segments: list", "pick_segments", dict(curve=c(), **seg, target_t=TARGETS)
    yield "pick_segments: tensor", "pick_segments", dict(curve=c(), **seg, target_t=t_dev())
    yield "thresholds", "thresholds", dict(curve=c(), **rng)
    yield "thresholds: default range", "thresholds", dict(curve=c())
    yield "thresholds: out", "thresholds", dict(curve=c(), **rng, out=kept_out(kind))
    yield "pick_thresholds", "pick_thresholds", dict(kept=k(), target_nmr_db=0.5)
    yield "pick_thresholds_segments: list", "pick_thresholds_segments", dict(kept=k(), **seg, target_t=TARGETS)
    yield "pick_thresholds_segments: tensor", "pick_thresholds_segments", dict(kept=k(), **seg, target_t=t_dev())

    # ---- refusals
    on_curve = {"solve": dict(**flags, limit_bytes=1000), "solve_segments": dict(seg_first=SEG_FIRST, limit_bytes=SEG_LIMIT),
                "solve_peak": dict(seg_first=SEG_FIRST, peak_bytes=SEG_LIMIT, limit_bytes=1000), "profile": {},
                "profile_segments": dict(**seg), "pick": dict(target_nmr_db=0.5),
                "pick_segments": dict(**seg, target_t=TARGETS), "thresholds": {}}
    on_kept = {"pick_thresholds": dict(target_nmr_db=0.5), "pick_thresholds_segments": dict(**seg, target_t=TARGETS)}
    for m, more in on_curve.items():
        for key, how in ((first, "dtype"), (second, "dtype"), ("steps" if kind == "rate" else "cap_alloc", "dtype"),
                         (second, "shape"), ("steps" if kind == "rate" else "cap", "rows")):
            yield f"{m}: curve {key} wrong {how}", m, dict(curve=bad(c(), key, how), **more)
    for m, more in on_kept.items():
        for key, how in (("e", "dtype"), (second, "dtype"), ("steps" if kind == "rate" else "cap_alloc", "dtype"),
                         (second, "shape"), ("steps" if kind == "rate" else "cap", "rows")):
            yield f"{m}: kept {key} wrong {how}", m, dict(kept=bad(k(), key, how), **more)
        yield f"{m}: kept range off the grid", m, dict(kept=kept(kind, lo=-1.01), **more)
        yield f"{m}: kept range over PROFILE_MAX", m, dict(kept=kept(kind, lo=-100, hi=100), **more)
    if kind == "band":                                     # a band curve's width is the handle's, a rate curve's its own
        yield "pick: curve of another band_stride", "pick", \
            dict(curve={k_: (v[:, :-1] if k_ != "cap" else v) for k_, v in c().items()}, target_nmr_db=0.5)
    for m in ("profile", "profile_segments", "thresholds"):
        more = on_curve[m]
        yield f"{m}: range off the grid", m, dict(curve=c(), **more, nmr_lo_db=-1.01, nmr_hi_db=1)
        yield f"{m}: range upside down", m, dict(curve=c(), **more, nmr_lo_db=1, nmr_hi_db=-1)
        yield f"{m}: range not finite", m, dict(curve=c(), **more, nmr_lo_db=float("-inf"), nmr_hi_db=1)
        yield f"{m}: range over PROFILE_MAX", m, dict(curve=c(), **more, nmr_lo_db=-100, nmr_hi_db=100)
    for m in ("profile_segments", "pick_segments", "pick_thresholds_segments"):
        src = dict(kept=k()) if "thresholds" in m else dict(curve=c())
        tt = {} if m == "profile_segments" else dict(target_t=TARGETS)
        yield f"{m}: seg_cf 0", m, dict(**src, seg_cf=0, first_off=0, **tt)
        yield f"{m}: seg_cf a bool", m, dict(**src, seg_cf=True, first_off=0, **tt)
        yield f"{m}: seg_cf not whole", m, dict(**src, seg_cf=2.5, first_off=0, **tt)
        yield f"{m}: first_off = seg_cf", m, dict(**src, seg_cf=2, first_off=2, **tt)
        yield f"{m}: first_off negative", m, dict(**src, seg_cf=2, first_off=-1, **tt)
        if tt:
            yield f"{m}: target_t too long", m, dict(**src, **seg, target_t=TARGETS + [0])
            yield f"{m}: target_t not whole", m, dict(**src, **seg, target_t=[0.5, 1])
            yield f"{m}: target_t tensor too short", m, dict(**src, **seg, target_t=t_dev()[:1])
            yield f"{m}: target_t tensor int64", m, dict(**src, **seg, target_t=t_dev().to(torch.int64))
            yield f"{m}: target_t tensor not contiguous", m, \
                dict(**src, **seg, target_t=torch.zeros((2, 2), dtype=torch.int32)[:, 0])
    yield "profile: out of another length", "profile", dict(curve=c(), **rng, out=torch.zeros(G + 1, dtype=torch.int64))
    yield "profile: out not contiguous", "profile", dict(curve=c(), **rng, out=torch.zeros(2 * G, dtype=torch.int64)[::2])
    yield "profile: out int32", "profile", dict(curve=c(), **rng, out=torch.zeros(G, dtype=torch.int32))
    yield "profile_segments: out of too few rows", "profile_segments", \
        dict(curve=c(), **seg, **rng, out=torch.zeros((n_seg - 1, G), dtype=torch.int64))
    yield "profile_segments: out not contiguous", "profile_segments", \
        dict(curve=c(), **seg, **rng, out=torch.zeros((n_seg, 2 * G), dtype=torch.int64)[:, ::2])
    o = kept_out(kind)
    o["e"] = torch.zeros(tuple(o["e"].shape[:1]) + tuple(reversed(o["e"].shape[1:])),
                         dtype=torch.uint16).transpose(-1, -2) if kind == "band" else \
        torch.zeros((N_CF, 2 * ROW), dtype=torch.uint16)[:, ::2]
    yield "thresholds: out with a tensor not contiguous", "thresholds", dict(curve=c(), **rng, out=o)
    o = kept_out(kind)
    o[second] = o[second].to(torch.int16)
    yield "thresholds: out with a wrong dtype", "thresholds", dict(curve=c(), **rng, out=o)
    o = kept_out(kind)
    del o["e"]
    yield "thresholds: out without e", "thresholds", dict(curve=c(), **rng, out=o)
    for m, lim in (("solve_segments", "limit_bytes"), ("solve_peak", "peak_bytes")):
        more = dict(limit_bytes=1000) if m == "solve_peak" else {}
        yield f"{m}: negative segment limit", m, dict(curve=c(), seg_first=SEG_FIRST, **{lim: [100, -1]}, **more)
        yield f"{m}: seg_first does not end at n_cf", m, dict(curve=c(), seg_first=[0, 2, 4], **{lim: SEG_LIMIT}, **more)
        yield f"{m}: seg_first decreases", m, dict(curve=c(), seg_first=[0, 3, 2, 3], **{lim: [1, 2, 3]}, **more)
        yield f"{m}: lengths disagree", m, dict(curve=c(), seg_first=SEG_FIRST, **{lim: [100]}, **more)
        yield f"{m}: limits not integers", m, dict(curve=c(), seg_first=SEG_FIRST, **{lim: [1.5, 2.0]}, **more)
    yield "solve_peak: negative limit_bytes", "solve_peak", \
        dict(curve=c(), seg_first=SEG_FIRST, peak_bytes=SEG_LIMIT, limit_bytes=-1)
    yield "solve_peak: limit_bytes not whole", "solve_peak", \
        dict(curve=c(), seg_first=SEG_FIRST, peak_bytes=SEG_LIMIT, limit_bytes=10.5)


def everything(A):
    """{kind: {label: transcript}} of every case, and what the twenty make of PACX_E_UNSUPPORTED"""
    doc = {}
    for kind in ("rate", "band"):
        doc[kind] = {label: transcript(A, f"{kind}_{m}", inputs) for label, m, inputs in cases(kind)}
        for label, m, inputs in cases(kind):
            if ":" not in label or label.endswith(": list"):       # one plain call of each of the ten
                doc[kind]["unsupported: " + m] = transcript(A, f"{kind}_{m}", inputs, rc=A._lib.E_UNSUPPORTED)
    return doc
