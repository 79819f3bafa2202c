"""The two kinds of curve the rate control works on, declared once: the rate curve (Encoder.rate_curve: worst NMR and
bits at every BitAlloc budget) and the band curve (Encoder.band_curve: every band's NMR at every mantissa size).  What
differs between pacx_rate_<operation> and pacx_band_<operation> (include/pacx.h) is said here as data; Encoder's
methods, pacfile's two paths and _lib.SIGNATURES read it, and the layout of a kept curve in bytes follows from it."""
import math
from collections import namedtuple

import torch

from . import _lib

W = "width"         # in a shape: the kind's width -- a rate curve's row, the encoder's band_stride for a band curve


class Array(namedtuple("Array", "key dtype tail")):
    """one array of a curve: [n_cf, *tail]"""

    def shape(self, n_cf, width):
        return (n_cf,) + tuple(width if d is W else d for d in self.tail)

    def bytes_per_cf(self, width):
        return torch.empty((), dtype=self.dtype).element_size() * math.prod(self.shape(1, width))


class CurveKind(namedtuple("CurveKind", "prefix curve kept kept_order head per_cf")):
    """prefix   of the Encoder methods and, behind pacx_, of the C symbols
    curve       the three arrays of a curve in C argument order
    kept        the three arrays of the curve kept as 16-bit thresholds (<prefix>_thresholds) in C argument order
    kept_order  the keys of `kept` in the order the arrays lie in a chunk's kept bytes
    head        the extra keys a dict of the kind carries, C arguments behind n_cf; the first is the width, which a kind
                without them takes from the encoder
    per_cf      the per-channel-frame output of a pick or a solve, an int32 Array"""

    @property
    def as_curve(self):
        return f"a curve as {self.prefix}_curve returns it"

    @property
    def as_kept(self):
        return f"a kept curve as {self.prefix}_thresholds returns it"

    def is_kept(self, d):
        """whether a dict of the kind is a kept curve: its thresholds are the array no curve has"""
        return self.kept[0].key in d

    def kept_bytes_per_cf(self, width):
        """the bytes one kept channel-frame takes: 6 row + 32, 33 band_stride + 32"""
        return sum(a.bytes_per_cf(width) for a in self.kept)

    def kept_views(self, buf, n_cf, width, **head):
        """the arrays of n_cf kept channel-frames as views of the first n_cf * kept_bytes_per_cf bytes of buf (uint8,
        256-byte aligned), one after the other in kept_order, each contiguous; head: the dict's extra keys"""
        views, at = dict(head), 0
        for a in sorted(self.kept, key=lambda a: self.kept_order.index(a.key)):
            n = n_cf * a.bytes_per_cf(width)
            views[a.key] = buf[at:at + n].view(a.dtype).view(a.shape(n_cf, width))
            at += n
        return views

    def no_frames(self, width, device, **head):
        """the curve of no frame at all"""
        return dict({a.key: torch.zeros(a.shape(0, width), dtype=a.dtype, device=device) for a in self.curve}, **head)


SUB, CAND = _lib.SUB, _lib.BAND_CAND
RATE = CurveKind(
    "rate",
    curve=(Array("worst", torch.float64, (W,)), Array("bits", torch.int32, (W,)), Array("steps", torch.int32, (SUB,))),
    kept=(Array("e", torch.uint16, (W,)), Array("bits", torch.int32, (W,)), Array("steps", torch.int32, (SUB,))),
    kept_order=("bits", "steps", "e"),                     # the widest first: every array stays aligned
    head=("row", "sub_stride"), per_cf=Array("budget", torch.int32, (SUB,)))
BAND = CurveKind(
    "band",
    curve=(Array("nmr", torch.float64, (W, CAND)), Array("cap", torch.int32, (SUB,)), Array("cap_alloc", torch.int32, (W,))),
    kept=(Array("e", torch.uint16, (W, CAND)), Array("cap", torch.int32, (SUB,)), Array("cap_alloc", torch.uint8, (W,))),
    kept_order=("e", "cap", "cap_alloc"),
    head=(), per_cf=Array("bit_alloc", torch.int32, (W,)))
KINDS = {"budget": RATE, "band": BAND}                      # by the `allocation` keyword of the streams
