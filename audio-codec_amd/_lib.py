"""ctypes binding of include/pacx.h.  The HIP library is the only compute path:
if libpacx.so is missing (or no GPU is visible at create time) this raises."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PACX_LIB") or os.path.join(HERE, "libpacx.so")   # PACX_LIB: kernel-variant experiments

PACX_ABI_VERSION = 7
PCM_I16, PCM_F64 = 0, 1
FLAG_LAST, FLAG_CUR, FLAG_NEXT = 1, 2, 4
ST_SHORT, ST_ZERO_SUBBLOCK, ST_ALLOC_CAP, ST_VQ_UNDEFINED, ST_GUARD, ST_MALFORMED = 1, 2, 4, 8, 16, 32
ST_REF_RAISES = 64
ST_RATE_CAP = 128
RATE_STEP = 32             # PACX_RATE_STEP: budgets of the constant-quality mode are multiples of this many bits
RATE_TARGET_GRID = 64      # PACX_RATE_TARGET_GRID: targets of pacx_rate_solve are multiples of 1 / 64 dB
BAND_CAND = 16             # PACX_BAND_CAND: mantissa sizes on a band curve, candidate i = 0 bits for i = 0, else i + 1
PROFILE_MAX = 8193         # PACX_PROFILE_MAX: grid targets of one pacx_band_profile
SEG_CF_MAX = 1 << 40       # PACX_SEG_CF_MAX: channel-frames of one segment given by value
E_ARG, E_UNSUPPORTED = -1, -2
# what the reference raises where PACX_ST_REF_RAISES is set (coder/quantize.py:74, see include/pacx.h)
REF_SCALAR_SBR_ERROR = "'numpy.int64' object does not support item assignment"
MAX_BANDS = 32
SUB = 8

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int32_p = ctypes.POINTER(ctypes.c_int32)


class PacxSmrTables(ctypes.Structure):
    """pacx_smr_tables (include/pacx.h): device pointers to caller-evaluated tables of pacx_smr_generic_batch"""
    _fields_ = [
        ("hann", ctypes.c_void_p),
        ("tw_cos", ctypes.c_void_p),
        ("tw_sin", ctypes.c_void_p),
        ("fft_norm", ctypes.c_double),
        ("fft_freq_step", ctypes.c_double),
        ("bark", ctypes.c_void_p),
        ("quiet", ctypes.c_void_p),
        ("band_lower", ctypes.c_void_p),
        ("band_lines", ctypes.c_void_p),
        ("n_bands", ctypes.c_int32),
    ]


class PacxConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("sample_rate", ctypes.c_int32),
        ("n_lines_long", ctypes.c_int32),
        ("n_lines_short", ctypes.c_int32),
        ("n_scale_bits", ctypes.c_int32),
        ("n_mant_size_bits", ctypes.c_int32),
        ("n_bands_long", ctypes.c_int32),
        ("n_bands_short", ctypes.c_int32),
        ("target_bits_per_sample", ctypes.c_double),
        ("band_lines_long", c_int32_p),
        ("band_lines_short", c_int32_p),
        ("win_long", c_double_p),
        ("win_short", c_double_p),
        ("hann_long", c_double_p),
        ("hann_short", c_double_p),
        ("bark_long", c_double_p),
        ("thresh_long", c_double_p),
        ("bark_short", c_double_p),
        ("thresh_short", c_double_p),
        ("fft_norm_long", ctypes.c_double),
        ("fft_norm_short", ctypes.c_double),
        ("fft_freq_step_long", ctypes.c_double),
        ("fft_freq_step_short", ctypes.c_double),
        ("use_vq", ctypes.c_int32),
        ("use_sbr", ctypes.c_int32),
        ("half_log2", c_double_p),
        ("vq_log2_tan", c_double_p),
        ("log_mu1", ctypes.c_double),
        ("sbr_gauss", c_double_p),
        ("sbr_gauss_radius", ctypes.c_int32),
        ("line_freq_long", c_double_p),
        ("kbd_long", c_double_p),
        ("kbd_short", c_double_p),
        ("guard", ctypes.c_int32),
    ]


class PacxVqEntry(ctypes.Structure):
    _fields_ = [("value", ctypes.c_uint64), ("width", ctypes.c_int32), ("band", ctypes.c_int32)]


class PacxPcm(ctypes.Structure):
    _fields_ = [
        ("data", ctypes.c_void_p),
        ("dtype", ctypes.c_int32),
        ("n_channels", ctypes.c_int32),
        ("n_frames", ctypes.c_int64),
        ("frame_stride", ctypes.c_int64),
        ("channel_stride", ctypes.c_int64),
        ("sample_stride", ctypes.c_int64),
    ]


# name -> (restype, argtypes); this is the full export list of include/pacx.h
_P = ctypes.c_void_p
SIGNATURES = {
    "pacx_abi_version": (ctypes.c_int, []),
    "pacx_create": (ctypes.c_int, [ctypes.POINTER(PacxConfig), ctypes.POINTER(_P)]),
    "pacx_destroy": (None, [_P]),
    "pacx_last_error": (ctypes.c_char_p, [_P]),
    "pacx_band_stride": (ctypes.c_int, [_P]),
    "pacx_payload_stride": (ctypes.c_int, [_P]),
    "pacx_reserve": (ctypes.c_int, [_P, ctypes.c_int64]),
    "pacx_tables_exact": (ctypes.c_int, [_P]),
    "pacx_default_bands": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_int32_p, c_int32_p]),
    "pacx_mdct_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, ctypes.c_int, _P, _P, _P]),
    "pacx_smr_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, ctypes.c_int, _P, _P, _P, _P]),
    "pacx_bitalloc_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, ctypes.c_int, _P, _P, _P, _P]),
    "pacx_quantize_batch": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, _P, ctypes.c_int, _P, _P, _P]),
    "pacx_encode_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P]),
    "pacx_encode_pack_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pacx_encode_vq_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P, _P,
                                            ctypes.c_int32, _P]),
    "pacx_pack_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pacx_gather_body": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P]),
    "pacx_window_batch": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int64, _P, _P, _P]),
    "pacx_window_table_batch": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int64, _P, _P, _P]),
    "pacx_quantize_uniform": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, _P, _P]),
    "pacx_scale_factor": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, ctypes.c_int, _P, _P]),
    "pacx_mantissa": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "pacx_dequantize_uniform": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, _P, _P]),
    "pacx_dequantize": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "pacx_mantissa_fp": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "pacx_dequantize_fp": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "pacx_imdct_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, _P]),
    "pacx_mdct_direct_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P]),
    "pacx_transient_detect_f64": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P, ctypes.c_double, _P, _P]),
    "pacx_unpack_batch": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pacx_set_side_fork": (ctypes.c_int, [_P, ctypes.c_int]),
    "pacx_smr_generic_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, ctypes.POINTER(PacxSmrTables), _P, _P,
                                              _P, _P]),
    "pacx_decode_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pacx_decode_sbr_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, _P, _P, _P, ctypes.c_int, _P, _P,
                                             _P, _P, _P]),
    "pacx_decode_vq_batch": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, ctypes.c_int, _P, _P, _P, _P, _P,
                                            _P, _P, _P, _P, _P]),
    "pacx_transient_flags": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P]),
    "pacx_bitalloc_generic": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, ctypes.c_int, _P, _P, _P]),
    "pacx_index_body": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _P, _P, _P, _P]),
    "pacx_overlap_add_pcm": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, ctypes.c_int, _P, _P]),
    "pacx_nmr_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P, _P]),
    "pacx_nmr_summary": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, _P, _P, _P, _P]),
    "pacx_encode_pack_nmr_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, ctypes.c_double, ctypes.c_double,
                                                  _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pacx_encode_pack_budget_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                     _P]),
    "pacx_rate_curve_layout": (ctypes.c_int, [_P, ctypes.c_double, c_int32_p, c_int32_p]),
    "pacx_rate_curve_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, ctypes.c_double, ctypes.c_int32, _P, _P, _P,
                                             _P]),
    "pacx_band_curve_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, ctypes.c_double, _P, _P, _P, _P]),
    "pacx_profile_solve": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P, _P]),
    # limit_bytes, result, worst_above: device memory
    "pacx_profile_solve_segments": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_double, ctypes.c_double, _P, _P,
                                                   _P]),
    "pacx_profile_clamp_add": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_double, ctypes.c_double, _P, _P]),
    "pacx_encode_pack_alloc_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                    _P]),
    "pacx_vq_band_curve_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, ctypes.c_double, _P, _P, _P, _P]),
    "pacx_encode_vq_alloc_batch": (ctypes.c_int, [_P, ctypes.POINTER(PacxPcm), _P, _P, _P, _P, _P, _P, _P, _P]),
}
# The operations on a curve, pacx_<kind>_<operation>(handle, n_cf, the kind's head, the curve's three arrays, the
# operation's tail): a rate curve's row and sub_stride go by value behind n_cf, a band curve has no head.  The tails end
# with the three per-channel-frame outputs of a pick (or a profile, or the three kept arrays) and the stream.
_I64, _D = ctypes.c_int64, ctypes.c_double
CURVE_HEADS = {"rate": [ctypes.c_int32, ctypes.c_int32], "band": []}
CURVE_TAILS = {
    "solve": [_I64, _D, _D, _P, _P, _P, _P, _P],                               # limit_bytes, the range; result
    # n_seg, then seg_first and limit_bytes, int64 arrays in host memory
    "solve_segments": [_I64, _P, _P, _D, _D, _P, _P, _P, _P, _P],
    # the limits are the peaks; limit_bytes by value; floor, result [n_seg], result_stream
    "solve_peak": [_I64, _P, _P, _I64, _D, _D, _P, _P, _P, _P, _P, _P, _P],
    "profile": [_D, _D, _P, _P],
    "profile_segments": [_I64, _I64, _D, _D, _P, _P],                          # seg_cf, first_off by value
    "pick": [_D, _P, _P, _P, _P],
    "pick_segments": [_I64, _I64, _P, _P, _P, _P, _P],                         # target_t on the device
    # a curve kept as 16-bit thresholds and the picks on it: the range by value before the target(s)
    "thresholds": [_D, _D, _P, _P, _P, _P],
    "pick_thresholds": [_D, _D, _D, _P, _P, _P, _P],
    "pick_thresholds_segments": [_I64, _I64, _D, _D, _P, _P, _P, _P, _P],
}
SIGNATURES.update({f"pacx_{kind}_{op}": (ctypes.c_int, [_P, _I64, *head, _P, _P, _P, *tail])
                   for kind, head in CURVE_HEADS.items() for op, tail in CURVE_TAILS.items()})


class PacxBucket(ctypes.Structure):
    """pacx_bucket (include/pacx_bucket.h): a leaky bucket, levels in 1 / 65536 byte"""
    _fields_ = [("drain_q16", ctypes.c_int64), ("size_bytes", ctypes.c_int64), ("start_q16", ctypes.c_int64)]


BUCKET_Q = 16              # levels of a bucket are int64 in units of 2 ** -BUCKET_Q byte
BUCKET_SIZE_MAX = 1 << 40  # size_bytes of a pacx_bucket at most
BUCKET_RESULT = ("total", "peak_q16", "peak_hop", "first_over", "end_q16")     # pacx_bucket_result, int64 each
# The export list of include/pacx_bucket.h, the companion header pacx.h includes (SIGNATURES is pacx.h's own text).  The
# buffered solves: the channels of a hop behind n_cf, then a plain solve's arguments with the bucket behind the limit
# and the bucket's result behind the solve's
BUCKET_SIGNATURES = {"pacx_bucket_scan": (ctypes.c_int, [_P, _I64, ctypes.c_int32, _P, ctypes.POINTER(PacxBucket), _P, _P,
                                                         _P])}
BUCKET_SIGNATURES.update({f"pacx_{kind}_solve_bucket": (ctypes.c_int, [_P, _I64, ctypes.c_int32, *head, _P, _P, _P, _I64,
                                                                       ctypes.POINTER(PacxBucket), _D, _D, _P, _P, _P, _P,
                                                                       _P, _P])
                          for kind, head in CURVE_HEADS.items()})
# The export list of include/pacx_bucket_pin.h, the second companion header: the level through every hop (pacx_bucket_scan
# with `through` behind `level`) and the pinned solves: a buffered solve's arguments with pin_step_t and max_phases
# behind the range, target_t and phase_of behind capped and the pacx_pin_result {phases, open} behind the bucket's result
PIN_PHASES_MAX = 16
PIN_RESULT = ("phases", "open")                                                  # pacx_pin_result, int32 each
BUCKET_PIN_SIGNATURES = {"pacx_bucket_through": (ctypes.c_int, [_P, _I64, ctypes.c_int32, _P, ctypes.POINTER(PacxBucket), _P,
                                                                _P, _P, _P])}
BUCKET_PIN_SIGNATURES.update({f"pacx_{kind}_solve_bucket_pinned": (ctypes.c_int, [_P, _I64, ctypes.c_int32, *head, _P, _P, _P,
                                                                                  _I64, ctypes.POINTER(PacxBucket), _D, _D,
                                                                                  ctypes.c_int32, ctypes.c_int32, _P, _P,
                                                                                  _P, _P, _P, _P, _P, _P, _P])
                              for kind, head in CURVE_HEADS.items()})
# The export list of include/pacx_bucket_kept.h, the third companion header: the buffered solve for a stream in chunks.  The
# bytes of a pick on a kept curve at n_targets targets (a pick_thresholds call with n_targets, target_t on the device
# and n_bytes_t [n_targets][n_cf] in place of the target and the three outputs), the scans of those rows folded into
# acc, and the tree of the bisection's next decisions on the caller's state block
BUCKET_TREE_LEVELS_MAX, BUCKET_TREE_TARGETS, BUCKET_TREE_STATE_BYTES = 5, 31, 128
BUCKET_KEPT_SIGNATURES = {f"pacx_{kind}_bytes_thresholds": (ctypes.c_int, [_P, _I64, *head, _P, _P, _P, _D, _D, ctypes.c_int32,
                                                                           _P, _P, _P])
                          for kind, head in CURVE_HEADS.items()}
BUCKET_KEPT_SIGNATURES.update({
    "pacx_bucket_scan_targets": (ctypes.c_int, [_P, _I64, ctypes.c_int32, ctypes.c_int32, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "pacx_bucket_tree_begin": (ctypes.c_int, [_P, ctypes.POINTER(PacxBucket), _D, _D, ctypes.c_int32, _P, _P, _P, _P]),
    "pacx_bucket_tree_step": (ctypes.c_int, [_P, _I64, ctypes.POINTER(PacxBucket), ctypes.c_int32, _P, _P, _P, _P, _P, _P]),
})
# the summary of pacx_nmr_summary (include/pacx.h): uint64 [2][NMR_MAX_BANDS][NMR_SUMMARY_WORDS]
NMR_MAX_BANDS, NMR_COUNT, NMR_AUDIBLE, NMR_MAX, NMR_HIST, NMR_HIST_BINS = 32, 0, 1, 2, 3, 320
NMR_HIST_LO, NMR_HIST_STEP = -120.0, 0.5
NMR_SUMMARY_WORDS = NMR_HIST + NMR_HIST_BINS + 2
INDEX_SEGMENT = 8192          # PACX_IX_SEG (csrc/body_index.h): bytes mapped by one workgroup of pacx_index_body
(WIN_SINE, WIN_START, WIN_STOP, WIN_STARTSTOP, WIN_SINE_SHORT, WIN_HANN, WIN_HANN_SHORT, WIN_KBD,
 WIN_KBD_SHORT) = range(9)
MDCT_SHORT, MDCT_PREWINDOWED, MDCT_KBD = 1, 2, 4

_lib = None


class PacxError(RuntimeError):
    pass


def load():
    """Load libpacx.so and declare every prototype.  No fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # The library must belong to the sources next to it: build.py keys that on a content hash
    # (sources + headers + flags) stored beside the .so.  A stale or missing library is an ERROR here,
    # not a silent ten-compile rebuild inside whatever process happened to import the package (a
    # torchrun rank, a run under rocprofv3, a timed test).  PACX_AUTOBUILD=1 opts in to the rebuild
    # (__graft_entry__, bench.py and the test suite set it; the rebuild says so on stderr).
    from . import build as _build
    if os.environ.get("PACX_LIB"):
        # a kernel-variant or debug library (build.py --variant / --phase-debug): it carries the hash of the
        # sources it was built from as well
        if _build._read(LIB_PATH + ".hash") != _build.library_hash():
            raise PacxError(f"{LIB_PATH} (PACX_LIB) was not built from the sources in this tree: rebuild it with "
                            "`python audio-codec_amd/build.py --variant ...` / `--phase-debug`")
    elif not _build.is_current():
        if os.environ.get("PACX_AUTOBUILD") == "1":
            import sys
            print("audio_codec_amd: libpacx.so is missing or stale -- rebuilding (PACX_AUTOBUILD=1)", file=sys.stderr,
                  flush=True)
            try:
                _build.build(verbose=False)
            except Exception as e:                   # no hipcc, compile error: say so, no fallback
                raise PacxError(f"libpacx.so is missing or stale and could not be rebuilt: {e}") from e
        else:
            raise PacxError("libpacx.so is missing or does not belong to the sources in this tree (content hash "
                            "mismatch): run `python audio-codec_amd/build.py` (or set PACX_AUTOBUILD=1).  "
                            "There is no CPU implementation of this path.")
    if not os.path.exists(LIB_PATH):
        raise PacxError(
            f"{LIB_PATH} not found: build it with `python audio-codec_amd/build.py` "
            "(hipcc, gfx950).  There is no CPU implementation of this path.")
    # One HIP runtime per process: PyTorch ships its own libamdhip64 (SONAME
    # libamdhip64.so.7).  Importing torch first makes the loader resolve this
    # library's NEEDED libamdhip64.so.7 to that already-loaded copy, so torch's
    # device pointers and streams are valid here.  (A C host without torch
    # resolves it through the RUNPATH to /opt/rocm.)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **BUCKET_SIGNATURES, **BUCKET_PIN_SIGNATURES,
                              **BUCKET_KEPT_SIGNATURES}.items():
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.pacx_abi_version() != PACX_ABI_VERSION:
        raise PacxError("libpacx.so ABI version does not match the Python binding")
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    if rc != 0:
        msg = lib.pacx_last_error(handle)
        raise PacxError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
