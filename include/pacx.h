/*
 * pacx.h -- C ABI of the MI355X (gfx950) batched audio-frame encode path.
 *
 * Drop-in boundary for the per-frame hot loop of Abhipray/audio-codec.  The
 * reference has no FFI layer: the path sits behind plain Python calls,
 *     PACFile.Encode        coder/pacfile.py:627-643
 *     codec.Encode          coder/codec.py:225-263
 *     codec.EncodeSingleChannel  coder/codec.py:266-380
 * and the five modules those call (window.py, mdct.py, psychoac.py,
 * bitalloc.py, quantize.py).  Each entry point below names the reference
 * function(s) it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative PACX_E_* code and
 *     never throws; pacx_last_error() gives the text;
 *   - the CALLER owns every data buffer.  All `const void*` / `T*` data
 *     arguments are DEVICE pointers (hipMalloc / torch tensor .data_ptr())
 *     unless the parameter is documented as host;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*, NULL =
 *     default stream) and is asynchronous; the library keeps a grow-only
 *     device workspace per handle (pacx_reserve() sizes it up front so that
 *     no allocation happens inside a timed or graph-captured region);
 *     a call that has to grow a workspace waits for the whole device first,
 *     then frees and allocates.  No other call waits for the host, except
 *     where its own text says so (a segmented or peak solve waits for the
 *     upload of the one before it, pacx_rate_solve_segments);
 *   - all calls of one handle belong on one stream: its workspaces and its
 *     internal streams and events are shared between them, and a call is
 *     ordered against the one before it by that stream alone;
 *   - one handle per device; handles are independent (no global state).
 *
 * Units: a "channel-frame" (cf) is one EncodeSingleChannel call: 2*nMDCTLines
 * samples of one channel in, nMDCTLines MDCT lines out.  cf index =
 * frame * n_channels + channel (the order blocks appear in a .pac file).
 */
#ifndef PACX_H
#define PACX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PACX_ABI_VERSION 7

/* error codes */
#define PACX_OK            0
#define PACX_E_ARG        -1   /* bad argument                               */
#define PACX_E_UNSUPPORTED -2  /* configuration outside what the kernels do  */
#define PACX_E_HIP        -3   /* a HIP runtime call failed                  */
#define PACX_E_NOMEM      -4

/* sample formats of pacx_pcm.dtype */
#define PACX_PCM_I16 0         /* 16-bit PCM codes (coder/pcmfile.py:89-99 contract) */
#define PACX_PCM_F64 1         /* signed fractions, as codec.Encode receives them    */

/* per-frame flag bits (coder/pacfile.py:575-577 order) */
#define PACX_FLAG_LAST 1u
#define PACX_FLAG_CUR  2u
#define PACX_FLAG_NEXT 4u

/* window kinds chosen by codec.getCorrectWindow (coder/codec.py:30-44) */
#define PACX_WIN_SINE 0
#define PACX_WIN_START 1
#define PACX_WIN_STOP 2
#define PACX_WIN_STARTSTOP 3
/* further tables addressable through pacx_window_batch */
#define PACX_WIN_SINE_SHORT 4  /* SineWindow on a 256-sample short block      */
#define PACX_WIN_HANN 5        /* HanningWindow, 2048 (coder/window.py:29-41) */
#define PACX_WIN_HANN_SHORT 6  /* HanningWindow, 256                          */
#define PACX_WIN_KBD 7         /* KBDWindow(alpha = 4), 2048 (coder/window.py:45-57) */
#define PACX_WIN_KBD_SHORT 8   /* KBDWindow(alpha = 4), 256                   */

/* mode bits of pacx_mdct_batch */
#define PACX_MDCT_SHORT 1        /* 8 short sub-blocks per frame              */
#define PACX_MDCT_PREWINDOWED 2  /* input already windowed: plain mdct.MDCT   */
#define PACX_MDCT_KBD 4          /* KBDWindow instead of the sine window, long or
                                    short blocks: MDCT(KBDWindow(x), halfN, halfN), the
                                    expression at coder/bitalloc.py:161 (frame_flags
                                    must be NULL)                              */

/* per-cf status word bits written by pacx_encode_batch */
#define PACX_ST_SHORT        1u   /* coded as 8 short sub-blocks               */
#define PACX_ST_ZERO_SUBBLOCK 2u  /* a short sub-block of some channel of the
                                     hop was all zeros: the reference drops the
                                     whole hop (coder/pacfile.py:530-533); set
                                     in every channel-frame of that hop        */
#define PACX_ST_ALLOC_CAP    4u   /* BitAlloc left through its 200-pass guard
                                     (coder/bitalloc.py:116-119)               */

#define PACX_ST_VQ_UNDEFINED  8u   /* gain-shape coder reached a case where the
                                     reference itself fails (a 1-dimensional
                                     PVQ leaf never returns, an all-zero half
                                     gives NaN pulses, a gain index wider than
                                     128 bits): the band's bits are zeros     */

#define PACX_ST_GUARD        16u   /* (handles created with pacx_config.guard = 1)
                                     a rounding decision of this cf sat within a few
                                     ulps of its boundary: a mantissa / scale-factor
                                     quantiser input (2^R-1)|x|+1 next to an even
                                     integer (coder/quantize.py:73), or a BitAlloc
                                     value Ropt - level next to k + 1/2
                                     (coder/bitalloc.py:103); with use_vq also a split
                                     angle or a band's mu-law gain at a boundary of its
                                     quantiser, a pulse search whose floor(K|x|/l1) or
                                     whose last pulse hangs on the last bits of the unit
                                     vector (coder/gain_shape_quantize.py:30-54, 315-408),
                                     and a coded band with a line at rounding-noise level
                                     (np.sign(0) erases a pulse).  The codes are still the
                                     ones this arithmetic gives; a harness that needs
                                     certainty recomputes flagged frames on the CPU  */
#define PACX_ST_MALFORMED    32u   /* decode: the payload of this channel-block is
                                     truncated or carries an impossible field (the
                                     reference raises "Only read a partial block of
                                     coded PACFile data", coder/pacfile.py:203-205):
                                     its outputs are zeros                          */
#define PACX_ST_REF_RAISES   64u   /* scalar mantissas + SBR (use_sbr without use_vq), long frame:
                                      an SBR-omitted band received bits.  The reference quantises the
                                      band's one value with vMantissa(np.mean(..)) -- a NumPy scalar its
                                      vQuantizeUniform assigns into -- and raises TypeError there
                                      (coder/codec.py:541-546, coder/quantize.py:73-74; recorded in
                                      tests/golden/sbr_scalar.json), so no output is defined: the
                                      frame's n_bytes is 0, its other outputs are unspecified, and the
                                      host mirror raises the reference's error                      */

#define PACX_ST_RATE_CAP    128u   /* pacx_encode_pack_nmr_batch: a long block or a short sub-block of this cf
                                      misses the target NMR even with the cap budget and was coded with it */

#define PACX_SHORT_PER_FRAME 8    /* sub-blocks of a short frame (coder/pacfile.py:527) */

typedef struct pacx_handle pacx_handle;

/*
 * Static configuration = the CodingParams attributes the path reads
 * (coder/pacfile.py:699-707, 323-330).  Table pointers are HOST pointers,
 * copied at create time.  Tables marked "optional" may be NULL: the library
 * then uses its built-in copies (csrc/pacx_tables_gen.h: the reference's NumPy
 * expressions evaluated once and stored as bit patterns, so a C host gets the
 * same bits as the Python host) -- windows and gain-shape tables always, the
 * Bark / threshold-in-quiet tables for 44.1 and 48 kHz.  At other sample rates
 * those two are evaluated with the C math library (last-place differences from
 * NumPy's are possible); pacx_tables_exact() tells which case a handle is in.
 */
typedef struct pacx_config {
    int32_t abi_version;            /* PACX_ABI_VERSION                           */
    int32_t device;                 /* HIP device ordinal                         */
    int32_t sample_rate;            /* Hz                                         */
    int32_t n_lines_long;           /* nMDCTLines of a long block: 1024           */
    int32_t n_lines_short;          /* 128 (coder/pacfile.py:490)                 */
    int32_t n_scale_bits;           /* 4                                          */
    int32_t n_mant_size_bits;       /* 12                                         */
    int32_t n_bands_long;           /* sfBands.nBands                             */
    int32_t n_bands_short;          /* sfBandsShort.nBands                        */
    double  target_bits_per_sample; /* kb/s per channel / (sampleRate/1000)       */
    const int32_t *band_lines_long;   /* [n_bands_long]  sfBands.nLines            */
    const int32_t *band_lines_short;  /* [n_bands_short] sfBandsShort.nLines       */
    /* optional float64 tables, evaluated by the caller with NumPy so that they
       are bit-identical to the reference's: */
    const double *win_long;         /* [4][2*n_lines_long] kinds PACX_WIN_*       */
    const double *win_short;        /* [2*n_lines_short] sine                     */
    const double *hann_long;        /* [2*n_lines_long]  coder/window.py:37-39    */
    const double *hann_short;       /* [2*n_lines_short]                          */
    const double *bark_long;        /* [n_lines_long]  Bark(mdct line freq)       */
    const double *thresh_long;      /* [n_lines_long]  Thresh(mdct line freq)     */
    const double *bark_short;       /* [n_lines_short]                            */
    const double *thresh_short;     /* [n_lines_short]                            */
    double fft_norm_long;           /* 4/(N^2 mean(np.hanning(N)^2)); 0 = compute */
    double fft_norm_short;
    double fft_freq_step_long;      /* np.fft.rfftfreq step 1/(N*(1/sr)); 0 = compute */
    double fft_freq_step_short;
    /* coding variant of the file (coder/pacfile.py:703-705):
       use_vq  -- gain-shape pyramid VQ of every band instead of scale factor +
                  mantissas (coder/gain_shape_quantize.py); the handle then
                  serves pacx_encode_vq_batch instead of pacx_encode_batch;
       use_sbr -- long blocks go through EncodeSingleChannel_SBR: the bands of
                  sbr.omitted_bands (coder/sbr.py:6-9) carry one value each.
                  With use_vq this is the configuration the reference's driver
                  selects below 128 kb/s.  Without use_vq (scalar mantissas,
                  coder/codec.py:529-555) the reference is defined only while the
                  omitted bands get no bits -- pacx_encode_batch / _pack_batch then
                  follow it bit for bit (budget from the full block, max|FFT| in the
                  overall scale, BitAlloc_SBR's one-line bands) and flag the frames
                  on which it raises with PACX_ST_REF_RAISES. */
    int32_t use_vq;
    int32_t use_sbr;
    const double *half_log2;        /* optional [max band lines + 1]: 0.5*np.log2(L) */
    const double *vq_log2_tan;      /* optional [2^12 - 1]: log2(tan(theta_q) + eps) of every
                                       quantised split angle of <= 12 bits; the codes of width a
                                       start at 2^(a-1) - 1 (bit_allocation_ms, :302-309)       */
    double log_mu1;                 /* np.log(256.0) of mu_law_fn; 0 = compute       */
    /* decode side of an SBR file (coder/codec.py:147, 163-164), optional: */
    const double *sbr_gauss;        /* [2r+1] normalised weights of gaussian_filter1d(sigma=200) */
    int32_t sbr_gauss_radius;       /* r = int(4*200 + 0.5) = 800                    */
    const double *line_freq_long;   /* [n_lines_long] (k + 1/2) * sampleRate/(2*n_lines_long)   */
    /* KBDWindow(alpha = 4) tables (coder/window.py:53-57), optional: */
    const double *kbd_long;         /* [2*n_lines_long]                              */
    const double *kbd_short;        /* [2*n_lines_short]                             */
    /* 1: compute PACX_ST_GUARD (rounding decisions near their boundaries) in the whole-path
       entry points, the gain-shape one included; costs about 3 % of the encode throughput, off by default */
    int32_t guard;
} pacx_config;

/* one written field of a gain-shape coded band (see pacx_encode_vq_batch) */
typedef struct pacx_vq_entry {
    uint64_t value;                 /* low 64 bits of the index                    */
    int32_t width;                  /* bits written                                */
    int32_t band;
} pacx_vq_entry;

/*
 * Strided view of PCM input.  Sample s of frame f, channel c is element
 *     data[f*frame_stride + c*channel_stride + s*sample_stride]   (strides in elements)
 * for s in [0, 2*n_lines_long).  A stream with 50 % overlap
 * (coder/pacfile.py:460-464: frame = prior hop || new hop) has
 * frame_stride = n_lines_long * sample_stride and holds n_frames+1 hops, the
 * first being the prior block (zeros at the start of a file,
 * coder/pacfile.py:335-339).  Independent frames use frame_stride >= 2*n_lines_long.
 * Fast path: dtype I16, sample_stride 1, data 16-byte aligned, strides
 * multiples of 8.
 */
typedef struct pacx_pcm {
    const void *data;
    int32_t dtype;                  /* PACX_PCM_*                                 */
    int32_t n_channels;
    int64_t n_frames;
    int64_t frame_stride;
    int64_t channel_stride;
    int64_t sample_stride;
} pacx_pcm;

/* ---- lifetime ---------------------------------------------------------- */
int  pacx_create(const pacx_config *cfg, pacx_handle **out);
void pacx_destroy(pacx_handle *h);
/* text of the last error on this handle (h may be NULL: last create error) */
const char *pacx_last_error(const pacx_handle *h);
int  pacx_abi_version(void);
/* ints per cf in the scale_factor / bit_alloc outputs:
   max(n_bands_long, 8*n_bands_short) */
int  pacx_band_stride(const pacx_handle *h);
/* bytes per cf slot in the packed-payload output of pacx_pack_batch.  No record of the handle is longer: pacx_create
   returns PACX_E_UNSUPPORTED (pacx_last_error names the size) for band layouts and widths whose longest record --
   every band at the largest mantissa size the widths allow, a short frame counting eight sub-blocks -- would not fit,
   e.g. nMantSizeBits 16 with seven or eight short bands (sample rates of 32 kHz and below) */
int  pacx_payload_stride(const pacx_handle *h);
/* pre-size the device workspace for batches of up to n_cf channel-frames */
int  pacx_reserve(pacx_handle *h, int64_t n_cf);
/* 1 if every float64 table of the handle is bit-identical to the reference's NumPy
   evaluation (supplied by the caller or built in), 0 if some came from the C math
   library (NULL Bark / threshold tables at a sample rate without built-in copies) */
int  pacx_tables_exact(const pacx_handle *h);
/*
 * psychoac.py band layout for hosts without NumPy: AssignMDCTLinesFromFreqLimits
 * (coder/psychoac.py:106-124) followed by the merge rule of ScaleFactorBands
 * (:143-149: a band of <= 12 lines joins its right neighbour).  Plain IEEE double
 * arithmetic, bit-for-bit the reference's.  band_lines (HOST, room for 25 ints)
 * receives sfBands.nLines, *n_bands their number.  No handle needed.
 */
int  pacx_default_bands(int sample_rate, int n_mdct_lines, int32_t *band_lines, int32_t *n_bands);

/* ---- stage entry points (one per replaced reference module) ------------ */

/*
 * window.py + mdct.py: MDCT(window(data), halfN, halfN)[:halfN]
 * (coder/codec.py:303-305; window choice coder/codec.py:30-44; int16 input is
 * first mapped as coder/pcmfile.py:89-99 does).
 *   mode 0: every frame is one long block; the window kind comes
 *       from frame_flags (NULL = all sine).  lines: [n_cf][n_lines_long].
 *   mode & PACX_MDCT_PREWINDOWED: no window is applied (mdct.MDCT alone,
 *       coder/mdct.py:43-69 with a = b = halfN).
 *   mode & PACX_MDCT_SHORT: every frame is cut into 8 short sub-blocks at
 *       n = 448 + 128 j (coder/pacfile.py:526-527), sine-windowed.
 *       lines: [n_cf][8][n_lines_short].
 *   mode & PACX_MDCT_KBD: as mode 0 / PACX_MDCT_SHORT with the KBD window
 *       (alpha = 4) in place of the sine window; frame_flags must be NULL.
 * frame_flags: device uint8 [n_frames] of PACX_FLAG_* or NULL.
 * max_scale (optional, device int32 [n_cf] or [n_cf][8]): the overall scale
 * factor ScaleFactor(max|line|, nScaleBits) (coder/codec.py:308-310).
 * The lines written are NOT multiplied by 2^scale.
 */
int pacx_mdct_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                    int mode, double *lines, int32_t *max_scale, void *stream);

/*
 * psychoac.py: CalcSMRs(data, mdctLines*2^scale, scale, sampleRate, sfBands)
 * (coder/psychoac.py:220-291, with getMaskedThreshold :163-217 and
 * estimate_peaks :308-329 inside).  `lines` are the UNSCALED MDCT lines
 * (X / 2^scale is what the reference feeds to SPL, :250-254).
 *   smr:       [n_cf][band_stride]  (short: sub-block j at [j*n_bands_short ...])
 *   threshold: optional [n_cf][n_lines_long] masked threshold in dB SPL
 *   n_peaks:   optional int32 [n_cf] (short: [n_cf][8]) tonal maskers found
 */
int pacx_smr_batch(pacx_handle *h, const pacx_pcm *in, const double *lines,
                   int short_blocks, double *smr, double *threshold,
                   int32_t *n_peaks, void *stream);

/*
 * bitalloc.py: BitAlloc(bitBudget, maxMantBits, nBands, nLines, SMRs)
 * (coder/bitalloc.py:62-121) with the budget rule of coder/codec.py:288-299
 * evaluated from the frame flags (scalar-mantissa variant).
 *   bit_alloc: int32 [n_cf][band_stride]; status (optional) uint32 [n_cf].
 */
int pacx_bitalloc_batch(pacx_handle *h, int64_t n_cf, int n_channels,
                        const uint8_t *frame_flags, int short_blocks,
                        const double *smr, int32_t *bit_alloc, uint32_t *status,
                        void *stream);

/*
 * quantize.py: per band ScaleFactor(max|line|, nScaleBits, bitAlloc) and
 * vMantissa(lines, scale, nScaleBits, bitAlloc) (coder/codec.py:362-377) on
 * lines * 2^overall_scale.
 *   scale_factor: int32 [n_cf][band_stride]
 *   mantissa:     int32 [n_cf][n_lines_long], LINE-indexed (0 where the band
 *                 got no bits); the reference's dense layout is the
 *                 concatenation of the allocated bands.
 */
int pacx_quantize_batch(pacx_handle *h, int64_t n_cf, const double *lines,
                        const int32_t *overall_scale, const int32_t *bit_alloc,
                        int short_blocks, int32_t *scale_factor, int32_t *mantissa,
                        void *stream);

/* ---- the whole path ---------------------------------------------------- */

/*
 * codec.Encode for a batch (coder/codec.py:225-380, scalar mantissas):
 * window -> MDCT -> overall scale -> SMR -> BitAlloc -> scale factors and
 * mantissas, for every channel of every frame.  Frames whose PACX_FLAG_CUR
 * bit is set are coded as 8 short sub-blocks (coder/pacfile.py:489-547).
 *   overall_scale: int32 [n_cf][8]      (long frames use [0])
 *   scale_factor, bit_alloc: int32 [n_cf][band_stride]
 *   mantissa: int32 [n_cf][n_lines_long] line-indexed
 *   status:   uint32 [n_cf] PACX_ST_*
 */
int pacx_encode_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                      int32_t *overall_scale, int32_t *scale_factor,
                      int32_t *bit_alloc, int32_t *mantissa, uint32_t *status,
                      void *stream);

/*
 * pacx_encode_batch followed by pacx_pack_batch in one call (what a file writer
 * wants: codec.Encode + PACFile.writeEncodedBits for every block,
 * coder/pacfile.py:466-482, 552-608).  Long frames run BitAlloc, quantisation
 * and packing in one kernel.  `mantissa` may be NULL when the line-indexed
 * mantissas are not wanted; the other outputs are as in the two calls above.
 */
int pacx_encode_pack_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                           int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc,
                           int32_t *mantissa, uint32_t *status, uint8_t *payload, int32_t *n_bytes,
                           void *stream);

/*
 * The shipped configuration of the reference (coder/pacfile.py:699-707: useVQ
 * always, useSBR below 128 kb/s) for a batch, from PCM to finished payloads:
 *   codec.Encode / EncodeSingleChannel with useVQ   coder/codec.py:239-246, 292-294, 330-360
 *   codec.Encode_SBR / EncodeSingleChannel_SBR      coder/codec.py:383-531 (long blocks of an SBR file,
 *                                                   routing coder/pacfile.py:639-643)
 *   BitAlloc_SBR                                    coder/bitalloc.py:123-145
 *   quantize_gain_shape, split_band_encode, quantize_pvq, pvq_search,
 *   encode_pvq_vector, pvq_compute_k_for_R, gain_shape_alloc,
 *   bit_allocation_ms, mu_law_fn                    coder/gain_shape_quantize.py:30-124, 244-408, 476-512
 *   getNumBytesNeeded + WriiteEncodedBitsVQ         coder/pacfile.py:342-402, 552-592
 * The handle must have been created with use_vq.  Field lists are variable
 * length, so the natural output is the bit string itself:
 *   overall_scale: int32 [n_cf][8];  bit_alloc: int32 [n_cf][band_stride], the
 *   FINAL allocation (a band of zero gain drops to 0, coder/codec.py:352-353);
 *   payload: uint8 [n_cf][payload_stride], n_bytes: int32 [n_cf] as pacx_pack_batch;
 *   status: uint32 [n_cf] PACX_ST_*.
 * entries / entry_count (optional, for callers that want the reference's
 * (indices, idx_bits) lists): entries [n_cf][8][32][entries_per_band] receives
 * the fields of sub-block j, band b in writing order, entry_count [n_cf][8][32]
 * how many there were (may exceed entries_per_band: the excess is not stored).
 */
int pacx_encode_vq_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                         int32_t *overall_scale, int32_t *bit_alloc, uint8_t *payload,
                         int32_t *n_bytes, uint32_t *status, pacx_vq_entry *entries,
                         int32_t *entry_count, int32_t entries_per_band, void *stream);

/*
 * pacfile.py bit layout (coder/pacfile.py:404-447, 552-577; bitpack.py:37-102):
 * per cf the MSB-first payload  last|cur|next | overallScale(4) |
 * per band: (alloc-1 or 0)(nMantSizeBits) scaleFactor(nScaleBits) mantissas,
 * eight such bodies for a short frame.
 *   payload: uint8 [n_cf][payload_stride]; n_bytes: int32 [n_cf]
 *   (0 for a hop the reference drops).
 */
int pacx_pack_batch(pacx_handle *h, int64_t n_cf, int n_channels,
                    const uint8_t *frame_flags, const int32_t *overall_scale,
                    const int32_t *scale_factor, const int32_t *bit_alloc,
                    const int32_t *mantissa, const uint32_t *status,
                    uint8_t *payload, int32_t *n_bytes, void *stream);

/*
 * Concatenate "<L nBytes" + payload of every cf in order (the body of a .pac
 * file after its header, coder/pacfile.py:566-568,608).
 *   body: uint8 [>= sum(4 + n_bytes)]; total_bytes: device int64 [1].
 */
int pacx_gather_body(pacx_handle *h, int64_t n_cf, const uint8_t *payload,
                     const int32_t *n_bytes, uint8_t *body, int64_t body_capacity,
                     int64_t *total_bytes, void *stream);

/* ---- function-level entry points --------------------------------------
 * One per remaining public function of the replaced modules, so that each has
 * a GPU implementation behind the reference's signature.  The batched path
 * above does not call these. */

/* window.py: y = window * x for n_rows rows (SineWindow / StartWindow /
 * StopWindow / StartStopWindow / HanningWindow / KBDWindow; coder/window.py:14-92).
 * `window` is a PACX_WIN_* id; rows are 2048 (256 for *_SHORT) float64. */
int pacx_window_batch(pacx_handle *h, int window, int64_t n_rows, const double *x, double *y,
                      void *stream);
/* the same with a caller-supplied DEVICE table of `len` float64 (any block length,
 * e.g. KBDWindow with another alpha or N): y[r][i] = table[i] * x[r][i] */
int pacx_window_table_batch(pacx_handle *h, const double *table, int len, int64_t n_rows,
                            const double *x, double *y, void *stream);
/* quantize.py: vQuantizeUniform(x, n_bits) (coder/quantize.py:61-78) */
int pacx_quantize_uniform(pacx_handle *h, int64_t n, const double *x, int n_bits, int64_t *codes,
                          void *stream);
/* quantize.py: ScaleFactor(x[i], n_scale_bits, n_mant_bits) (coder/quantize.py:99-125) */
int pacx_scale_factor(pacx_handle *h, int64_t n, const double *x, int n_scale_bits, int n_mant_bits,
                      int64_t *scale, void *stream);
/* quantize.py: vMantissa(x, scale, n_scale_bits, n_mant_bits) (coder/quantize.py:229-250) */
int pacx_mantissa(pacx_handle *h, int64_t n, const double *x, int scale, int n_scale_bits,
                  int n_mant_bits, int64_t *mantissa, void *stream);
/* quantize.py, decode side: vDequantizeUniform(codes, n_bits) (coder/quantize.py:82-95; the scalar
 * DequantizeUniform, :40-57, gives the same values) -- float64 signed fractions; n_bits <= 53 */
int pacx_dequantize_uniform(pacx_handle *h, int64_t n, const int64_t *codes, int n_bits, double *x,
                            void *stream);
/* quantize.py: vDequantize(scale, mantissa, n_scale_bits, n_mant_bits) (coder/quantize.py:254-274; the
 * scalar Dequantize, :200-225, likewise) */
int pacx_dequantize(pacx_handle *h, int64_t n, const int64_t *mantissa, int scale, int n_scale_bits,
                    int n_mant_bits, double *x, void *stream);
/* quantize.py: MantissaFP / DequantizeFP (coder/quantize.py:130-175), the floating-point pair of the module
 * (not used by the codec; for a complete module swap and the module's self-test, :283-319) */
int pacx_mantissa_fp(pacx_handle *h, int64_t n, const double *x, int scale, int n_scale_bits,
                     int n_mant_bits, int64_t *mantissa, void *stream);
int pacx_dequantize_fp(pacx_handle *h, int64_t n, const int64_t *mantissa, int scale, int n_scale_bits,
                       int n_mant_bits, double *x, void *stream);
/* mdct.py: IMDCT(lines, a, a) (coder/mdct.py:56-62, 73-77) for the codec's block sizes, on the FFT kernels
 * of the decode path.  mode 0: rows of n_lines_long lines -> rows of 2*n_lines_long samples; PACX_MDCT_SHORT:
 * rows of 8 x n_lines_short lines -> the eight 256-sample outputs overlap-added at 448 + 128 s inside a
 * 2048-sample row (a lone sub-block 0 comes out at samples 448..703).  No window, no overall scale. */
int pacx_imdct_batch(pacx_handle *h, int64_t n_rows, int mode, const double *lines, double *blocks,
                     void *stream);
/* mdct.py for ANY split a + b (coder/mdct.py:14-77: MDCTslow / MDCT / IMDCT at the sizes the FFT kernels do
 * not cover -- the reference's own self-test uses a = b = 4 and 6): the defining cosine sums with an exact
 * integer phase reduction, O(N^2) per row.  forward: x [n_rows][a+b] -> y [n_rows][(a+b)/2]; inverse: the
 * other way round (the reference's scaling: 2/N on the forward transform, 2 on the inverse). */
int pacx_mdct_direct_batch(pacx_handle *h, int64_t n_rows, int a, int b, int inverse, const double *x,
                           double *y, void *stream);
/* bitalloc.py: BitAlloc(budget[i], max_mant_bits, n_bands, band_lines, smr[i])
 * for n independent problems (coder/bitalloc.py:62-121); all pointers device. */
int pacx_bitalloc_generic(pacx_handle *h, int64_t n, int n_bands, const int32_t *band_lines,
                          const double *budget, int max_mant_bits, const double *smr,
                          int32_t *bit_alloc, void *stream);

/* detect_transients.py + the flag shifting of the driver loop
 * (coder/detect_transients.py:5-23, coder/pacfile.py:717-741): `hops` views the
 * stream hop by hop (frame_stride = one hop, n_frames = number of hops read from
 * the file); transient[h] = parTransientDetect(hop h || zeros).  If frame_flags
 * is not NULL it receives n_frames + 2 PACX_FLAG_* bytes: one per block the
 * driver writes (every hop, the last hop a second time, the Close block). */
int pacx_transient_flags(pacx_handle *h, const pacx_pcm *hops, uint8_t *transient,
                         uint8_t *frame_flags, void *stream);

/* detect_transients.parTransientDetect(block, thresh, axis=1) (coder/detect_transients.py:5-23) for any
 * float64 blocks [n_blocks][n_channels][n_samples] (device): result[i] = 2 where the mean is exactly zero (the
 * reference returns the int 0 there), else 1 / 0 = any(peak / avg > thresh).  The mean is taken in NumPy's
 * pairwise order.  The encode path itself uses pacx_transient_flags on the int16 hops. */
int pacx_transient_detect_f64(pacx_handle *h, int64_t n_blocks, int n_channels, int n_samples,
                              const double *blocks, double thresh, uint8_t *result, void *stream);

/*
 * All-long scalar batches run on the caller's stream alone (the default), or with the side chain (FFT, peaks: it
 * only reads the PCM) forked to a second stream of the handle beside the transform.  The fork pays where the
 * runtime puts both streams on one hardware queue -- a process that keeps several steps in flight on several
 * handles (engine.EncoderPool switches it on) -- and costs where it does not: a fork and a join across hardware
 * queues take longer than the transform they hide (one handle, one step in flight: 39.1 against 42.6 M cf/s).
 * No effect where transform and side chain are one kernel: batches of 16-byte-aligned unit-stride int16 PCM without
 * per-frame flags on a handle without SBR (the default; PACX_FUSE_FRONT=0 in the environment brings the two kernels back).
 */
int pacx_set_side_fork(pacx_handle *h, int enable);

/*
 * psychoac.CalcSMRs / getMaskedThreshold (coder/psychoac.py:163-291) for block lengths other than the two the
 * handle's tuned kernels are built for (2 * n_lines_long and 2 * n_lines_short samples: 2048 and 256, the
 * reference driver's, coder/pacfile.py:699,490) -- nMDCTLines = 512, for instance.  A function-level path: one
 * workgroup per block, the spectrum by a direct DFT, then the tuned kernels' arithmetic.  All tables are the
 * CALLER's, evaluated the way the reference evaluates them (the Python mirror does it with NumPy), on the device:
 */
typedef struct pacx_smr_tables {
    const double *hann;             /* [n_samples] 0.5 (1 - cos(2 pi (n + 1/2) / N)), window.HanningWindow      */
    const double *tw_cos, *tw_sin;  /* [n_samples] cos / sin (2 pi m / N)                                       */
    double fft_norm;                /* 4 / (N^2 mean(np.hanning(N)^2)), coder/psychoac.py:172-173                */
    double fft_freq_step;           /* rfftfreq(N, 1 / sampleRate)[1]                                            */
    const double *bark, *quiet;     /* [n_samples / 2] Bark value and threshold in quiet of the MDCT lines       */
    const int32_t *band_lower;      /* [n_bands] first line of a band                                            */
    const int32_t *band_lines;      /* [n_bands] its line count (> 0)                                            */
    int32_t n_bands;                /* 1 .. 32                                                                   */
} pacx_smr_tables;
/*
 *   data:   float64 [n_blocks][n_samples], the time block CalcSMRs gets (unwindowed);
 *   lines:  float64 [n_blocks][n_samples / 2], MDCTdata / 2^MDCTscale;
 *   smr:    float64 [n_blocks][n_bands]; threshold (optional): [n_blocks][n_samples / 2] dB SPL;
 *   n_peaks (optional): int32 [n_blocks].
 */
int pacx_smr_generic_batch(pacx_handle *h, int64_t n_blocks, int n_samples, const double *data,
                           const double *lines, const pacx_smr_tables *t, double *smr, double *threshold,
                           int32_t *n_peaks, void *stream);

/* ---- decode side (scalar-mantissa streams) ---------- */

/*
 * Inverse of pacx_pack_batch: parse the payload of every channel-block
 * (coder/pacfile.py:185-213, 264-266).  Payload i starts at
 * payload + offsets[i] (offsets != NULL, e.g. a .pac body) or at
 * payload + i*payload_stride.  Outputs use the layouts of pacx_encode_batch;
 * cf_flags: uint8 [n_cf] PACX_FLAG_* read from each payload.
 * status (optional): uint32 [n_cf], PACX_ST_MALFORMED for a channel-block whose
 * fields run past its n_bytes or carry an allocation above maxMantBits = 16 (its
 * other outputs are then zeros; nothing is read beyond n_bytes either way).
 */
int pacx_unpack_batch(pacx_handle *h, int64_t n_cf, const uint8_t *payload, int payload_stride,
                      const int64_t *offsets, const int32_t *n_bytes, uint8_t *cf_flags,
                      int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc,
                      int32_t *mantissa, uint32_t *status, void *stream);

/*
 * codec.Decode for a batch (coder/codec.py:47-92: vDequantize, / 2^overall, IMDCT,
 * window) and the overlap-and-add + 16-bit PCM mapping around it
 * (coder/pacfile.py:272-295, coder/pcmfile.py:127-134).  Blocks are in stream
 * order, n_blocks hops of n_channels channels.
 *   blocks: optional float64 [n_blocks*n_channels][2*n_lines_long], the windowed
 *           IMDCT output before overlap-and-add (what codec.Decode returns);
 *   pcm:    optional int16 [(n_blocks+1)*n_lines_long][n_channels] (interleaved):
 *           every hop plus the final half-block the reference flushes at EOF.
 */
int pacx_decode_batch(pacx_handle *h, int64_t n_blocks, int n_channels, const uint8_t *cf_flags,
                      const int32_t *overall_scale, const int32_t *scale_factor,
                      const int32_t *bit_alloc, const int32_t *mantissa, double *blocks,
                      int16_t *pcm, void *stream);

/*
 * The scalar-mantissa blocks of an SBR file (handle created with use_sbr and without use_vq).
 * pacx_decode_batch is codec.Decode for every block, whatever the handle.  This entry routes:
 *   every_long_block == 0: as PACFile.Decode does (coder/pacfile.py:645-668) -- a long block with
 *           bits in an omitted band is codec.Decode_SBR's, every other block codec.Decode's;
 *   every_long_block != 0: codec.Decode_SBR on every long block (the function itself).
 * Decode_SBR's scalar branch (coder/codec.py:95-222 with useVQ off, :117-134): one line per omitted
 * band, dequantised from the mantissa at THAT line of the line-indexed array -- pacx_unpack_batch
 * leaves a coded omitted band's single mantissa (coder/pacfile.py:203-205) on every line of the
 * band, as the reader does -- then the reconstruction of :136-198.  Optional outputs:
 *   lines:  float64 [n_cf][n_lines_long], the dequantised lines after the reconstruction and
 *           BEFORE the division by 2^overallScale (short frames: 8 x n_lines_short);
 *   status: uint32 [n_cf], PACX_ST_VQ_UNDEFINED where Decode_SBR raises IndexError (the cut lies
 *           in the lower half of the spectrum: band tables of rates above 48 kHz); that block
 *           decodes from its lines as they stood before the reconstruction.
 * No encoder of the reference writes a scalar block with a coded omitted band (it raises there:
 * PACX_ST_REF_RAISES); its reader and decoder take one, so this one does.  On a handle without
 * use_sbr this is pacx_decode_batch with the lines as an extra output.
 */
int pacx_decode_sbr_batch(pacx_handle *h, int64_t n_blocks, int n_channels, const uint8_t *cf_flags,
                          const int32_t *overall_scale, const int32_t *scale_factor,
                          const int32_t *bit_alloc, const int32_t *mantissa, int every_long_block,
                          double *lines, double *blocks, int16_t *pcm, uint32_t *status, void *stream);

/*
 * Decode of gain-shape coded channel-blocks (handle created with use_vq), from
 * payload to PCM:
 *   PACFile.ReadDataBlock / getDecodedBlock   coder/pacfile.py:177-298 (useVQ branch)
 *   PACFile.Decode routing                    coder/pacfile.py:645-668
 *   codec.Decode with useVQ                   coder/codec.py:47-92
 *   codec.Decode_SBR                          coder/codec.py:95-222 (incl. the SciPy
 *                                             gaussian_filter1d / interp1d calls)
 *   dequantize_gain_shape, split_band_decode, dequantize_pvq,
 *   decode_pvq_vector, inv_mu_law_fn          coder/gain_shape_quantize.py:127-176, 259-272,
 *                                             298-299, 411-473, 515-541
 * Payload addressing as pacx_unpack_batch.  Outputs: cf_flags uint8 [n_cf],
 * overall_scale int32 [n_cf][8], bit_alloc int32 [n_cf][band_stride], status
 * uint32 [n_cf]; optional lines float64 [n_cf][n_lines_long] (the MDCT lines
 * after SBR reconstruction, BEFORE the division by 2^overallScale), blocks and
 * pcm as pacx_decode_batch.
 */
int pacx_decode_vq_batch(pacx_handle *h, int64_t n_blocks, int n_channels, const uint8_t *payload,
                         int payload_stride, const int64_t *offsets, const int32_t *n_bytes,
                         uint8_t *cf_flags, int32_t *overall_scale, int32_t *bit_alloc, double *lines,
                         double *blocks, int16_t *pcm, uint32_t *status, void *stream);

/* ---- decoding a stream in chunks ------------------------------------------ */

/*
 * The record index of a .pac body, built on the device: where the payloads start and how long they
 * are, in the form pacx_unpack_batch / pacx_decode_vq_batch take (offsets relative to `body`).
 * body (device, n_body bytes) starts at a length prefix ('<L nBytes').  A record is valid when
 * 1 <= nBytes <= pacx_payload_stride(h) and it ends at or before n_body.  Outputs (device):
 *   offsets int64 [max_records], n_bytes int32 [max_records]: the records on the chain from byte 0,
 *           in order;
 *   result  int64 [3]: [0] records returned, always a multiple of n_channels; [1] bytes consumed
 *           (the position of the first prefix not returned); [2] the position of the prefix at
 *           which the chain broke, or -1.
 * The chain stops without error at max_records and, when final == 0, at a record (or a prefix)
 * that runs past n_body: the piece a caller carries into its next chunk.  With final != 0 such a
 * tail is an error, as is a length outside 1..pacx_payload_stride(h) anywhere ON THE CHAIN (lengths
 * that appear inside payload bytes mean nothing).  On an error the records before it are still
 * returned.  Nothing at or past body + n_body is read.  Segments of 8192 bytes are mapped in
 * parallel and stitched (csrc/body_index.h); the tables live in the handle (about 1.1 bytes per
 * body byte, grow-only), so calls on one handle must not overlap each other.
 */
int pacx_index_body(pacx_handle *h, const uint8_t *body, int64_t n_body, int n_channels, int final,
                    int64_t max_records, int64_t *offsets, int32_t *n_bytes, int64_t *result,
                    void *stream);

/*
 * Overlap-and-add + 16-bit PCM mapping of one batch of a longer stream (the last stage of
 * pacx_decode_batch with the half-block across the batch boundary in the caller's hands).
 *   blocks: float64 [n_blocks*n_channels][2*n_lines_long], the `blocks` output of the decoders;
 *   tail:   float64 [n_channels][n_lines_long], in and out: the second half of the block before this
 *           batch (zeros at the start of a stream); on return the second half of the last block
 *           (unchanged when n_blocks == 0);
 *   pcm:    int16 [(n_blocks + (flush != 0)) * n_lines_long][n_channels]: hop 0 = tail + first half
 *           of block 0, hop h = second half of block h-1 + first half of block h, and with flush
 *           the half-block the reference writes at EOF (coder/pacfile.py:272-295) as one more hop.
 * A zeroed tail with flush = 1 gives pacx_decode_batch's pcm bit for bit.  No state is kept in the
 * handle.
 */
int pacx_overlap_add_pcm(pacx_handle *h, int64_t n_blocks, int n_channels, const double *blocks,
                         double *tail, int flush, int16_t *pcm, void *stream);

/* ---- quality of an encode: noise-to-mask ratios ---------------------------- */

/*
 * Per-band noise-to-mask ratio of coded blocks against the masked threshold the encoder's own
 * psychoacoustic model gives for the original (no function of the reference: it judges an encode by
 * plotting spectrograms, test_sbr.py / test_blockswitch.py).  In the reference's conventions, for one
 * block (1024 lines and the long band table, or a 128-line sub-block and the short table):
 *   X[k]   MDCT lines of the original with the window the frame flags select, not multiplied by
 *          2^overallScale (pacx_mdct_batch's lines);
 *   Xh[k]  the lines the decoder hands to the IMDCT: dec_lines[k] / 2^overall_scale;
 *   T[k]   getMaskedThreshold of the original block in dB SPL (coder/psychoac.py:163-217,
 *          pacx_smr_batch's threshold);
 *   n[k] = 4 (X[k] - Xh[k])^2   the MDCT intensity normalisation of coder/psychoac.py:250-253;
 *   m[k] = 10^((T[k] - 96) / 10)   Intensity(), coder/psychoac.py:28-32;
 *   per band b: N_b = mean(n), M_b = mean(m) over the band's lines and
 *   NMR_b = 10 log10((N_b + eps) / M_b), eps = 2^-52 as in the reference's SPL() -- a noiseless band
 *   gets a finite value; SPL()'s clamps and its "exact zero -> 1e-8" rule are left out.
 * NMR_b > 0 dB: the coding noise of the band is predicted to be audible.  Lines beyond the last band
 * (sample rates above 48 kHz) are ignored.
 *   in, frame_flags: the original PCM and the flags the blocks were coded with (PACX_FLAG_CUR: eight
 *          short sub-blocks); NULL flags = all long sine blocks;
 *   dec_lines:     float64 [n_cf][n_lines_long], the `lines` output of pacx_decode_sbr_batch /
 *                  pacx_decode_vq_batch (BEFORE the division by 2^overallScale; short: 8 x n_lines_short);
 *   overall_scale: int32 [n_cf][8] as the decoders and encoders write it (long frames use [0]);
 *   status (optional): uint32 [n_cf]; a cf with PACX_ST_ZERO_SUBBLOCK, PACX_ST_MALFORMED,
 *                  PACX_ST_VQ_UNDEFINED or PACX_ST_REF_RAISES has no defined payload: its outputs are NaN;
 *   noise, mask, nmr_db: float64 [n_cf][band_stride]: N_b, M_b and NMR_b (short: sub-block j at
 *                  [j*n_bands_short ...], the layout of pacx_smr_batch); unused slots hold NaN.
 * Runs MDCT -> side chain -> masked threshold -> k_nmr on `stream`.  The threshold lives in the handle's
 * workspace (8 KB per cf, grow-only, allocated by the first call; from then on pacx_reserve sizes it too).
 */
int pacx_nmr_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, const double *dec_lines,
                   const int32_t *overall_scale, const uint32_t *status, double *noise, double *mask,
                   double *nmr_db, void *stream);

/* the summary of pacx_nmr_summary: uint64 [2][PACX_NMR_MAX_BANDS][PACX_NMR_SUMMARY_WORDS], [0] long blocks,
 * [1] short sub-blocks, per band index.  Words: */
#define PACX_NMR_MAX_BANDS 32
#define PACX_NMR_COUNT 0          /* values (NaN slots are not counted)                          */
#define PACX_NMR_AUDIBLE 1        /* values above 0 dB                                           */
#define PACX_NMR_MAX 2            /* the maximum as a key: the bits b of the double, ~b if its sign
                                     bit is set, else b | 2^63 (unsigned order = numeric order); 0: none */
#define PACX_NMR_HIST 3           /* [0] v < PACX_NMR_HIST_LO, [1 + i] bin i = floor((v - LO) / STEP),
                                     [1 + PACX_NMR_HIST_BINS] v >= LO + BINS * STEP                */
#define PACX_NMR_HIST_BINS 320
#define PACX_NMR_HIST_LO (-120.0) /* dB */
#define PACX_NMR_HIST_STEP 0.5    /* dB */
#define PACX_NMR_SUMMARY_WORDS (PACX_NMR_HIST + PACX_NMR_HIST_BINS + 2)

/*
 * Adds the nmr_db values of a batch ([n_cf][band_stride], as pacx_nmr_batch writes them) to `summary`
 * (device; the caller zeroes it before the first batch of a stream, so chunks accumulate).  Integer
 * atomics and a maximum only: the result does not depend on the order the values arrive in.
 * Percentiles are read from the histogram on the host.
 */
int pacx_nmr_summary(pacx_handle *h, int64_t n_cf, int n_channels, const uint8_t *frame_flags,
                     const double *nmr_db, uint64_t *summary, void *stream);

/* ---- coding to a target noise-to-mask ratio -------------------------------- */

#define PACX_RATE_STEP 32         /* budgets found by the search are multiples of this many bits */

/*
 * Constant quality instead of constant rate, for the scalar coder (long and short blocks, 1024 lines): every
 * long block and every short sub-block ("unit") gets the BitAlloc budget a bisection finds for it, the smallest
 * on its path whose predicted noise stays at or below target_nmr_db of the mask in every band.  The .pac format
 * carries no rate, every record its own length and every band its own allocation, so the result is an ordinary
 * scalar .pac stream (no function of the reference: its only control is the rate of the whole file).
 *
 * The search, per unit, on the quantities of pacx_encode_pack_batch -- lines X (not multiplied by
 * 2^overallScale), the overall scale, the band SMRs, the masked threshold T[k]:
 *
 *   cap = the budget rule of coder/codec.py:288-299 (pacx_bit_budget, csrc/pacx_exact.h) with
 *         max_bits_per_sample in place of the handle's rate, same flags and short-block handling
 *   J   = max(floor(cap / PACX_RATE_STEP), 0)
 *   ok(B): alloc = BitAlloc(double(B), maxMantBits, bands, SMR)           the encoder's own arithmetic
 *          per band the scale factor and the mantissas exactly as the encoder makes them, then vDequantize
 *          Xh = dequantised / 2^overallScale (0 in a band without bits)
 *          NMR_b as pacx_nmr_batch defines it (n = 4 (X - Xh)^2, m = 10^((T - 96) / 10), band means, eps = 2^-52)
 *          return max_b NMR_b <= target_nmr_db
 *   if not ok(32 J):  budget = 32 J, status |= PACX_ST_RATE_CAP
 *   else: lo = -1, hi = J; while hi - lo > 1: mid = (lo + hi) / 2; if ok(32 mid) hi = mid else lo = mid
 *         budget = 32 hi
 *
 * ok() is not strictly monotone in B (BitAlloc's rounding ladder and its 200-pass guard), so the result is the
 * bisection's, not a global minimum: ok holds at the budget returned and failed at the last budget tried below
 * it.  Every loop has a constant bound: at most 1 + ceil(log2(J + 1)) evaluations with J <= 512
 * (max_bits_per_sample <= 16, the widest mantissa), each with BitAlloc's own 200-pass guard.  A short-coded hop
 * the reference drops (PACX_ST_ZERO_SUBBLOCK) stays dropped; its budgets are 0.
 *
 *   target_nmr_db:       finite; 0 = noise at the mask, negative = below it
 *   max_bits_per_sample: cap rate, kb/s per channel / (sampleRate / 1000); 0 < . <= 16
 *   budget (out):        int32 [n_cf][8], long frames use [0] (the rest is 0)
 *   mantissa:            optional; the other outputs as pacx_encode_pack_batch, bit_alloc being the allocation
 *                        of the budget found
 * Runs MDCT -> side chain -> masked threshold (kept in the handle's workspace as pacx_nmr_batch keeps it) ->
 * k_rate_search -> scale factors + mantissas -> pack on `stream`.  PACX_E_UNSUPPORTED on a handle created with
 * use_vq or use_sbr; PACX_E_ARG for a null output, a non-finite target, a cap rate outside (0, 16].
 */
int pacx_encode_pack_nmr_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, double target_nmr_db,
                               double max_bits_per_sample, int32_t *overall_scale, int32_t *scale_factor,
                               int32_t *bit_alloc, int32_t *mantissa, uint32_t *status, uint8_t *payload,
                               int32_t *n_bytes, int32_t *budget, void *stream);

/*
 * The same path without the search: BitAlloc of every unit with the caller's budget (int32 [n_cf][8] in bits,
 * any value; long frames use [0]), then scale factors, mantissas and payloads -- the second pass of a two-pass
 * rate control.  With the budgets pacx_encode_pack_nmr_batch returned it writes that call's payloads again.
 */
int pacx_encode_pack_budget_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                  const int32_t *budget, int32_t *overall_scale, int32_t *scale_factor,
                                  int32_t *bit_alloc, int32_t *mantissa, uint32_t *status, uint8_t *payload,
                                  int32_t *n_bytes, void *stream);

/* ---- coding to an average bit rate: one target NMR per stream ---------------- */

#define PACX_RATE_TARGET_GRID 64  /* targets of pacx_rate_solve are multiples of 1 / 64 dB */

/*
 * "The best constant quality that fits N bytes", in two steps that share nothing but arrays: the rate-distortion
 * curve of every unit (pacx_rate_curve_batch, one analysis of the PCM), then one cheap solve per size wanted
 * (pacx_rate_solve).  The budgets it returns go to pacx_encode_pack_budget_batch, whose n_bytes equal the ones
 * predicted here.  Scalar coder, 1024 lines, as pacx_encode_pack_nmr_batch.
 *
 * The curve.  Units, cap, J and the evaluation are those of pacx_encode_pack_nmr_batch (one device function serves
 * both, so the same unit, budget and target give the same decision bit for bit).  For j = 0 ... J:
 *
 *   worst[j] = max_b NMR_b of the unit coded with BitAlloc budget 32 j        what ok(32 j) compares with the target
 *   bits[j]  = nScaleBits + sum_b (nMantSizeBits + nScaleBits + alloc_b * lines_b)      what the packer writes for it
 *
 * One row of `row` entries per channel-frame: a long frame uses [0 ... J], a short-coded frame keeps sub-block sb
 * at [sb * sub_stride ... sb * sub_stride + J]; entries beyond are not written.  steps int32 [n_cf][8] holds J of
 * every unit and -1 where there is none: slots 1-7 of a long frame, every slot of a hop the reference drops
 * (PACX_ST_ZERO_SUBBLOCK).  pacx_rate_curve_layout (host only) gives row and sub_stride = J_short_max + 1 for a
 * handle and a cap rate, the maximum over the flag combinations (the budget rule depends on them).
 *
 *   max_bits_per_sample: as pacx_encode_pack_nmr_batch, 0 < . <= 16
 *   row:                 at least pacx_rate_curve_layout's
 *   worst (out):         float64 [n_cf][row];  bits (out): int32 [n_cf][row];  steps (out): int32 [n_cf][8]
 * Runs MDCT -> side chain -> masked threshold -> k_rate_curve on `stream`; the lines, thresholds, overall scales
 * and status words stay in the handle's workspace.  PACX_E_UNSUPPORTED on a handle created with use_vq or use_sbr;
 * PACX_E_ARG for a null output, a cap rate outside (0, 16], a row that is too small.
 */
int pacx_rate_curve_layout(const pacx_handle *h, double max_bits_per_sample, int32_t *row, int32_t *sub_stride);
int pacx_rate_curve_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, double max_bits_per_sample,
                          int32_t row, double *worst, int32_t *bits, int32_t *steps, void *stream);

typedef struct pacx_rate_result {
    int32_t t;                    /* the target found, in 1 / PACX_RATE_TARGET_GRID dB */
    int32_t met;                  /* 1: total <= limit_bytes; 0: not even at nmr_hi_db (t is then its grid value) */
    int64_t total;                /* body bytes at t, the 4-byte length prefixes included */
} pacx_rate_result;

/*
 * The solve.  The target lives on a grid, T = t / 64 dB, t an integer in [t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db]:
 *
 *   pick(unit, T): the bisection of pacx_encode_pack_nmr_batch with ok(32 j) := worst[j] <= T
 *                  -> j*; not (worst[J] <= T): j* = J and the channel-frame is marked capped
 *   bytes(cf, T) = 0 for a dropped hop, else ((sum over its units of bits[j*]) + 4 + 7) >> 3
 *   total(T)     = sum over cf with bytes > 0 of (bytes + 4)                  the .pac body, length prefixes included
 *   if total(t_hi) > limit_bytes:  met = 0, t = t_hi
 *   else: lo = t_lo - 1, hi = t_hi; while hi - lo > 1: mid = floor((lo + hi) / 2);
 *                                                      if total(mid) <= limit_bytes: hi = mid else lo = mid
 *         t = hi, met = 1
 *
 * worst[j] is not monotone in j (see the search above) and total need not be monotone in t, so the result is this
 * bisection's, not a global optimum: total(t) <= limit_bytes holds at the t returned and failed at the last t
 * tried below it.  On the device this is pacx_rate_solve_segments' solve with the whole batch as its one segment
 * (there is one implementation; see below): a pick kernel (one channel-frame per thread, at most 8 x 11 look-ups, a
 * workgroup reduction, one 64-bit integer atomicAdd per workgroup) and a step kernel, enqueued as
 * 2 + ceil(log2(t_hi - t_lo + 2)) pairs whatever the data; pairs after the answer is known do nothing, and the
 * host waits for none: the limit travels as a kernel argument, nothing is copied from the host.  Integer sums: the
 * result does not depend on the order of execution.  The solve's few words of state live in the handle: solves of
 * one handle belong on one stream, as all its calls do.
 *
 *   worst, bits, steps, row, sub_stride: a curve as pacx_rate_curve_batch writes it (row >= 7 sub_stride + 1); a
 *                  J that would leave its row is cut to the row
 *   limit_bytes:   >= 0, for the body (the file's header is not counted)
 *   nmr_lo_db <= nmr_hi_db: finite, multiples of 1 / 64 dB, at most 2^20 dB in magnitude
 *   budget (out):  int32 [n_cf][8], the layout pacx_encode_pack_budget_batch takes (0 where there is no unit)
 *   n_bytes (out): int32 [n_cf], bytes(cf, T) at the t returned
 *   capped (out):  uint8 [n_cf]
 *   result (out):  device memory
 * PACX_E_UNSUPPORTED on a handle created with use_vq or use_sbr; PACX_E_ARG for a null pointer, a bad row, bounds
 * that are not finite, inverted or off the grid, a negative limit.
 */
int pacx_rate_solve(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                    const int32_t *bits, const int32_t *steps, int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db,
                    int32_t *budget, int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result, void *stream);

/* ---- bits handed to the bands one by one: the minimum for a target NMR ------- */

#define PACX_BAND_CAND 16         /* mantissa sizes on a band curve: candidate i means bits(i) = 0 for i = 0, else i + 1 */

/*
 * The search and the curve above hand the bits to the bands by the reference's BitAlloc, which works from the
 * psychoacoustic model's SMRs: the worst band dictates the budget and every other band is coded finer than the
 * target asks.  In this coder the noise of a band depends on that band's own mantissa size and on nothing else (the
 * overall scale is fixed before the allocation, the scale factor comes from the band's own maximum, mantissas and
 * dequantiser are per line), and a record carries every band's allocation (0, 2, 3, ..., maxMantBits are the
 * representable sizes).  So the smallest stream that keeps every band at or below a target is found band by band:
 * one curve of PACX_BAND_CAND values per band (pacx_band_curve_batch), a pick or a solve on it (pacx_band_pick,
 * pacx_band_solve), and a second pass that codes with the allocation found (pacx_encode_pack_alloc_batch), whose
 * n_bytes equal the ones predicted.  Scalar coder, 1024 lines, one batch, as pacx_encode_pack_nmr_batch.
 *
 * Per unit, on the quantities of pacx_encode_pack_nmr_batch -- lines X, the overall scale, the masked threshold
 * T[k], the band maxima max_b of |X 2^overall|:
 *
 *   n_cand = maxMantBits = min(2^nMantSizeBits, 16)
 *   nmr[b][i], i < n_cand: NMR_b as pacx_nmr_batch defines it when band b is coded with bits(i): the scale factor
 *          pacx_scale_factor(max_b, nScaleBits, bits), per line pacx_mantissa -> pacx_dequantize -> / 2^overall
 *          (Xh = 0 for 0 bits), n = 4 (X - Xh)^2, band means, eps = 2^-52, m = 10^((T - 96) / 10)
 *   nmr[b][i], i >= n_cand: +inf
 *   cap       = 32 J, J exactly as the search takes it (pacx_rate_steps with max_bits_per_sample, same flags and
 *               short-block handling)
 *   cap_alloc = BitAlloc(double(32 J), maxMantBits, bands, SMR), the encoder's own; the status bits it raises
 *               (PACX_ST_ALLOC_CAP, PACX_ST_GUARD) are kept per cf in the handle beside the front end's, as
 *               pacx_rate_curve_batch keeps its front end's
 *
 *   pick(unit, T): per band a_b = bits(i*), i* the smallest i, scanning in ascending order, with nmr[b][i] <= T
 *          (some bands' NMR rises somewhere along the sizes, so the scan visits them all and does not bisect);
 *          a NaN or a miss at every i gives a_b = bits(n_cand - 1) and marks the band missed.
 *          If any band missed, or sum_b a_b lines_b > cap, the unit is capped and its channel-frame marked in
 *          `capped` (what PACX_ST_RATE_CAP marks for the search).  A capped unit whose sum exceeds cap is coded with
 *          cap_alloc -- exactly as the search codes a unit it flags PACX_ST_RATE_CAP; one whose sum fits keeps its a_b.
 *   bits(unit)   = nScaleBits + sum_b (nMantSizeBits + nScaleBits + a_b lines_b)
 *   bytes(cf, T) = 0 for a dropped hop, else ((sum over its units of bits(unit)) + 4 + 7) >> 3
 *   total(T)     = sum over cf with bytes > 0 of (bytes + 4)
 *
 * Wherever no unit is capped, a_b is the minimum over all representable sizes that keeps band b at or below T.
 * There a_b and total(T) are non-increasing in T (the set of passing sizes only grows with T), so the solve below
 * returns the lowest grid target that fits, not merely the bisection's answer.  Where a unit moves from capped to
 * uncapped as T rises, total may rise.  A unit capped for size spends at most cap mantissa bits -- the bound of the
 * existing capped path; pacx_band_curve_batch checks that this keeps every record within pacx_payload_stride for
 * the cap rate given (an allocation of maxMantBits everywhere need not fit for a short-coded frame, which is why
 * the cap is not optional) and returns PACX_E_UNSUPPORTED otherwise.  A short-coded hop the reference drops
 * (PACX_ST_ZERO_SUBBLOCK) stays dropped.
 *
 *   nmr (out):       float64 [n_cf][band_stride][PACX_BAND_CAND], band slots as bit_alloc: cf band_stride + sb nb + b;
 *                    slots no band of the frame uses are not written
 *   cap (out):       int32 [n_cf][8], 32 J of every unit and -1 where there is none: slots 1-7 of a long frame, every
 *                    slot of a dropped hop -- the later steps need no flags
 *   cap_alloc (out): int32 [n_cf][band_stride], 0 where there is no band
 * Runs MDCT -> side chain -> masked threshold -> k_band_curve on `stream` (maxMantBits passes over a unit's lines
 * instead of a BitAlloc and a pass per budget).  PACX_E_UNSUPPORTED on a handle created with use_vq or use_sbr;
 * PACX_E_ARG for a null output, a cap rate outside (0, 16].
 */
int pacx_band_curve_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, double max_bits_per_sample,
                          double *nmr, int32_t *cap, int32_t *cap_alloc, void *stream);

/*
 * pick(unit, T) for every unit at T = target_nmr_db (finite), on the arrays alone: one wave per channel-frame, a
 * lane per (unit, band) pair.
 *   bit_alloc (out): int32 [n_cf][band_stride], 0 where there is no unit
 *   n_bytes (out):   int32 [n_cf], bytes(cf, T);  capped (out): uint8 [n_cf]
 */
int pacx_band_pick(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                   double target_nmr_db, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, void *stream);

/*
 * pacx_rate_solve with this pick in place of the curve look-up: the same grid (PACX_RATE_TARGET_GRID), the same
 * decision, state, fixed number of pick / step pairs without a host wait, and the same pacx_rate_result.  Argument
 * rules are pacx_rate_solve's; the outputs are those of pacx_band_pick at the t returned.
 */
int pacx_band_solve(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                    int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db, int32_t *bit_alloc, int32_t *n_bytes,
                    uint8_t *capped, pacx_rate_result *result, void *stream);

/* ---- the size at every target of the grid: a stream solved piece by piece ---- */

#define PACX_PROFILE_MAX 8193     /* grid targets of one profile: a range of 128 dB */

/*
 * pacx_band_solve needs the whole stream's curve resident: it bisects with one pick per target tried.  total(T) is a
 * sum over channel-frames of integers, so the size at EVERY target of the grid can be taken in one pass instead, piece
 * by piece in any order, and the solve read from that.  With [t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db] and
 * G = t_hi - t_lo + 1:
 *
 *   for g = 0 ... G - 1:  profile[g] += total(T_g) over the n_cf channel-frames given,  T_g = (t_lo + g) / 64
 *
 * total, bytes, pick, the miss rule and the cap rule are exactly pacx_band_pick's: a NaN entry never passes, -inf
 * passes everywhere and +inf nowhere, a dropped hop (cap all -1) adds nothing, a unit whose sum exceeds its cap takes
 * cap_alloc.  The call ADDS to what profile holds -- the caller zeroes it before the first piece -- and integer sums
 * make the result independent of how the stream is cut and of the order of execution.
 *
 * It is not G picks.  Per (unit, band) the size picked is a step function of the target with at most PACX_BAND_CAND
 * steps: nmr[b][i] <= t / 64 is 64 nmr[b][i] <= t (both scalings are exact), so size i passes from the grid index
 * e_i = ceil(64 nmr[b][i]) - t_lo on -- 0 where that is negative, never where the entry is NaN or above nmr_hi_db,
 * decided by comparisons in double before any conversion to an integer -- and the pick at g is the smallest i with
 * e_i <= g, bits(n_cand - 1) below all of them.  A workgroup puts a unit's steps as deltas into a difference array
 * over the grid in LDS, scans it, applies the cap rule to the unit's sum at every g and keeps the bytes of its
 * frames per g; it adds them to profile with one 64-bit atomicAdd per entry at its end.  One launch, no host wait.
 *
 *   nmr, cap, cap_alloc: a band curve as pacx_band_curve_batch or pacx_vq_band_curve_batch writes it
 *   nmr_lo_db <= nmr_hi_db: pacx_band_solve's rules, and G <= PACX_PROFILE_MAX
 *   profile (in/out):    int64 [G] in device memory
 * n_cf = 0 is a valid call that adds nothing.  Any scalar handle with the curve's band layout serves, as for the
 * pick.  PACX_E_UNSUPPORTED on a handle created with use_vq or use_sbr; PACX_E_ARG for a null pointer, a bad count,
 * bounds that are not finite, inverted, off the grid or more than PACX_PROFILE_MAX targets apart.
 */
int pacx_band_profile(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                      double nmr_lo_db, double nmr_hi_db, int64_t *profile, void *stream);

/*
 * The decision of pacx_rate_solve (above), word for word, with total(t) := profile[t - t_lo]: met = 0 and t = t_hi
 * if profile[G - 1] > limit_bytes, else the bisection from lo = t_lo - 1, hi = t_hi; result->total = profile[t - t_lo].
 * On a profile of a whole curve the result is pacx_band_solve's on that curve.  One single-thread kernel with a trip
 * count fixed by G; nothing waits for the device.
 *   profile: int64 [G] in device memory, the range it was taken with;  limit_bytes >= 0;  result (out): device memory
 * Errors as pacx_band_profile, and PACX_E_ARG for a negative limit.
 */
int pacx_profile_solve(pacx_handle *h, const int64_t *profile, int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db,
                       pacx_rate_result *result, void *stream);

/* ---- a profile per segment: segmented and peak solves piece by piece ---- */

#define PACX_SEG_CF_MAX (1LL << 40)   /* channel-frames of one segment given by value, at most */

/*
 * A profile per segment is additive over pieces of a stream exactly as the stream's profile is, and that carries the
 * segmented solve and the two-level peak solve (below) to streams of any length.  Segments here are uniform
 * stretches of the stream given by value -- no table, no upload, nothing the host waits for:
 *
 *   seg_cf    in [1, PACX_SEG_CF_MAX]: channel-frames per segment
 *   first_off in [0, seg_cf): channel-frames of the piece's first segment that lie before the piece
 *   frame cf of the piece lies in local segment (first_off + cf) / seg_cf;  n_seg = ceil((first_off + n_cf) / seg_cf)
 *
 * pacx_band_profile_segments: for every local segment s, row s of profile += what pacx_band_profile adds for that
 * segment's frames of the piece, under every rule of pacx_band_profile (the steps decided in double before any cast,
 * NaN and the infinities, dropped hops, the cap rule, integer sums; n_cf = 0 adds nothing).  A segment cut by the
 * piece's start or end gets the rest of its row from the neighbouring piece's call.  The kernel is pacx_band_profile's
 * per frame; a workgroup walks a contiguous run of frames and adds the bytes it holds in registers to the row of the
 * segment it is in whenever that changes (one 64-bit atomicAdd per entry), so a flush happens once per workgroup and
 * segment touched, not once per frame.  One launch, no host wait.
 *   profile (in/out): int64 [n_seg][G] in device memory; rows beyond n_seg are not touched
 *
 * pacx_profile_solve_segments: result[s] = pacx_profile_solve's decision on row s against limit_bytes[s], and
 * worst_above[s] = max over g >= result[s].t - t_lo of row_s[g]: the most the segment takes at its target or any higher
 * one.  A negative limit is never met (met = 0, t = t_hi).  An all-zero row gives t = t_lo, met = 1, total = 0.  One
 * launch, a wave per row, trip counts fixed by G.
 *   n_seg >= 1;  profile: int64 [n_seg][G];  limit_bytes: int64 [n_seg] in DEVICE memory
 *   result (out): pacx_rate_result [n_seg];  worst_above (out): int64 [n_seg], may be NULL -- device memory
 *
 * pacx_profile_clamp_add: stream_profile[g] += sum over s of row_s[max(g, result[s].t - t_lo)].  With result[s].t the
 * floor u_s of pacx_band_solve_peak's stage A (the solve above against the peaks), the sum over all segments of a
 * stream is total*(t) of stage B at every t of the grid, and pacx_profile_solve on it against the stream's limit is
 * stage B's decision word for word; T_s = max(t*, u_s).  One launch.
 *   result: pacx_rate_result [n_seg] with t in [t_lo, t_hi];  stream_profile (in/out): int64 [G] -- device memory
 *
 * pacx_band_pick_segments: pacx_band_pick with the target target_t[s] / 64 for the frames of local segment s.  With
 * all targets equal it gives pacx_band_pick's outputs bit for bit.
 *   target_t: int32 [n_seg] in device memory, targets in grid units (64 per dB)
 *
 * PACX_E_UNSUPPORTED on a handle created with use_vq or use_sbr.  PACX_E_ARG for a null pointer, a bad count, seg_cf
 * outside [1, PACX_SEG_CF_MAX], first_off outside [0, seg_cf), bounds that are not finite, inverted, off the grid or more than
 * PACX_PROFILE_MAX targets apart.
 */
int pacx_band_profile_segments(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                               const int32_t *cap_alloc, int64_t seg_cf, int64_t first_off, double nmr_lo_db,
                               double nmr_hi_db, int64_t *profile, void *stream);
int pacx_profile_solve_segments(pacx_handle *h, int64_t n_seg, const int64_t *profile, const int64_t *limit_bytes,
                                double nmr_lo_db, double nmr_hi_db, pacx_rate_result *result, int64_t *worst_above,
                                void *stream);
int pacx_profile_clamp_add(pacx_handle *h, int64_t n_seg, const int64_t *profile, const pacx_rate_result *result,
                           double nmr_lo_db, double nmr_hi_db, int64_t *stream_profile, void *stream);
int pacx_band_pick_segments(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                            int64_t seg_cf, int64_t first_off, const int32_t *target_t, int32_t *bit_alloc,
                            int32_t *n_bytes, uint8_t *capped, void *stream);

/* ---- the same on a rate curve: BitAlloc budgets solved piece by piece ---- */

/*
 * pacx_rate_solve needs the whole stream's rate curve resident for the same reason pacx_band_solve does.  With pick,
 * bytes and total of pacx_rate_solve (above), word for word, [t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db] and
 * G = t_hi - t_lo + 1 <= PACX_PROFILE_MAX:
 *
 *   pacx_rate_profile:           profile[g] += total((t_lo + g) / 64) over the n_cf channel-frames given
 *   pacx_rate_profile_segments:  row_s[g] += sum over the piece's channel-frames cf in local segment
 *                                s = (first_off + cf) / seg_cf of (bytes(cf, (t_lo + g) / 64) + 4 where bytes > 0)
 *
 * The whole stream is the one-segment case: one kernel serves both.  The calls ADD to what profile holds -- the caller
 * zeroes it before the first piece -- and integer sums make the result independent of how the stream is cut and of the
 * order of execution; n_cf = 0 is a valid call that adds nothing.  On such profiles pacx_profile_solve is
 * pacx_rate_solve's decision, pacx_profile_solve_segments per row is pacx_rate_solve_segments', and with
 * pacx_profile_clamp_add pacx_rate_solve_peak's: those three work on rows alone.
 *
 * It is not G picks.  worst[j] <= t / 64 is 64 worst[j] <= t (both scalings are exact), so entry j of a unit passes from
 * the grid index e_j = ceil(64 worst[j]) - t_lo on -- 0 where that is at or below t_lo, never where the entry is NaN,
 * +inf or above nmr_hi_db, decided by comparisons in double before any conversion to an integer -- and the pick at g
 * is pacx_rate_solve's bisection with ok(j) := e_j <= g: the cap test on entry J first (a capped unit takes J), the
 * same halvings, a J that would leave its row cut to the row, a unit with steps < 0 does not exist, a frame without
 * units adds nothing, a short-coded frame's eight units are summed before the bytes are taken.  A workgroup of 1024
 * threads walks a contiguous run of frames; per frame it turns the row of worst into 16-bit e_j in LDS with the row of
 * bits beside them, every thread runs the bisection for the grid entries it owns, and the bytes it holds in registers
 * go to the row of the segment it is in whenever that changes and at its end, one 64-bit atomicAdd per entry.  A row
 * of more than 8 x 513 entries (no pacx_rate_curve_layout gives one) is read in place instead, with the comparison
 * 64 worst[j] <= t_lo + g itself.  One launch, no host wait.
 *
 *   worst, bits, steps, row, sub_stride: a curve as pacx_rate_curve_batch writes it (row >= 7 sub_stride + 1)
 *   seg_cf, first_off:  as pacx_band_profile_segments;  n_seg = ceil((first_off + n_cf) / seg_cf)
 *   profile (in/out):   int64 [G], of the segmented call [n_seg][G], in device memory; rows beyond n_seg are not touched
 *
 * pacx_rate_pick: pick(unit, T) for every unit at T = target_nmr_db, on the arrays alone, one channel-frame per thread:
 * what pacx_rate_solve's last launch writes at the t it returns.  The call is defined on the grid: target_nmr_db is a
 * finite multiple of 1 / 64 dB, at most 2^20 dB in magnitude.  pacx_rate_pick_segments: the same with the target
 * target_t[s] / 64 for the frames of local segment s; with all targets equal it gives pacx_rate_pick's outputs bit for
 * bit, with the targets of pacx_rate_solve_segments its outputs.  Neither keeps state in the handle.
 *   target_t: int32 [n_seg] in device memory, targets in grid units (64 per dB)
 *   budget (out): int32 [n_cf][8];  n_bytes (out): int32 [n_cf];  capped (out): uint8 [n_cf] -- pacx_rate_solve's layout
 *
 * PACX_E_UNSUPPORTED on a handle created with use_vq or use_sbr.  PACX_E_ARG for a null pointer, a bad count, a bad
 * row, seg_cf outside [1, PACX_SEG_CF_MAX], first_off outside [0, seg_cf), a target off the grid, bounds that are not
 * finite, inverted, off the grid or more than PACX_PROFILE_MAX targets apart.
 */
int pacx_rate_profile(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                      const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db, int64_t *profile,
                      void *stream);
int pacx_rate_profile_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                               const int32_t *bits, const int32_t *steps, int64_t seg_cf, int64_t first_off,
                               double nmr_lo_db, double nmr_hi_db, int64_t *profile, void *stream);
int pacx_rate_pick(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                   const int32_t *bits, const int32_t *steps, double target_nmr_db, int32_t *budget, int32_t *n_bytes,
                   uint8_t *capped, void *stream);
int pacx_rate_pick_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                            const int32_t *bits, const int32_t *steps, int64_t seg_cf, int64_t first_off,
                            const int32_t *target_t, int32_t *budget, int32_t *n_bytes, uint8_t *capped, void *stream);

/* ---- a curve kept as thresholds: what a pick on the grid reads of it, in 16 bits an entry ---- */

/*
 * A chunked encode takes every chunk's curve twice, once for the profile and once for the pick, because a curve in
 * doubles is too large to keep.  The pick does not need the doubles.  Every target it is asked for is a point of the
 * 1/64 dB grid inside a known range, and there the decision on an entry x is the threshold the profiles above already
 * use.  With [t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db] and G = t_hi - t_lo + 1 <= PACX_PROFILE_MAX:
 *
 *   threshold(x) = 0                     where 64 x <= t_lo
 *                  ceil(64 x) - t_lo     where t_lo < 64 x <= t_hi
 *                  G ("never")           where x is NaN, +inf or above nmr_hi_db
 *
 * decided by comparisons in double before anything is converted to an integer (e_i of pacx_band_profile, e_j of
 * pacx_rate_profile).  x <= t / 64 holds iff threshold(x) <= t - t_lo for every grid target t of the range.  G <= 8193
 * fits 16 bits.
 *
 * The kept band curve, made by pacx_band_thresholds from a curve as pacx_band_curve_batch or pacx_vq_band_curve_batch
 * writes it:
 *   e              uint16 [n_cf][band_stride][PACX_BAND_CAND]
 *   kept_cap       int32 [n_cf][8], cap copied
 *   kept_cap_alloc uint8 [n_cf][band_stride]: cap_alloc (0 ... 16; a value outside 0 ... 255 saturates, no curve call
 *                  writes one)
 * EVERY entry is written: e = G for candidates i >= n_cand, for slots no band of the frame uses and for every slot of a
 * dropped hop, kept_cap_alloc = 0 in those slots.  Whether a unit exists is read from cap as pacx_band_pick reads it,
 * the band layout from the handle's tables.  The kept arrays are therefore a function of the curve's defined entries
 * alone, 33 band_stride + 32 bytes per channel-frame where the curve has 132 band_stride + 32.
 *
 * The kept rate curve, made by pacx_rate_thresholds from a curve as pacx_rate_curve_batch writes it:
 *   e              uint16 [n_cf][row]
 *   kept_bits      int32 [n_cf][row], not narrowed: the solves accept any int32
 *   kept_steps     int32 [n_cf][8], steps with a J that would leave its row cut to the row, as the pick cuts it
 * Entries no unit uses (outside [sb sub_stride, sb sub_stride + J] of every unit of the frame) hold e = G and
 * kept_bits = 0.  6 row + 32 bytes per channel-frame where the curve has 12 row + 32.
 *
 * The picks, for a grid target t of the range, g = t - t_lo:
 *   pacx_band_pick_thresholds  per band the smallest i, in ascending order, with e_i <= g; the miss rule, the cap rule
 *                              with cap_alloc, bits(unit), bytes(cf) and capped are pacx_band_pick's, word for word
 *   pacx_rate_pick_thresholds  pacx_rate_pick's bisection with ok(j) := e_j <= g: the cap test on entry J first, the
 *                              same halvings, a short-coded frame's eight units summed before the bytes are taken
 *   ..._segments               the same with the target target_t[s] for the frames of local segment
 *                              s = (first_off + cf) / seg_cf, as pacx_band_pick_segments / pacx_rate_pick_segments
 *                              take their segments; target_t: int32 [n_seg] in device memory, grid units (64 per dB)
 * One kernel serves a pair: the target by value is the one-segment case.  Outputs have the layouts of the picks on the
 * curve: bit_alloc int32 [n_cf][band_stride] or budget int32 [n_cf][8], then n_bytes int32 [n_cf], capped uint8 [n_cf].
 *
 * The contract: for every grid target of the range, every output equals that of pacx_band_pick / pacx_rate_pick (and
 * their _segments forms) on the curve the thresholds were made from, with the same range given to both calls here.
 * A target in target_t that lies outside the range is clamped into it; that is outside the contract.
 *
 * Handle and argument rules are those of pacx_band_profile / pacx_rate_profile and of the picks: a scalar handle with
 * the curve's band layout (a gain-shape stream uses its scalar sibling, as for pacx_band_pick); n_cf = 0 is a valid
 * call that does nothing; no state is kept in the handle and nothing waits for the device.  nmr and the band form's e
 * are 16-byte aligned (any slice of whole channel-frames of an aligned array is).  PACX_E_UNSUPPORTED on a handle
 * created with use_vq or use_sbr.  PACX_E_ARG for a null pointer, a bad count, a bad row, seg_cf or first_off, a
 * misaligned nmr or e, bounds that are not finite, inverted, off the grid or more than PACX_PROFILE_MAX targets apart,
 * and a target given by value that is off the grid or outside the range.
 */
int pacx_band_thresholds(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                         double nmr_lo_db, double nmr_hi_db, uint16_t *e, int32_t *kept_cap, uint8_t *kept_cap_alloc,
                         void *stream);
int pacx_band_pick_thresholds(pacx_handle *h, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                              const uint8_t *cap_alloc, double nmr_lo_db, double nmr_hi_db, double target_nmr_db,
                              int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, void *stream);
int pacx_band_pick_thresholds_segments(pacx_handle *h, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                                       const uint8_t *cap_alloc, int64_t seg_cf, int64_t first_off, double nmr_lo_db,
                                       double nmr_hi_db, const int32_t *target_t, int32_t *bit_alloc, int32_t *n_bytes,
                                       uint8_t *capped, void *stream);
int pacx_rate_thresholds(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                         const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db, uint16_t *e,
                         int32_t *kept_bits, int32_t *kept_steps, void *stream);
int pacx_rate_pick_thresholds(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const uint16_t *e,
                              const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db,
                              double target_nmr_db, int32_t *budget, int32_t *n_bytes, uint8_t *capped, void *stream);
int pacx_rate_pick_thresholds_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const uint16_t *e,
                                       const int32_t *bits, const int32_t *steps, int64_t seg_cf, int64_t first_off,
                                       double nmr_lo_db, double nmr_hi_db, const int32_t *target_t, int32_t *budget,
                                       int32_t *n_bytes, uint8_t *capped, void *stream);

/* ---- one target per stretch of a stream: the two solves, segment by segment ---- */

/*
 * pacx_rate_solve and pacx_band_solve know one size constraint: the whole batch within limit_bytes at one target.
 * These two take one limit per segment -- the segments of a stream that must each fit a size, or the items of a
 * batch that must not pay for one another -- and find one target per segment, in the same number of launches.
 *
 * Segments are stretches of consecutive channel-frames (cf = block * nCh + ch as everywhere; a caller who means
 * blocks multiplies by the channel count):
 *
 *   n_seg:        >= 1, bounded like n_cf
 *   seg_first:    int64 [n_seg + 1] in HOST memory: seg_first[0] = 0, non-decreasing, seg_first[n_seg] = n_cf;
 *                 segment s holds the channel-frames [seg_first[s], seg_first[s + 1]) and may be empty
 *   limit_bytes:  int64 [n_seg] in HOST memory, each >= 0 (the plain solves take their limit by value too)
 *   result (out): pacx_rate_result [n_seg] in device memory
 *
 * The contract: result[s] and the per-cf outputs in [seg_first[s], seg_first[s + 1]) are those of pacx_rate_solve /
 * pacx_band_solve called with that slice of every array and limit_bytes[s] -- grid, bounds (all segments share
 * nmr_lo_db and nmr_hi_db), decision, the met = 0 rule and the caveats about totals that are not monotone are the
 * plain solves', per segment.  An empty segment gives t = t_lo, met = 1, total = 0, as a plain solve with n_cf = 0.
 *
 * Both host arrays are checked on the host, copied before the call returns (the caller may free them at once) and
 * uploaded on `stream` through a pinned buffer of the handle's; a call waits for the upload of the segmented solve
 * before it on the same handle, and for nothing else.  The call is therefore not meant for stream capture into a
 * graph; its callers read the result back anyway.  On the device one state per segment lives in the handle beside
 * the boundaries: init and step kernels run one thread per segment, the pick kernels do the per-frame work described
 * above with the target taken from the frame's segment (found in at most ceil(log2(n_seg + 1)) halvings of the
 * boundaries) and the frame's bytes added to that segment's total: reduced on chip, then one 64-bit integer
 * atomicAdd per workgroup whose frames lie in one segment, one per segment present (pacx_band_solve_segments: per
 * wave) in a workgroup that straddles a boundary.  Frames of a segment whose answer is known are skipped until the
 * last pick, which writes the outputs.  2 + ceil(log2(t_hi - t_lo + 2)) pairs whatever the data, no host wait.
 * These kernels are the only solve there is: pacx_rate_solve and pacx_band_solve run them with n_seg = 1 and the
 * table {0, n_cf, limit_bytes} written on the device, so the contract above holds by construction.  Plain and
 * segmented solves may follow one another on a handle's stream in any order.
 *
 * Other arguments, PACX_E_UNSUPPORTED and PACX_E_ARG: as pacx_rate_solve / pacx_band_solve; PACX_E_ARG also for
 * n_seg < 1, a null seg_first or limit_bytes, boundaries that do not start at 0, decrease or do not end at n_cf, and
 * a negative limit.
 */
int pacx_rate_solve_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                             const int32_t *bits, const int32_t *steps, int64_t n_seg, const int64_t *seg_first,
                             const int64_t *limit_bytes, double nmr_lo_db, double nmr_hi_db, int32_t *budget,
                             int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result, void *stream);
int pacx_band_solve_segments(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                             const int32_t *cap_alloc, int64_t n_seg, const int64_t *seg_first,
                             const int64_t *limit_bytes, double nmr_lo_db, double nmr_hi_db, int32_t *bit_alloc,
                             int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result, void *stream);

/* ---- an average for the stream, a peak for every stretch of it: the two solves on two levels ---- */

/*
 * The whole-stream solves spend the bytes best, but a loud passage may take several times the nominal rate; the
 * segmented solves bound every segment, but a quiet segment cannot pass on what it does not need.  These two hold both
 * constraints: one target for the stream within limit_bytes, and a higher one only for a segment that would exceed
 * its peak at the stream's.
 *
 * Arguments as pacx_rate_solve_segments / pacx_band_solve_segments -- n_seg, seg_first and the bounds under the same
 * rules and the same host-side checks; the per-segment array of limits is here called peak_bytes -- and:
 *
 *   limit_bytes:         >= 0, by value, for the whole batch (a kernel argument, as the plain solves')
 *   floor (out):         int32 [n_seg] in device memory, u_s on the grid
 *   result (out):        pacx_rate_result [n_seg] in device memory
 *   result_stream (out): one pacx_rate_result in device memory
 *
 *   stage A   u_s      = the t that pacx_*_solve_segments(seg_first, peak_bytes) finds for segment s
 *                        (t_hi where the segment cannot be reached);   floor[s] = u_s
 *   stage B   T_s(t)   = max(t, u_s)
 *             total*(t) = sum over s of total_s(T_s(t)),  total_s = the plain solve's total over the frames of s
 *             the plain solve's decision, unchanged, on total* against limit_bytes: the probe of t_hi, met* = 0 and
 *             t* = t_hi if it does not fit, else the same bisection with lo = t_lo - 1, hi = t_hi  ->  t*, met*
 *   outputs   per cf: the pick's outputs at T_seg(cf)(t*)
 *             result_stream = { t*, met*, total*(t*) }
 *             result[s]     = { t: T_s(t*),  met: total_s(T_s(t*)) <= peak_bytes[s],  total: total_s(T_s(t*)) }
 *
 * What follows from it:
 *   - With peaks that never bind every u_s = t_lo, and every output is pacx_rate_solve's / pacx_band_solve's with
 *     limit_bytes (result[s] then carries t* and the segment's share of the total).
 *   - With a limit_bytes that never binds t* = t_lo, and every output is pacx_*_solve_segments' with peak_bytes.
 *   - A segment is pinned iff result[s].t > result_stream.t.
 *   - An empty segment gives floor = t_lo, met = 1, total = 0 (and t = t*).  n_cf = 0 gives t* = t_lo, met* = 1.
 *   - result[s].met is measured at the final target, not inherited from stage A.  Where total_s is non-increasing in
 *     the target, a segment that stage A could reach stays within its peak at any T_s >= u_s; band allocation with
 *     no capped unit in the segment is such a case (see pacx_band_curve_batch).  Elsewhere a unit leaves its cap as
 *     the target rises, or the budget curve's worst[j] is not monotone: the total may then rise, and met = 0 reports
 *     it.  This is the bisection's answer, as for the existing solves.  Nothing re-pins such a segment.
 *
 * On the device there stays one solve.  Stage A is the segmented solve's init and its pick / step pairs without the
 * last pair: after P - 1 pairs, P = 2 + ceil(log2(t_hi - t_lo + 2)), every segment's state holds u_s, and nothing
 * needs the outputs at it.  One kernel, a thread per segment, writes floor, clears the segments' totals and starts one
 * more state, the stream's, kept in the handle behind the segments'.  Stage B drives that state through P pairs with
 * the plain decision: its picks are the same two pick kernels in a second instance that takes every frame at
 * max(stream target, floor of its segment) -- before the last pick a workgroup adds all its frames to the stream's
 * total in one 64-bit integer atomicAdd, the last pick writes the per-cf outputs and adds per segment exactly as the
 * segmented solve's.  A last kernel with a thread per segment writes result[s] and sums the segments' totals into the
 * stream's, and one with a single thread writes result_stream.  In all
 *
 *     4 P + 1 kernel launches (2 P + 2 when n_cf = 0) and the one upload of seg_first and peak_bytes,
 *
 * fixed by t_lo, t_hi and whether there are frames; a segmented solve takes 2 P + 1.  No host wait between the
 * stages; the upload goes through the handle's pinned buffer under pacx_rate_solve_segments' rule.  All sums are
 * 64-bit integers: no result depends on the order of execution.  Plain, segmented and peak solves may follow one
 * another on a handle's stream in any order.
 *
 * PACX_E_UNSUPPORTED and PACX_E_ARG as pacx_*_solve_segments; PACX_E_ARG also for a negative limit_bytes and a null
 * floor or result_stream.
 */
int pacx_rate_solve_peak(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                         const int32_t *bits, const int32_t *steps, int64_t n_seg, const int64_t *seg_first,
                         const int64_t *peak_bytes, int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db,
                         int32_t *budget, int32_t *n_bytes, uint8_t *capped, int32_t *floor, pacx_rate_result *result,
                         pacx_rate_result *result_stream, void *stream);
int pacx_band_solve_peak(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                         int64_t n_seg, const int64_t *seg_first, const int64_t *peak_bytes, int64_t limit_bytes,
                         double nmr_lo_db, double nmr_hi_db, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                         int32_t *floor, pacx_rate_result *result, pacx_rate_result *result_stream, void *stream);

/*
 * The second pass: pacx_encode_pack_budget_batch with the allocation of every band given by the caller instead of a
 * budget per unit.  bit_alloc_in: int32 [n_cf][band_stride] (may be the bit_alloc output itself); a value below 2
 * is taken as 0 and one above maxMantBits as maxMantBits, slots no band uses are ignored, and bit_alloc receives
 * what was coded.  With the allocation of a pick it writes records of exactly the predicted lengths.  A
 * channel-frame whose record would not fit pacx_payload_stride with the allocation asked for (no pick gives one)
 * is coded without mantissa bits and flagged PACX_ST_RATE_CAP.  status carries the front end's bits and that one
 * only: no BitAlloc runs here.  Runs MDCT -> k_band_sanitize -> scale factors + mantissas -> pack on `stream`.
 */
int pacx_encode_pack_alloc_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                 const int32_t *bit_alloc_in, int32_t *overall_scale, int32_t *scale_factor,
                                 int32_t *bit_alloc, int32_t *mantissa, uint32_t *status, uint8_t *payload,
                                 int32_t *n_bytes, void *stream);

/* ---- the same for gain-shape streams: a band curve taken with the coder itself ---- */

/*
 * Without SBR the gain-shape (PVQ) coder is band by band as well: quantize_gain_shape codes a band from that band's
 * lines and its own allocation a_b (a_b lines_b bits, coder/gain_shape_quantize.py:476-512), the spill of unused bits
 * into the next band exists only in the SBR encoder (coder/codec.py:522-524), a record carries every band's
 * allocation, and its length is the scalar formula, nScaleBits + sum_b (nMantSizeBits + nScaleBits + a_b lines_b): the
 * size rule counts a scale factor per band that is not written (coder/pacfile.py:342-361).  So a band curve in
 * pacx_band_curve_batch's layout makes the pick and every solve above usable for gain-shape streams as they are.
 *
 * pacx_vq_band_curve_batch: outputs, layout, cap rule, dropped hops and -1 slots as pacx_band_curve_batch, for a handle
 * created with use_vq and without use_sbr (1024 lines, long and short blocks, one batch).  The front end runs once
 * (MDCT -> side chain -> masked threshold, as pacx_encode_vq_batch up to BitAlloc); then one pass per candidate
 * i = 1 ... n_cand - 1, n_cand = maxMantBits: every band of every unit at bits(i) = i + 1 through the gain-shape coder
 * (k_vq*), its payload through the gain-shape decoder to lines (k_vq_dec*), those through k_nmr, the row into column i.
 * "The decoder's lines" are the decoder's by construction.
 *
 *   nmr[b][0]            NMR_b with Xh = 0, as the scalar curve's
 *   nmr[b][i], i < n_cand   pacx_nmr_batch's NMR_b of the band coded with bits(i) lines_b bits
 *   a band whose lines are all zero (the coder gives it no bits whatever it is offered, coder/codec.py:352-353):
 *                        -inf at every candidate below n_cand, so that a pick gives it 0 bits at any target
 *   a pass that flags the channel-frame PACX_ST_VQ_UNDEFINED: +inf at that candidate for every band of the frame
 *   nmr[b][i], i >= n_cand  +inf
 *   cap                  32 J, J by pacx_rate_steps exactly as the scalar curve takes it
 *   cap_alloc            BitAlloc(double(32 J), maxMantBits, bands, SMR) with the all-zero bands set to 0: a unit coded
 *                        with it writes exactly the predicted length
 *
 * The noise of a gain-shape band is not monotone in its size (the pulse count and the split of the bits between gain
 * and shape move in steps): the pick's ascending scan is the right one here too.  The status bits the passes raise
 * stay in the passes' own words; the handle keeps the front end's (and BitAlloc's at the cap budget) as
 * pacx_band_curve_batch does.  The buffers of one pass -- a payload slot, the decoded lines, one row of k_nmr's three
 * outputs, the allocation and the status word per channel-frame -- are grow-only workspace of the handle, allocated by
 * the first call and from then on sized by pacx_reserve too.  The call enqueues a fixed number of launches -- the
 * front end, BitAlloc, and per pass the same kernels whatever the data -- and the host waits for none.  It is
 * n_cand - 1 runs of the coder and the decoder, and a run at a large size costs several times one at an ordinary rate:
 * from about 4 bits a line the frame-level walks (k_vq_frame, k_vq_dec_frame) hand their blocks to the band-by-band
 * kernels behind them (tools/vq_band_probe.py measures every size; README).
 *
 * The pick and the solves -- pacx_band_pick, pacx_band_solve, pacx_band_solve_segments, pacx_band_solve_peak -- read
 * band tables and header widths only, and they answer a use_vq handle with PACX_E_UNSUPPORTED as before: a C host
 * creates a second handle with the same sample rate, band tables and widths and without use_vq, and hands it the
 * arrays (the Python binding keeps that sibling per gain-shape handle, context.scalar_sibling).
 *
 * PACX_E_UNSUPPORTED on a handle created without use_vq or with use_sbr (there the bands interact, and the
 * reconstructed bands have no NMR an allocation controls); the other argument rules are pacx_band_curve_batch's,
 * except that an empty batch (n_frames = 0) returns at once whatever the output pointers, as pacx_encode_vq_batch does.
 */
int pacx_vq_band_curve_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, double max_bits_per_sample,
                             double *nmr, int32_t *cap, int32_t *cap_alloc, void *stream);

/*
 * The second pass: pacx_encode_vq_batch with the allocation of every band given by the caller.  bit_alloc_in: int32
 * [n_cf][band_stride] (may be the bit_alloc output itself), made representable as pacx_encode_pack_alloc_batch makes
 * it: below 2 -> 0, above maxMantBits -> maxMantBits, and all zeros with PACX_ST_RATE_CAP for a channel-frame whose
 * record would not fit pacx_payload_stride.  overall_scale, bit_alloc (the FINAL allocation: a band of zero gain
 * drops to 0), payload, n_bytes and status as pacx_encode_vq_batch writes them.  With the allocation of a pick on
 * pacx_vq_band_curve_batch's curve it writes records of exactly the predicted lengths.  Runs MDCT -> k_band_sanitize
 * -> the gain-shape coder on `stream`: no side chain, no mask, no BitAlloc.  PACX_E_UNSUPPORTED as above.
 */
int pacx_encode_vq_alloc_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                               const int32_t *bit_alloc_in, int32_t *overall_scale, int32_t *bit_alloc,
                               uint8_t *payload, int32_t *n_bytes, uint32_t *status, void *stream);

/* ---- a leaky bucket: the level of a decoder's buffer, and the solves under it ---- */
/* pacx_bucket_scan, pacx_band_solve_bucket and pacx_rate_solve_bucket (additive exports, ABI 7): declared in the
   companion header beside this one, which is part of this interface and is included nowhere else */
#include "pacx_bucket.h"
/* per-block targets under a bucket (additive exports, ABI 7): the second companion header, behind the first */
#include "pacx_bucket_pin.h"
/* the buffered solve in chunks, on kept thresholds (additive exports, ABI 7): the third companion header */
#include "pacx_bucket_kept.h"

#ifdef __cplusplus
}
#endif
#endif /* PACX_H */
