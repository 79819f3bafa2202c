/*
 * pacx_dev.h -- device-side views shared by the kernels and the C-ABI layer.
 */
#ifndef PACX_DEV_H
#define PACX_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pacx_exact.h"

#define PACX_N_LONG 2048      /* window length of a long block               */
#define PACX_M_LONG 1024      /* MDCT lines of a long block (nMDCTLines)      */
#define PACX_N_SHORT 256
#define PACX_M_SHORT 128
#define PACX_SUB 8            /* short sub-blocks per frame                   */
#define PACX_SHORT_FIRST 448  /* first sub-block starts here (long/2-short/2) */
#define PACX_MAX_PEAKS 512    /* strict local maxima of 1025 bins             */
/* payload slot of one channel-block, bytes and 32-bit words.  A record is 3 flag bits and, per (sub-)block,
   nScaleBits + nBands * (nMantSizeBits + nScaleBits) header bits and up to 16 bits per covered line, rounded up with
   the size rule's extra bit: at the widths 4 / 12 at most 2181 bytes (8 short bands), but 2193 with 16-bit size fields
   and 7 short bands.  The packers build a record in this many LDS words and copy it whole, so pacx_create refuses a
   handle whose longest record (its layouts and widths, every band at 16 bits) is longer; pacx_payload_stride()
   reports the slot */
#define PACX_PAYLOAD_STRIDE 2192
#define PACX_PAYLOAD_WORDS (PACX_PAYLOAD_STRIDE / 4)

/* Tables resident in HBM for the life of a handle (all float64 / complex128). */
struct PacxTables {
    const double *win_long;     /* [4][2048]                                  */
    const double *win_short;    /* [256]                                      */
    const double *hann_long;    /* [2048]                                     */
    const double *hann_short;   /* [256]                                      */
    const double *ones;         /* [2048] of 1.0: MDCT of pre-windowed data     */
    const double *kbd_long;     /* [2048] KBDWindow(alpha=4), coder/window.py:53-57 */
    const double *kbd_short;    /* [256]                                      */
    const double *hann_long_pcm;   /* hann_long  * 2/65535 (int16 side chain)   */
    const double *hann_short_pcm;  /* hann_short * 2/65535                      */
    const double2 *tw_long;     /* exp(-j pi (8n+1)/8192), n < 512            */
    const double2 *tw_short;    /* exp(-j pi (8n+1)/1024), n < 64             */
    const double2 *w512;        /* exp(-2 pi j m/512),  m < 512               */
    const double2 *w1024;       /* exp(-2 pi j k/1024), k < 512               */
    const double2 *w2048;       /* exp(-2 pi j k/2048), k <= 1024             */
    const double2 *w128;        /* exp(-2 pi j k/128),  k < 64                */
    const double2 *w256;        /* exp(-2 pi j k/256),  k <= 128              */
    const double *bark_long, *thresh_long;      /* [1024]                     */
    const double *bark_short, *thresh_short;    /* [128]                      */
    const double *bark_bin_long;     /* [1025] Bark of the long FFT bin frequencies i*fstep_long: BOUNDS for the
                                        side chain's masker screen only (C math library, never in a result) */
    const int32_t *band_lower_long, *band_lines_long;     /* [nb_long]        */
    const int32_t *band_lower_short, *band_lines_short;   /* [nb_short]       */
    const uint8_t *line_band_long;   /* [1024] band of each line              */
    const uint8_t *line_band_short;  /* [128]                                 */
    double norm_long, norm_short;    /* 4/(N^2 mean(hanning^2))               */
    double fstep_long, fstep_short;  /* rfftfreq step                         */
    double target_bps;
    int nb_long, nb_short;
    int n_scale_bits, n_mant_size_bits;
    int band_stride;
    /* gain-shape / SBR variants (coder/pacfile.py:703-705, 326-327) */
    int use_vq, use_sbr;
    int first_omitted;                /* first band of sbr.omitted_bands (they are the tail) */
    const int32_t *band_lines_long_alloc;   /* nLines with omitted bands counted as 1 */
    int guard;                        /* compute PACX_ST_GUARD (pacx_config.guard) */
};

struct PacxPcmView {
    const void *base;
    long long frame_stride, ch_stride, samp_stride;
    int n_ch;
};

/* one peak (tonal masker) as the mask kernel consumes it */
struct __attribute__((aligned(8))) PacxPeak {
    double z;       /* Bark of the energy-weighted frequency                  */
    double spl;     /* SPL of the two-bin energy                              */
    double slope;   /* -27 + 0.367*max(spl-40,0): upper-side slope, dB/Bark   */
};

/* a mixed (block-switched) batch splits into two independent chains -- long-coded frames and
   short-coded frames -- that the entry points put on different streams: the launchers take
   the part in the upper bits of their `mixed` argument (0 = both parts) */
#define PACX_PART_LONG  (1 << 4)
#define PACX_PART_SHORT (2 << 4)

/* outputs of the tail fused into the long mask kernel (k_psy.hip k_mask<1024, true>) */
struct MaskTail {
    const int32_t *overall;     /* [cf][8], from the MDCT kernel              */
    int32_t *bit_alloc;         /* [cf][band_stride]                          */
    int32_t *scale_factor;      /* [cf][band_stride]                          */
    int32_t *mantissa;          /* [cf][1024] line-indexed, optional          */
    uint32_t *status;           /* [cf]                                       */
    uint8_t *payload;           /* [cf][payload_stride], optional             */
    int32_t *n_bytes;           /* [cf]                                       */
    int payload_stride;
};

/* XCD-aware order.  Workgroups are handed to the 8 XCDs round-robin, so workgroup b runs on XCD b % 8.
   Consecutive channel-frames share a hop of PCM; giving every XCD a CONTIGUOUS run of frames keeps that
   shared hop in one XCD's L2 instead of fetching it from HBM once per XCD (a quarter of the hops were read
   twice).  Two remaps, which must give the same answer to "which XCD reads frame cf":
     - the persistent MDCT kernels (k_mdct_long_v2, k_mdct_long_x2p) run workgroup b as virtual workgroup
       pacx_xcd_block(b): XCD x takes the x-th eighth of the workgroups.  On the headline shape (256 workgroups of
       8 waves, n_cf a multiple of 2048) that is the frames with (cf / 256) % 8 == x;
     - the one-frame-per-workgroup kernels of the side chain (k_side_long, k_front_long), which read the same
       PCM at the same time on another stream, run block b on frame pacx_xcd_frame(b): the same assignment, so
       that the hop is in this XCD's L2 whichever kernel asks first. */
__device__ __forceinline__ unsigned pacx_xcd_block(unsigned b, unsigned n_blocks)
{
    return (n_blocks & 7u) ? b : (b & 7u) * (n_blocks >> 3) + (b >> 3);
}
__device__ __forceinline__ long long pacx_xcd_frame(unsigned b, unsigned n_blocks, long long n_cf)
{
    if ((n_cf & 2047) != 0 || n_blocks != (unsigned)n_cf)
        return b;
    const unsigned idx = b >> 3;
    return (long long)(idx >> 8) * 2048 + (b & 7u) * 256 + (idx & 255u);
}

/* workspace of pacx_index_body (k_index.hip, body_index.h): byte offsets into one allocation of the handle,
   sized by the call (pacx_index_ws_bytes) */
struct PacxIndexWs {
    long long n_seg, n_groups;
    size_t tab;       /* uint32 [n_seg][PACX_IX_ENTRIES]     segment maps                     */
    size_t gtab;      /* uint64 [n_groups][PACX_IX_ENTRIES]  composed groups                  */
    size_t gentry;    /* int32 [n_groups]   entry offset of each group                        */
    size_t gbase;     /* int64 [n_groups]   first record number of each group                 */
    size_t entry;     /* int32 [n_seg]      entry offset of each segment, -1 off the chain    */
    size_t base;      /* int64 [n_seg]      first record number of each segment               */
    size_t fin;       /* int64 [3]          the call's result as the stitch knows it          */
};

#endif
