/*
 * pacx_launch.h -- every function of the library that crosses a translation unit without being part
 * of the C ABI: the kernel launchers and the sizing / view helpers the k_*.hip files define and
 * pacx_api.hip (or another k_*.hip) calls.  pacx_api.hip and each defining file include this header, and
 * the definitions are written qualified (void pacx_k::pacx_launch_mdct(...)): a definition whose
 * argument list differs from the declaration here does not compile, where an unqualified one would
 * be a new overload and show only as an unresolved symbol when the library is loaded.
 */
#ifndef PACX_LAUNCH_H
#define PACX_LAUNCH_H

#include "../../include/pacx.h"
#include "pacx_dev.h"

struct PvqTables;        /* pvq_dev.h */

namespace pacx_k {

/* k_mdct.hip, k_mdct2.hip (long frames of 16-byte-aligned int16 batches), k_mdct3.hip (those without flags) */
void pacx_launch_mdct(const PacxTables &T, const PacxPcmView &in, int dtype, int fast,
                      const uint8_t *flags, long long n_cf, int short_blocks, int mixed, int prewin,
                      double *lines, int32_t *scale_out, int scale_stride, uint32_t *status,
                      hipStream_t st);
void pacx_launch_mdct_v2(const PacxTables &T, const PacxPcmView &in, const uint8_t *flags, long long n_cf,
                         int skip_cur, double *lines, int32_t *scale_out, int scale_stride,
                         uint32_t *status_init, int n_cu, const int32_t *cf_list, const int32_t *cf_count,
                         hipStream_t st);
void pacx_launch_mdct_x2(const PacxTables &T, const PacxPcmView &in, long long n_cf, double *lines,
                         int32_t *scale_out, int scale_stride, uint32_t *status_init, int n_cu, hipStream_t st);

/* k_psy.hip */
void pacx_launch_side(const PacxTables &T, const PacxPcmView &in, int dtype, int fast,
                      const uint8_t *flags, long long n_cf, int short_blocks, int mixed,
                      PacxPeak *peaks, int32_t *n_peaks, int32_t *n_kept, double *sbr_mean,
                      int32_t *sbr_overall, hipStream_t st);
/* the fused front end of an all-long step (k_front_long): MDCT lines, overall scale (stride PACX_SUB, sub-block
   scales zeroed), status initialisation and the side chain of every frame, for 16-byte-aligned unit-stride int16
   batches without per-frame flags on handles without SBR */
void pacx_launch_front_long(const PacxTables &T, const PacxPcmView &in, long long n_cf, double *lines,
                            int32_t *overall_scale, uint32_t *status, PacxPeak *peaks, int32_t *n_peaks,
                            int32_t *n_kept, hipStream_t st);
void pacx_launch_mask(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                      int short_blocks, int mixed, const PacxPeak *peaks, const int32_t *n_peaks,
                      const double *lines, double *smr, double *thr_out, int n_cu,
                      const int32_t *list_long, const int32_t *list_short, const int32_t *counts,
                      const MaskTail *tail, hipStream_t st);
size_t pacx_smr_generic_lds(int n);
void pacx_launch_smr_generic(long long n_blocks, int n, int nb, const double *data, const double *lines,
                             const double *hann, const double *tw_cos, const double *tw_sin, double norm, double fstep,
                             const double *bark, const double *quiet, const int32_t *band_lower,
                             const int32_t *band_count, double *smr, double *thr_out, int32_t *n_peaks_out,
                             hipStream_t st);

/* k_quant.hip */
void pacx_launch_bitalloc(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                          int short_blocks, int mixed, int skip_long, const double *smr, int32_t *bit_alloc,
                          uint32_t *status, hipStream_t st);
void pacx_launch_quantize(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                          int short_blocks, int mixed, const double *lines, const int32_t *overall,
                          int overall_stride, const int32_t *bit_alloc, int32_t *scale_factor,
                          int32_t *mantissa, hipStream_t st);
void pacx_launch_pack(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                      const int32_t *overall, const int32_t *scale_factor, const int32_t *bit_alloc,
                      const int32_t *mantissa, const uint32_t *status, uint8_t *payload,
                      int payload_stride, int32_t *n_bytes, hipStream_t st);
void pacx_launch_tail(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, const double *smr,
                      const double *lines, const int32_t *overall, int32_t *bit_alloc, int32_t *scale_factor,
                      int32_t *mantissa, uint32_t *status, uint8_t *payload, int payload_stride,
                      int32_t *n_bytes, const int32_t *list_short, const int32_t *count_short, int skip_long,
                      hipStream_t st);
void pacx_launch_gather(long long n_cf, const uint8_t *payload, int payload_stride,
                        const int32_t *n_bytes, long long *chunk_buf, long long *offs_buf, uint8_t *body,
                        long long capacity, long long *total, hipStream_t st);

/* k_misc.hip */
void pacx_launch_frame_lists(const uint8_t *flags, long long n_frames, int n_ch, int32_t *list_long,
                             int32_t *list_short, int32_t *counts, hipStream_t st);
void pacx_launch_window(const double *win, long long n_rows, int len, const double *x, double *y,
                        hipStream_t st);
void pacx_launch_quant_elem(int op, long long n, const double *x, int scale, int a, int b, int64_t *out,
                            hipStream_t st);
void pacx_launch_dequant_elem(int op, long long n, const int64_t *codes, int scale, int a, int b, double *out,
                              hipStream_t st);
void pacx_launch_mdct_direct(long long n_rows, int a, int b, int inverse, const double *x, double *y, hipStream_t st);
void pacx_launch_bitalloc_generic(long long n, int nb, const int32_t *n_lines, const double *budget,
                                  int max_mant, const double *smr, int32_t *bits, hipStream_t st);
void pacx_launch_transient_f64(long long n_blocks, int n_ch, int n, const double *blocks, double thresh, uint8_t *out,
                               hipStream_t st);
void pacx_launch_transient(const PacxPcmView &in, long long n_hops, int hop, uint8_t *transient,
                           uint8_t *flags, hipStream_t st);

/* k_decode.hip */
void pacx_launch_imdct_plain(const PacxTables &T, long long n_rows, int short_blocks, const double *lines,
                             double *blocks, hipStream_t st);
void pacx_launch_sbr_scalar_lines(const PacxTables &T, long long n_cf, const uint8_t *cf_flags,
                                  const int32_t *scale_factor, const int32_t *bit_alloc, const int32_t *mantissa,
                                  double *lines, uint8_t *sbr_flag, int routing, hipStream_t st);
void pacx_launch_unpack(const PacxTables &T, long long n_cf, const uint8_t *payload, int payload_stride,
                        const long long *offsets, const int32_t *n_bytes, uint8_t *flags_out, int32_t *overall,
                        int32_t *scale_factor, int32_t *bit_alloc, int32_t *mantissa, uint32_t *status,
                        hipStream_t st);
void pacx_launch_decode(const PacxTables &T, long long n_blocks, int n_ch, const uint8_t *cf_flags,
                        const int32_t *overall, const int32_t *scale_factor, const int32_t *bit_alloc,
                        const int32_t *mantissa, const double *lines_in, double *blocks, int16_t *pcm,
                        hipStream_t st);
void pacx_launch_ola_tail(long long n_blocks, int n_ch, const double *blocks, double *tail, int flush, int16_t *pcm,
                          hipStream_t st);

/* k_index.hip */
size_t pacx_index_ws_bytes(long long n_body, PacxIndexWs *ws);
void pacx_launch_index(const PacxIndexWs &ws, char *mem, const uint8_t *body, long long n_body, int n_ch, int final,
                       long long max_records, long long *offsets, int32_t *n_bytes, long long *result, hipStream_t st);

/* k_nmr.hip */
void pacx_launch_nmr(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, const double *lines,
                     const double *dec_lines, const int32_t *overall, const double *thr, const uint32_t *status,
                     double *noise, double *mask, double *nmr_db, hipStream_t st);
void pacx_launch_nmr_summary(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                             const double *nmr_db, unsigned long long *summary, hipStream_t st);

/* k_rate.hip: the budget search of pacx_encode_pack_nmr_batch (one wave per long block / short sub-block; budget
   int32 [n_cf][8], long frames use [0]) and BitAlloc with the caller's budgets */
void pacx_launch_rate_search(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                             double target_nmr_db, double max_bits_per_sample, const double *lines,
                             const double *thr, const double *smr, const int32_t *overall, int32_t *budget,
                             int32_t *bit_alloc, uint32_t *status, hipStream_t st);
void pacx_launch_bitalloc_budget(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                                 const int32_t *budget, const double *smr, int32_t *bit_alloc, uint32_t *status,
                                 hipStream_t st);
/* the rate curve of pacx_rate_curve_batch (k_rate_search's units and evaluation, every step j = 0 ... J) */
void pacx_launch_rate_curve(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                            double max_bits_per_sample, int row, int sub_stride, const double *lines,
                            const double *thr, const double *smr, const int32_t *overall, const uint32_t *status,
                            double *worst, int32_t *bits, int32_t *steps, hipStream_t st);

/* The solve, the only one: one target per segment of consecutive channel-frames, found on stored curves.  A whole-
   stream solve (pacx_rate_solve, pacx_band_solve) is the solve of one segment.  Nothing here waits for the device. */
struct PacxSolve {
    void *ws;                         /* n_seg states of pacx_rate_solve_ws_bytes() bytes (a peak solve: one more) */
    long long *seg;                   /* device: seg_first [n_seg + 1], then limit [n_seg] */
    int n_seg;
    const long long *one_limit;       /* nullptr: seg is uploaded.  Else n_seg == 1, and the init kernel writes
                                         {0, n_cf, *one_limit} into seg itself: no copy from the host */
    long long n_cf;
    int t_lo, t_hi;                   /* the target range on the grid */
    pacx_rate_result *result;         /* [n_seg] */
};
size_t pacx_rate_solve_ws_bytes(void);
int pacx_rate_solve_pairs(int t_lo, int t_hi);
int pacx_segment_search_steps(int n_seg);
/* init and step: one thread per segment (k_rate.hip) */
void pacx_launch_solve_init_segments(const PacxSolve &v, hipStream_t st);
void pacx_launch_solve_step_segments(const PacxSolve &v, int final, hipStream_t st);

/* the driver: init, then pacx_rate_solve_pairs(t_lo, t_hi) pick / step pairs, the last of which writes the outputs.
   pick(search_steps, final) launches the solve's own pick kernel, which finds a frame's segment in
   pacx_segment_search_steps(n_seg) halvings (none for one segment: seg_first is not read); without frames no pick */
template <class Pick>
inline void pacx_solve_drive(const PacxSolve &v, hipStream_t st, Pick pick)
{
    const int pairs = pacx_rate_solve_pairs(v.t_lo, v.t_hi), search = pacx_segment_search_steps(v.n_seg);
    pacx_launch_solve_init_segments(v, st);
    for (int p = 0; p < pairs; ++p) {
        const int final = p == pairs - 1;
        if (v.n_cf > 0)
            pick(search, final);
        pacx_launch_solve_step_segments(v, final, st);
    }
}

/* the solve on a rate curve: a frame's units at the budgets the curve gives at its segment's target */
void pacx_launch_rate_solve_segments(const PacxSolve &v, int row, int sub_stride, const double *worst,
                                     const int32_t *bits, const int32_t *steps, int32_t *budget, int32_t *n_bytes,
                                     uint8_t *capped, hipStream_t st);

/* the pick on a rate curve at targets given with the call (k_rate.hip, k_rate_pick): frame cf takes
   target_t[(first_off + cf) / seg_cf] / 64; target_t == nullptr: every frame takes t_all / 64 */
void pacx_launch_rate_pick_segments(long long n_cf, int row, int sub_stride, const double *worst, const int32_t *bits,
                                    const int32_t *steps, long long seg_cf, long long first_off, const int32_t *target_t,
                                    int t_all, int32_t *budget, int32_t *n_bytes, uint8_t *capped, hipStream_t st);

/* k_rate_profile.hip: total(t / 64) of a rate curve added into profile [n_seg][G], row (first_off + cf) / seg_cf of
   frame cf, for every t of the range at once (G = t_hi - t_lo + 1 <= PACX_PROFILE_MAX); the whole stream is the
   one-segment case (seg_cf = PACX_SEG_CF_MAX, first_off = 0).  One launch */
void pacx_launch_rate_profile_segments(long long n_cf, int row, int sub_stride, const double *worst, const int32_t *bits,
                                       const int32_t *steps, long long seg_cf, long long first_off, int t_lo, int t_hi,
                                       int64_t *profile, hipStream_t st);

/* The second level (pacx_rate_solve_peak / pacx_band_solve_peak): a limit for the whole batch above the segments'
   peaks.  v is a segmented solve with the peaks as its limits and ws holding n_seg + 1 states: the last one is the
   stream's. */
struct PacxSolveStream {
    long long limit;                  /* for the whole batch: a kernel argument */
    int32_t *floor;                   /* [n_seg] */
    pacx_rate_result *result;         /* the stream's, one entry */
};
void pacx_launch_peak_init(const PacxSolve &v, const PacxSolveStream &p, hipStream_t st);
void pacx_launch_peak_step(const PacxSolve &v, const PacxSolveStream &p, int final, hipStream_t st);

/* the driver.  Stage A: pacx_solve_drive without its last pair -- after pacx_rate_solve_pairs - 1 pairs every
   segment's answer is in its state, and nothing needs the outputs at it.  Then the init of the second level (floors
   out, the stream's state started) and stage B: the same number of pairs as a solve, on the stream's state, with
   pick(search_steps, final, true) taking every frame at max(stream target, its segment's floor); the last step
   writes result[n_seg] (one launch) and the stream's (one more).  With P = pacx_rate_solve_pairs(t_lo, t_hi):
   4 P + 1 launches, 2 P + 2 without frames, whatever the data; nothing waits for the device. */
template <class Pick>
inline void pacx_peak_drive(const PacxSolve &v, const PacxSolveStream &p, hipStream_t st, Pick pick)
{
    const int pairs = pacx_rate_solve_pairs(v.t_lo, v.t_hi), search = pacx_segment_search_steps(v.n_seg);
    pacx_launch_solve_init_segments(v, st);
    for (int q = 0; q < pairs - 1; ++q) {
        if (v.n_cf > 0)
            pick(search, 0, false);
        pacx_launch_solve_step_segments(v, 0, st);
    }
    pacx_launch_peak_init(v, p, st);
    for (int q = 0; q < pairs; ++q) {
        const int final = q == pairs - 1;
        if (v.n_cf > 0)
            pick(search, final, true);
        pacx_launch_peak_step(v, p, final, st);
    }
}
void pacx_launch_rate_solve_peak(const PacxSolve &v, const PacxSolveStream &p, int row, int sub_stride,
                                 const double *worst, const int32_t *bits, const int32_t *steps, int32_t *budget,
                                 int32_t *n_bytes, uint8_t *capped, hipStream_t st);

/* k_band.hip: the band-by-band allocation of pacx_band_curve_batch / pacx_band_pick / pacx_band_solve_segments / _peak (nmr
   float64 [n_cf][band_stride][PACX_BAND_CAND], cap int32 [n_cf][8], cap_alloc int32 [n_cf][band_stride]; the solve is
   the one above with a pick of its own) and the sanitised copy of a caller's allocation (in == out allowed) */
void pacx_launch_band_curve(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                            double max_bits_per_sample, const double *lines, const double *thr, const double *smr,
                            const int32_t *overall, uint32_t *status, double *nmr, int32_t *cap, int32_t *cap_alloc,
                            hipStream_t st);
void pacx_launch_band_pick(const PacxTables &T, long long n_cf, double target, const double *nmr, const int32_t *cap,
                           const int32_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                           hipStream_t st);
/* the pick with one grid target per uniform segment: frame cf takes target_t[(first_off + cf) / seg_cf] / 64 */
void pacx_launch_band_pick_segments(const PacxTables &T, long long n_cf, long long seg_cf, long long first_off,
                                    const int32_t *target_t, const double *nmr, const int32_t *cap,
                                    const int32_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                                    hipStream_t st);
void pacx_launch_band_solve_segments(const PacxTables &T, const PacxSolve &v, const double *nmr, const int32_t *cap,
                                     const int32_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                                     hipStream_t st);
void pacx_launch_band_solve_peak(const PacxTables &T, const PacxSolve &v, const PacxSolveStream &p, const double *nmr,
                                 const int32_t *cap, const int32_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes,
                                 uint8_t *capped, hipStream_t st);
void pacx_launch_band_sanitize(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, const int32_t *in,
                               int32_t *out, uint32_t *status, int payload_stride, hipStream_t st);

/* k_profile.hip: total(t / 64) of a band curve added into profile [t_hi - t_lo + 1] for every t of the range at once
   (t_hi - t_lo + 1 <= PACX_PROFILE_MAX), and the solve's decision read from such a profile: one launch each */
void pacx_launch_band_profile(const PacxTables &T, long long n_cf, int t_lo, int t_hi, const double *nmr,
                              const int32_t *cap, const int32_t *cap_alloc, int64_t *profile, hipStream_t st);
void pacx_launch_profile_solve(const int64_t *profile, long long limit, int t_lo, int t_hi, pacx_rate_result *result,
                               hipStream_t st);

/* k_seg_profile.hip: the profile per uniform segment of a piece (profile [n_seg][G], row (first_off + cf) / seg_cf of
   frame cf, added to), the solve's decision per row against limit_bytes [n_seg] on the device with the row's maximum
   from the target found on (worst_above, may be null), and the rows clamped below their targets summed into one
   stream profile [G]: one launch each */
void pacx_launch_band_profile_segments(const PacxTables &T, long long n_cf, long long seg_cf, long long first_off,
                                       int t_lo, int t_hi, const double *nmr, const int32_t *cap,
                                       const int32_t *cap_alloc, int64_t *profile, hipStream_t st);
void pacx_launch_profile_solve_segments(long long n_seg, const int64_t *profile, const int64_t *limit_bytes, int t_lo,
                                        int t_hi, pacx_rate_result *result, int64_t *worst_above, hipStream_t st);
void pacx_launch_profile_clamp_add(long long n_seg, const int64_t *profile, const pacx_rate_result *result, int t_lo,
                                   int t_hi, int64_t *stream_profile, hipStream_t st);

/* k_kept.hip: a curve as the 16-bit grid indices from which its entries pass (G = t_hi - t_lo + 1: never), and the
   picks on them.  Band: e uint16 [n_cf][band_stride][PACX_BAND_CAND] (16-byte aligned, as nmr), cap copied, cap_alloc
   as bytes.  Rate: e uint16 [n_cf][row], bits copied (0 where no unit uses the entry), steps cut to the row.  The
   picks: frame cf takes target_t[(first_off + cf) / seg_cf], target_t == nullptr: every frame takes t_all; grid units,
   clamped into [t_lo, t_hi].  One launch each */
void pacx_launch_band_thresholds(const PacxTables &T, long long n_cf, int t_lo, int t_hi, const double *nmr,
                                 const int32_t *cap, const int32_t *cap_alloc, uint16_t *e, int32_t *kept_cap,
                                 uint8_t *kept_cap_alloc, hipStream_t st);
void pacx_launch_band_pick_thresholds(const PacxTables &T, long long n_cf, long long seg_cf, long long first_off,
                                      const int32_t *target_t, int t_all, int t_lo, int t_hi, const uint16_t *e,
                                      const int32_t *cap, const uint8_t *cap_alloc, int32_t *bit_alloc, int32_t *n_bytes,
                                      uint8_t *capped, hipStream_t st);
void pacx_launch_rate_thresholds(long long n_cf, int row, int sub_stride, int t_lo, int t_hi, const double *worst,
                                 const int32_t *bits, const int32_t *steps, uint16_t *e, int32_t *kept_bits,
                                 int32_t *kept_steps, hipStream_t st);
void pacx_launch_rate_pick_thresholds(long long n_cf, int row, int sub_stride, long long seg_cf, long long first_off,
                                      const int32_t *target_t, int t_all, int t_lo, int t_hi, const uint16_t *e,
                                      const int32_t *bits, const int32_t *steps, int32_t *budget, int32_t *n_bytes,
                                      uint8_t *capped, hipStream_t st);

/* k_bucket.hip: the level of a leaky bucket over the hops of n_bytes (pacx_bucket_scan: one launch of one workgroup)
   and the buffered solve: the plain solve's bisection with the bucket's peak as a second condition */
void pacx_launch_bucket_scan(long long n_hops, int n_ch, const int32_t *n_bytes, const pacx_bucket &b, int64_t *level,
                             pacx_bucket_result *result, hipStream_t st);
struct PacxBucketSolve {
    void *ws;                         /* one state of pacx_bucket_ws_bytes() bytes */
    long long n_cf;
    int n_ch;                         /* n_cf / n_ch hops */
    int t_lo, t_hi;                   /* the target range on the grid */
    long long limit;                  /* for the whole batch, and the bucket: kernel arguments */
    pacx_bucket bucket;
    const int32_t *n_bytes;           /* what the picks write and the steps scan */
    pacx_rate_result *result;
    pacx_bucket_result *bucket_result;
};
size_t pacx_bucket_ws_bytes(void);
const int32_t *pacx_bucket_target(const PacxBucketSolve &v);      /* device: the word a pick reads its target from */
void pacx_launch_bucket_init(const PacxBucketSolve &v, hipStream_t st);
void pacx_launch_bucket_step(const PacxBucketSolve &v, int final, hipStream_t st);

/* the driver: init (the target word at t_hi), then pacx_rate_solve_pairs(t_lo, t_hi) pairs of pick(target_t) -- the
   one-segment pick of pacx_launch_band_pick_segments / pacx_launch_rate_pick_segments at the state's target word -- and
   the step that scans what it wrote and decides; the last pick runs at the target found and the last step writes both
   results.  2 pairs + 1 launches (pairs + 1 without frames), whatever the data; nothing waits for the device */
template <class Pick>
inline void pacx_bucket_drive(const PacxBucketSolve &v, hipStream_t st, Pick pick)
{
    const int pairs = pacx_rate_solve_pairs(v.t_lo, v.t_hi);
    pacx_launch_bucket_init(v, st);
    for (int p = 0; p < pairs; ++p) {
        if (v.n_cf > 0)
            pick(pacx_bucket_target(v));
        pacx_launch_bucket_step(v, p == pairs - 1, st);
    }
}

/* k_bucket_pin.hip: the level through every hop (pacx_bucket_through: one launch of one workgroup) and the pinned
   solves of include/pacx_bucket_pin.h: a target per hop, the phase's level or the hop's pin */
void pacx_launch_bucket_through(long long n_hops, int n_ch, const int32_t *n_bytes, const pacx_bucket &b, int64_t *level,
                                int64_t *through, pacx_bucket_result *result, hipStream_t st);
struct PacxPinSolve {
    void *ws;                         /* pacx_pin_ws_head() + n_hops pacx_pin_ws_unit() bytes: state, F_h, pins */
    long long n_cf;
    int n_ch;                         /* n_cf / n_ch hops */
    int t_lo, t_hi;                   /* the target range on the grid */
    int pin_step_t, max_phases;
    long long limit;                  /* for the whole batch, and the bucket: kernel arguments */
    pacx_bucket bucket;
    const int32_t *n_bytes;           /* what the picks write and the kernels scan */
    int32_t *target_t, *phase_of;     /* [n_hops]: what the picks read; the phase that pinned a hop */
    pacx_rate_result *result;
    pacx_bucket_result *bucket_result;
    pacx_pin_result *pin_result;
};
size_t pacx_pin_ws_head(void);
size_t pacx_pin_ws_unit(void);        /* the head is a whole number of units */
void pacx_launch_pin_init(const PacxPinSolve &v, hipStream_t st);
void pacx_launch_pin_step(const PacxPinSolve &v, hipStream_t st);
void pacx_launch_pin_freeze(const PacxPinSolve &v, hipStream_t st);
void pacx_launch_pin_finish(const PacxPinSolve &v, hipStream_t st);

/* the driver: init (every target t_hi); per phase pacx_rate_solve_pairs(t_lo, t_hi) pairs of pick() -- the pick of
   pacx_launch_band_pick_segments / pacx_launch_rate_pick_segments with seg_cf = n_ch at v.target_t -- and the step,
   then the pick at A(q) and the freeze; last the pick at the targets returned and the finish.
   max_phases (2 pairs + 2) + 3 launches (max_phases (pairs + 1) + 2 without frames), whatever the data; nothing waits
   for the device.  A finished solve's kernels return at once; its picks still run */
template <class Pick>
inline void pacx_pin_drive(const PacxPinSolve &v, hipStream_t st, Pick pick)
{
    const int pairs = pacx_rate_solve_pairs(v.t_lo, v.t_hi);
    pacx_launch_pin_init(v, st);
    for (int k = 0; k < v.max_phases; ++k) {
        for (int p = 0; p < pairs; ++p) {
            if (v.n_cf > 0)
                pick();
            pacx_launch_pin_step(v, st);
        }
        if (v.n_cf > 0)
            pick();
        pacx_launch_pin_freeze(v, st);
    }
    if (v.n_cf > 0)
        pick();
    pacx_launch_pin_finish(v, st);
}

/* k_bucket_kept.hip: the buffered solve for a stream in chunks (include/pacx_bucket_kept.h).  The bytes of a pick on a
   kept curve at n_targets grid targets read from the device (n_bytes_t [n_targets][n_cf]; targets clamped into
   [t_lo, t_hi]), the scans of n_targets rows folded into acc, and the tree of the bisection's decisions on the
   caller's state block.  One launch each; nothing waits for the device */
void pacx_launch_band_bytes_thresholds(const PacxTables &T, long long n_cf, int n_targets, const int32_t *target_t,
                                       int t_lo, int t_hi, const uint16_t *e, const int32_t *cap, const uint8_t *cap_alloc,
                                       int32_t *n_bytes_t, hipStream_t st);
void pacx_launch_rate_bytes_thresholds(long long n_cf, int row, int sub_stride, int n_targets, const int32_t *target_t,
                                       int t_lo, int t_hi, const uint16_t *e, const int32_t *bits, const int32_t *steps,
                                       int32_t *n_bytes_t, hipStream_t st);
void pacx_launch_bucket_scan_targets(long long n_hops, int n_ch, int n_targets, const int32_t *n_bytes_t,
                                     long long row_stride, long long drain_q16, long long size_bytes, long long hop_off,
                                     pacx_bucket_result *acc, hipStream_t st);
void pacx_launch_bucket_tree_begin(void *state, int t_lo, int t_hi, int levels, long long start_q16, int32_t *target_t,
                                   pacx_bucket_result *acc, hipStream_t st);
void pacx_launch_bucket_tree_step(void *state, long long limit, long long size_bytes, long long start_q16, int levels,
                                  int32_t *target_t, pacx_bucket_result *acc, pacx_rate_result *result,
                                  pacx_bucket_result *bucket_result, hipStream_t st);

/* k_vq_band.hip: what pacx_vq_band_curve_batch does around its passes through the gain-shape coder, its decoder and
   k_nmr.  cap / budget int32 [n_cf][8] (-1 / 0 where there is no unit); alloc, cap_alloc int32 [n_cf][band_stride];
   row float64 [n_cf][band_stride], k_nmr's; status_front: the front end's words, status_pass: the pass's own (nullptr
   for candidate 0, which no coder ran for) */
void pacx_launch_vq_band_cap(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf,
                             double max_bits_per_sample, const uint32_t *status, int32_t *cap, int32_t *budget,
                             hipStream_t st);
void pacx_launch_vq_band_fill(const PacxTables &T, long long n_cf, int bits, const uint32_t *status_in, int32_t *alloc,
                              uint32_t *status_out, hipStream_t st);
void pacx_launch_vq_band_store(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, int cand,
                               const double *row, const int32_t *alloc, const uint32_t *status_front,
                               const uint32_t *status_pass, double *nmr, hipStream_t st);
void pacx_launch_vq_band_zero(const PacxTables &T, const uint8_t *flags, int n_ch, long long n_cf, const int32_t *alloc,
                              const uint32_t *status_front, int32_t *cap_alloc, hipStream_t st);

/* k_vq.hip (sizes_long / sizes_short: vector dimension of every band as the coder sees it) */
void pacx_launch_vq(const PacxTables &T, const void *vq_view, const uint8_t *flags, int n_ch, long long n_cf,
                    const double *lines, const int32_t *overall, int32_t *bit_alloc, const double *sbr_mean,
                    uint32_t *status, uint8_t *payload, int payload_stride, int32_t *n_bytes,
                    unsigned *unit_words, int32_t *unit_bits, pacx_vq_entry *log, int32_t *log_count,
                    int log_cap, int stage, const int32_t *cf_list, const int32_t *cf_count, int frame, int bfs,
                    hipStream_t st);
size_t pacx_vq_view_size(void);
void pacx_vq_view_fill(void *dst, const PvqTables &tab, double log_mu1, const double *log2_tan,
                       const int32_t *sizes_long, int nb_long, const int32_t *sizes_short, int nb_short);

/* k_vq_dec.hip */
size_t pacx_vqdec_view_size(void);
void pacx_vqdec_view_fill(void *dst, const PvqTables &tab, const double *log2_tan, const double *gauss,
                          int gauss_r, const double *line_freq, const int32_t *sizes_long, int nb_long,
                          const int32_t *sizes_short, int nb_short);
void pacx_launch_vq_dec(const PacxTables &T, const void *view, long long n_cf, const uint8_t *payload,
                        int payload_stride, const long long *offsets, const int32_t *n_bytes,
                        uint8_t *cf_flags, int32_t *overall, int32_t *bit_alloc, double *lines,
                        uint8_t *sbr_flag, uint32_t *status, int frame, hipStream_t st);
void pacx_launch_sbr_recon(const PacxTables &T, const void *view, long long n_cf, const uint8_t *sbr_flag,
                           double *lines, uint32_t *status, hipStream_t st);

}  // namespace pacx_k

#endif
