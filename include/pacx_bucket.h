/*
 * pacx_bucket.h -- the leaky-bucket section of include/pacx.h: the level of a decoder's buffer over the hops of a
 * stream and the two solves under it.  Included by pacx.h, inside its extern "C" block and behind the types it uses
 * (pacx_handle, pacx_rate_result); not for inclusion on its own.  Additive exports of ABI 7.
 */
#ifndef PACX_BUCKET_H
#define PACX_BUCKET_H
#ifndef PACX_H
#error "include pacx.h, which includes this header"
#endif

/*
 * Every constraint of the solves in pacx.h is a sum over an aligned stretch of blocks.  A transport or a hardware decoder states another
 * one: drain bytes leave my buffer per block, it holds size bytes, it must never overflow (the bit reservoir, VBV).
 * A hop h is n_ch consecutive channel-frames, cf = h n_ch + ch, in stream order; levels are int64 in units of
 * 1 / 65536 byte ("q16"), so a fractional drain is exact integer arithmetic:
 *
 *   x_h   = sum over ch of (n_bytes[cf] > 0 ? n_bytes[cf] + 4 : 0)      the terms of total(T) of pacx_rate_solve
 *   X_h   = x_h << 16
 *   F_0   = start_q16
 *   L_h   = F_h + X_h                      the level right after hop h's records arrive
 *   F_h+1 = max(0, L_h - drain_q16)        one hop of draining, never below empty
 *   total      = sum x_h
 *   peak_q16   = max(start_q16, max_h L_h)
 *   peak_hop   = the first h with L_h == peak_q16; -1 if no L_h is above start_q16 (the peak is the start level) or
 *                n_hops == 0
 *   first_over = the first h with L_h > size_bytes << 16, -1 if none
 *   end_q16    = F_n_hops                  the start of the next piece: the scan of a stream in pieces is exact (a
 *                                          piece starts within the buffer; an end_q16 above it follows an overflow)
 *
 * Domain: n_ch >= 1; 0 <= n_hops n_ch <= 2^30; drain_q16 >= 0; 0 <= size_bytes <= 2^40; 0 <= start_q16 <=
 * size_bytes << 16: anything else is PACX_E_ARG.  Entries of n_bytes (device memory, not checked) lie in [0, 65535];
 * a negative entry counts as 0.  Inside this domain nothing leaves int64: total <= 2^30 65539 < 2^47, and every level
 * is at most start_q16 + (total << 16) <= 2^56 + 2^46 65539 < 2^62 + 2^57.  A drain above that bound empties the
 * bucket at every hop exactly as the bound itself does, and is taken as the bound.
 *
 * F -> max(lo, F + s) is closed under composition -- a hop is (s, lo) = (X_h - drain, 0), "A then B" is
 * (sA + sB, max(loB, loA + sB)) -- so the levels are an associative scan: one workgroup of 1024 threads, a hop per
 * thread, walks the hops 1024 at a time (64-lane shuffles, the waves' totals through LDS, the carry in a register).
 * 64-bit integers throughout, no atomics, no floating point: the result does not depend on the order of execution.
 *
 *   level (out):  int64 [n_hops] in device memory, L_h; may be NULL
 *   result (out): device memory
 * n_hops = 0 is valid: total = 0, peak_q16 = end_q16 = start_q16, both hop fields -1.  The call is defined on arrays
 * alone and answers any handle.  One launch on `stream`; PACX_E_ARG also for a null b or result, or a null n_bytes with
 * n_hops > 0.
 */
typedef struct pacx_bucket {
    int64_t drain_q16;            /* leaves the buffer per hop */
    int64_t size_bytes;           /* the buffer holds this much */
    int64_t start_q16;            /* its level before the first hop */
} pacx_bucket;

typedef struct pacx_bucket_result {
    int64_t total, peak_q16, peak_hop, first_over, end_q16;
} pacx_bucket_result;

int pacx_bucket_scan(pacx_handle *h, int64_t n_hops, int32_t n_ch, const int32_t *n_bytes, const pacx_bucket *b,
                     int64_t *level, pacx_bucket_result *result, void *stream);

/*
 * The buffered solves: pacx_band_solve / pacx_rate_solve with one more condition in the decision,
 *
 *   fits(t) := total(t) <= limit_bytes  &&  peak_q16(t) <= size_bytes << 16        (the scan of the pick's n_bytes at t)
 *
 * in place of total(t) <= limit_bytes, and the bisection otherwise word for word: met = 0 and t = t_hi when fits(t_hi)
 * fails, else lo = t_lo - 1, hi = t_hi, halved while hi - lo > 1.  peak(t) is no more monotone in t than total(t) is:
 * the answer is this bisection's -- fits holds at the t returned and failed at the last t tried below it -- as
 * documented for the plain solves.  The per-channel-frame outputs are those of pacx_band_pick / pacx_rate_pick at the t
 * returned, result is the plain solve's, bucket_result (device memory) the scan's at that t.  With a buffer that no
 * level reaches (size_bytes = 2^40 for any stream below a terabyte) every output is the plain solve's; with a
 * limit_bytes that never binds only the buffer decides.  n_cf = 0 gives t = t_lo, met = 1 and the scan of no hop.
 *
 * On the device: an init kernel, then 2 + ceil(log2(t_hi - t_lo + 2)) pairs of the pick kernel of
 * pacx_band_pick_segments / pacx_rate_pick_segments -- one segment, its target read from the solve's state -- and a step
 * kernel, the scan above over the n_bytes just written, whose thread 0 decides and writes the next target; the last
 * pair's pick runs at the target found and its step writes both results.  A fixed number of launches whatever the
 * data; the host waits for none and uploads nothing: the limit and the bucket travel as kernel arguments.  The state
 * lives in the handle beside the plain solves': solves of one handle belong on one stream.
 *
 * n_ch: channels of a hop, >= 1, n_cf a multiple of it (PACX_E_ARG otherwise); b under pacx_bucket_scan's rules; every
 * other argument rule and PACX_E_UNSUPPORTED as pacx_band_solve / pacx_rate_solve.
 */
int pacx_band_solve_bucket(pacx_handle *h, int64_t n_cf, int32_t n_ch, const double *nmr, const int32_t *cap,
                           const int32_t *cap_alloc, int64_t limit_bytes, const pacx_bucket *b, double nmr_lo_db,
                           double nmr_hi_db, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                           pacx_rate_result *result, pacx_bucket_result *bucket_result, void *stream);
int pacx_rate_solve_bucket(pacx_handle *h, int64_t n_cf, int32_t n_ch, int32_t row, int32_t sub_stride,
                           const double *worst, const int32_t *bits, const int32_t *steps, int64_t limit_bytes,
                           const pacx_bucket *b, double nmr_lo_db, double nmr_hi_db, int32_t *budget, int32_t *n_bytes,
                           uint8_t *capped, pacx_rate_result *result, pacx_bucket_result *bucket_result, void *stream);

#endif /* PACX_BUCKET_H */
