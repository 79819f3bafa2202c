/*
 * pacx_bucket_pin.h -- per-block targets under a leaky bucket: the level through every hop and the two pinned solves.
 * Included by pacx.h right behind pacx_bucket.h, inside its extern "C" block; not for inclusion on its own.  Additive
 * exports of ABI 7.  Notation is pacx_bucket.h's: hops of n_ch channel-frames, x_h, X_h = x_h << 16, L_h, F_h, the
 * bucket b, size_q16 = size_bytes << 16.
 */
#ifndef PACX_BUCKET_PIN_H
#define PACX_BUCKET_PIN_H
#ifndef PACX_BUCKET_H
#error "include pacx.h, which includes pacx_bucket.h and then this header"
#endif

/*
 * The buffered solves of pacx_bucket.h find ONE target under a size and a buffer: the loudest stretch the buffer cannot
 * absorb sets the quality of all of it.  The solves below keep the stream's target wherever the buffer allows and pin
 * a higher one only where it does not.
 *
 * The level through a hop.
 *
 *   R_h       = X_h + max(0, R_h+1 - drain_q16)     nothing behind the last hop: the forward recursion from an empty
 *                                                    buffer over the hops in reverse order
 *   through_h = F_h + R_h  ( = L_h + R_h - X_h )
 *
 * the highest level that any stretch of consecutive hops containing h brings the buffer to, the start level counted
 * as a stretch that begins before hop 0.  Hop h lies in a stretch that overflows if and only if through_h > size_q16.
 * F_h and R_h hold the bytes of disjoint hops, so through_h stays below the bound of pacx_bucket.h (2^62 + 2^57).
 *
 * pacx_bucket_through: pacx_bucket_scan's domain, argument rules and result, and
 *   level (out):   int64 [n_hops] in device memory, L_h; may be NULL
 *   through (out): int64 [n_hops] in device memory; not NULL when n_hops > 0
 * One launch of one workgroup of 1024 threads: the scan of pacx_bucket_scan forward, F_h left in `through`, and the
 * same scan over the reversed hops from an empty buffer, which adds R_h.  Defined on arrays alone; answers any handle.
 */
int pacx_bucket_through(pacx_handle *h, int64_t n_hops, int32_t n_ch, const int32_t *n_bytes, const pacx_bucket *b,
                        int64_t *level, int64_t *through, pacx_bucket_result *result, void *stream);

/*
 * The pinned solves.  Inputs: the curve, n_cf, n_ch, limit_bytes, b and [t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db] of
 * pacx_*_solve_bucket; pin_step_t >= 1 in grid units (1 / 64 dB); max_phases = K in [1, PACX_PIN_PHASES_MAX].
 *
 * State per hop: pin[h], initially t_lo - 1 ("free").  An assignment at level p is A(p)[h] = max(p, pin[h]); bytes(A)
 * is pacx_*_pick_segments with one segment per hop (seg_cf = n_ch); fits(A) := total <= limit_bytes && peak_q16 <=
 * size_q16, both from pacx_bucket_scan of those bytes.  For phase k = 0 ... K - 1, until finished:
 *
 *   1. hi0 = t_hi for k = 0, else p_k-1.  In phase 0, if fits(A(t_hi)) fails: met = 0, T = t_hi, finished -- the
 *      buffered solves' rule, and phases = 0.
 *   2. lo = t_lo - 1, hi = hi0; while hi - lo > 1: mid = floor((lo + hi) / 2); fits(A(mid)) ? hi = mid : lo = mid.
 *      p_k = hi.
 *   3. p_k == t_lo: finished.
 *   4. q = max(t_lo, p_k - pin_step_t), and through of bytes(A(q)): every FREE hop with through_h > size_q16 gets
 *      pin[h] = p_k and phase_of[h] = k.  None froze: finished (only the size binds).
 *
 * Outputs: T = the last p_k; target_t[h] = max(T, pin[h]); phase_of[h] (-1: free); the pick's per-channel-frame
 * outputs at target_t; result = {T, met, total} and bucket_result, the scan of those bytes; pin_result.phases, the
 * number of bisections run, and pin_result.open, 1 if phase K - 1 still froze a hop: the phases ran out while the
 * buffer bound.
 *
 * By construction: phase 0 is pacx_*_solve_bucket word for word, and with max_phases = 1 every shared output equals
 * its; with a buffer no level reaches every output is the plain solve's, phases = 1 and no hop is pinned; the
 * assignment returned is the last one measured to fit whenever met = 1 (no monotonicity is assumed for that); no hop
 * ends above the one-target solve's target.  pin_step_t = 1 is progressive filling on the full grid; larger steps trade
 * at most pin_step_t of quality on pinned hops for fewer phases.
 *
 * On the device: an init kernel; per phase pacx_rate_solve's number of pairs (2 + ceil(log2(t_hi - t_lo + 2))) of the
 * per-hop pick and a step kernel (the scan, thread 0's decision, all threads write the next target_t), then the pick
 * at A(q) and the freeze kernel (the through-scan, the pins, the next phase's first targets); last the pick at
 * target_t and a finishing kernel.  K (2 pairs + 2) + 3 launches, fixed by K and the range alone; the host waits for
 * none and uploads nothing.  The kernels of a finished solve, and the steps of a phase whose level is found, return
 * before they scan; the picks between them still run, at the targets that stand.  The state, the pins and an int64
 * per hop live in the handle beside the other solves': solves of one handle belong on one stream.
 *
 *   target_t, phase_of (out): int32 [n_cf / n_ch] in device memory
 *   pin_result (out):         device memory
 * PACX_E_ARG for a null target_t or phase_of with n_cf > 0, a null pin_result, pin_step_t < 1 or max_phases outside
 * [1, PACX_PIN_PHASES_MAX]; every other rule, and PACX_E_UNSUPPORTED, as pacx_band_solve_bucket / pacx_rate_solve_bucket.
 */
#define PACX_PIN_PHASES_MAX 16

typedef struct pacx_pin_result {
    int32_t phases;               /* bisections run */
    int32_t open;                 /* 1: the last phase allowed still pinned a hop */
} pacx_pin_result;

int pacx_band_solve_bucket_pinned(pacx_handle *h, int64_t n_cf, int32_t n_ch, const double *nmr, const int32_t *cap,
                                  const int32_t *cap_alloc, int64_t limit_bytes, const pacx_bucket *b, double nmr_lo_db,
                                  double nmr_hi_db, int32_t pin_step_t, int32_t max_phases, int32_t *bit_alloc,
                                  int32_t *n_bytes, uint8_t *capped, int32_t *target_t, int32_t *phase_of,
                                  pacx_rate_result *result, pacx_bucket_result *bucket_result,
                                  pacx_pin_result *pin_result, void *stream);
int pacx_rate_solve_bucket_pinned(pacx_handle *h, int64_t n_cf, int32_t n_ch, int32_t row, int32_t sub_stride,
                                  const double *worst, const int32_t *bits, const int32_t *steps, int64_t limit_bytes,
                                  const pacx_bucket *b, double nmr_lo_db, double nmr_hi_db, int32_t pin_step_t,
                                  int32_t max_phases, int32_t *budget, int32_t *n_bytes, uint8_t *capped,
                                  int32_t *target_t, int32_t *phase_of, pacx_rate_result *result,
                                  pacx_bucket_result *bucket_result, pacx_pin_result *pin_result, void *stream);

#endif /* PACX_BUCKET_PIN_H */
