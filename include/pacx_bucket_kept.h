/*
 * pacx_bucket_kept.h -- the buffered solve of pacx_bucket.h for a stream that arrives in chunks, on curves kept as
 * thresholds.  Included by pacx.h right behind pacx_bucket_pin.h, inside its extern "C" block; not for inclusion on its
 * own.  Additive exports of ABI 7.  Notation is pacx_bucket.h's: hops of n_ch channel-frames, x_h, L_h, F_h, the bucket
 * b, size_q16 = size_bytes << 16; a kept curve and its range [t_lo, t_hi] = 64 [nmr_lo_db, nmr_hi_db] are those of
 * pacx_band_thresholds / pacx_rate_thresholds (pacx.h).
 */
#ifndef PACX_BUCKET_KEPT_H
#define PACX_BUCKET_KEPT_H
#ifndef PACX_BUCKET_PIN_H
#error "include pacx.h, which includes pacx_bucket.h, pacx_bucket_pin.h and then this header"
#endif

/*
 * fits(t) of pacx_*_solve_bucket needs peak_q16(t), which is neither a sum over chunks nor monotone in t: the
 * bisection's path has to be walked probe by probe, and with the stream in chunks every probe is a pass over all of
 * them.  Two facts make that cheap.  The scan of a stream in pieces is exact (end_q16), so a chunk's scan at a target
 * carries on from the chunk before it, target by target.  And the next L decisions of the bisection depend only on
 * fits at the 2^L - 1 targets the bisection could visit in them, the nodes of a tree of depth L: one pass that
 * evaluates all of them takes L decisions.  The path is the plain solve's, decision for decision.
 *
 * A pass over a stream's chunks, in stream order:
 *   per chunk   pacx_*_bytes_thresholds: the chunk's n_bytes at every target of the pass, its thresholds read once
 *               pacx_bucket_scan_targets: every target's scan carried over the chunk
 *   at the end  pacx_bucket_tree_step: up to L decisions, the next pass's targets
 * after pacx_bucket_tree_begin once.  ceil((P - 1) / L) passes with P = 2 + ceil(log2(t_hi - t_lo + 2)), the pairs of
 * pacx_*_solve_bucket: 13, 7, 5, 4, 3 passes for L = 1 ... 5 on 60 dB.  Fixed by the range alone; the host waits for
 * nothing between the calls and the handle holds no state of the solve: it lives in the caller's device memory.
 */
#define PACX_BUCKET_TREE_LEVELS_MAX 5
#define PACX_BUCKET_TREE_TARGETS 31           /* 2^PACX_BUCKET_TREE_LEVELS_MAX - 1: target_t and acc of a solve */
#define PACX_BUCKET_TREE_STATE_BYTES 128      /* the state block of a solve, 8-byte aligned device memory */

/*
 * The bytes of a pick at several targets.  n_bytes_t[m][cf], int32 [n_targets][n_cf] in device memory, is the n_bytes
 * that pacx_band_pick_thresholds / pacx_rate_pick_thresholds write for channel-frame cf at the grid target target_t[m]
 * (int32 [n_targets] in DEVICE memory, grid units, clamped into [t_lo, t_hi]); no allocation and no `capped` are
 * written.  1 <= n_targets <= PACX_BUCKET_TREE_TARGETS.  Every other argument, its rules and PACX_E_UNSUPPORTED as
 * the pick's; n_cf = 0 returns at once.  One launch on `stream`.
 */
int pacx_band_bytes_thresholds(pacx_handle *h, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                               const uint8_t *cap_alloc, double nmr_lo_db, double nmr_hi_db, int32_t n_targets,
                               const int32_t *target_t, int32_t *n_bytes_t, void *stream);
int pacx_rate_bytes_thresholds(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const uint16_t *e,
                               const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db,
                               int32_t n_targets, const int32_t *target_t, int32_t *n_bytes_t, void *stream);

/*
 * pacx_bucket_scan of one piece of a stream at n_targets targets, folded into what came before.  Row m of n_bytes_t
 * (int32, row_stride entries apart, row_stride >= n_hops n_ch) holds the piece's n_bytes at target m; acc (device
 * memory, in and out, [n_targets]) the scan of the stream so far.  For every m, with piece = pacx_bucket_scan of the
 * row from start_q16 = acc[m].end_q16 under (drain_q16, size_bytes):
 *
 *   total      += piece.total
 *   peak_q16, peak_hop: the piece's and piece.peak_hop + hop_off if a hop of the piece rose above acc[m].peak_q16,
 *                       else as they were (of equal peaks the earlier hop stands)
 *   first_over  = the first there is: as it was if >= 0, else piece.first_over + hop_off if that is >= 0
 *   end_q16     = piece.end_q16
 *
 * hop_off: the hops of the stream before the piece.  Started from the scan of no hop, {0, start_q16, -1, -1,
 * start_q16}, acc[m] after the pieces of a stream in order is pacx_bucket_scan of the whole row, field for field.
 * n_hops = 0 is valid and leaves acc as it is.  Domain: pacx_bucket_scan's for n_hops, n_ch, drain_q16 and
 * size_bytes; hop_off >= 0, hop_off + n_hops <= 2^30; 1 <= n_targets <= PACX_BUCKET_TREE_TARGETS: anything else,
 * and a null acc or a null n_bytes_t with n_hops > 0, is PACX_E_ARG.  Defined on arrays alone; answers any handle.
 * One launch of n_targets workgroups of 1024 threads.
 */
int pacx_bucket_scan_targets(pacx_handle *h, int64_t n_hops, int32_t n_ch, int32_t n_targets, const int32_t *n_bytes_t,
                             int64_t row_stride, int64_t drain_q16, int64_t size_bytes, int64_t hop_off,
                             pacx_bucket_result *acc, void *stream);

/*
 * The tree.  state: PACX_BUCKET_TREE_STATE_BYTES of device memory; target_t: int32 [PACX_BUCKET_TREE_TARGETS]; acc:
 * pacx_bucket_result [PACX_BUCKET_TREE_TARGETS]; all three the caller's, in device memory, given to every call of
 * one solve.  levels = L in [1, PACX_BUCKET_TREE_LEVELS_MAX]; a pass has n = 2^L - 1 targets.
 *
 * A pass's targets are the nodes of the depth-L tree of the solve's decision from the current state, in heap order:
 * slot 0 is the state's next probe; slots 2k + 1 and 2k + 2 are the next probe after the decision at slot k with
 * fits = 0 and fits = 1.  A slot below a decision that ends the solve repeats the target found and is never read.
 *
 * pacx_bucket_tree_begin: the state of pacx_*_solve_bucket before its first probe (lo = t_lo - 1, hi = t_hi, the
 * probe of t_hi next), the first pass's targets, every acc the scan of no hop from b->start_q16.
 *
 * pacx_bucket_tree_step: from slot k = 0, at most L times and until the solve has ended:
 *   fits := acc[k].total <= limit_bytes && acc[k].peak_q16 <= size_q16; the decision of pacx_*_solve_bucket on it;
 *   the probe's acc is kept if it fits (hi moved there) and, fit or not, in the first decision (the probe of t_hi);
 *   k = 2k + 1 + fits.
 * Then the next pass's targets, every acc the scan of no hop again, and the results: result = {the state's probe,
 * met, the kept acc's total}, bucket_result = the kept acc.  Both are the buffered solve's once the solve has ended,
 * which it has after ceil((P - 1) / L) steps; a step on an ended solve changes nothing.
 *
 * PACX_E_ARG: levels outside its range, a null pointer, limit_bytes < 0, a range or a bucket outside the rules of
 * pacx_*_solve_bucket; before any launch.  Defined on the caller's memory alone; answers any handle.  One launch of
 * one thread each.
 */
int pacx_bucket_tree_begin(pacx_handle *h, const pacx_bucket *b, double nmr_lo_db, double nmr_hi_db, int32_t levels,
                           void *state, int32_t *target_t, pacx_bucket_result *acc, void *stream);
int pacx_bucket_tree_step(pacx_handle *h, int64_t limit_bytes, const pacx_bucket *b, int32_t levels, void *state,
                          int32_t *target_t, pacx_bucket_result *acc, pacx_rate_result *result,
                          pacx_bucket_result *bucket_result, void *stream);

#endif /* PACX_BUCKET_KEPT_H */
