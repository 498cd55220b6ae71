/* g2048_ntmeantc.h -- C ABI of temporal-coherence learning on the batch-mean rule for the n-tuple
 * value network (libg2048_ntmeantc.so).
 *
 * g2048_nttc_step gives every table entry a rate of its own, |E| / A over the running sums of the
 * deltas it received and of their magnitudes.  In a lock-step batch a hot entry receives thousands
 * of deltas of both signs in ONE step, so its |E| / A collapses within the first steps.
 * g2048_ntmean_step moves every touched entry once per step, by the mean floor(D / C) of its hits,
 * but at one fixed rate.  This library is the two together: an entry hit in a step receives one
 * update, the mean m of its hits, scaled by rate(E, A); and E and A accumulate that one m, not the
 * C deltas behind it.  The accumulators then see one error per entry per step, the unbatched
 * regime temporal coherence was designed for.  It is the rule for the network of g2048_ntuple.h on
 * gfx950 (csrc/g2048_ntmeantc.hip).  It is a library of its own: every other header and library
 * keeps its ABI, and this library does not link against another library of the project -- it takes
 * the same spec and the same table.  Boards, moves, legal masks and status codes are those of
 * g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h: idx(b, g, t), V(b), q[a], after(b, a), legal(b), F = 10.
 *
 * State  lut   int32 lut[T][16^m], as in g2048_ntuple.h.
 *        acc   int64 acc[T][16^m][2], 16-byte aligned: acc[t][i] = (D, C) of the entry lut[t][i],
 *              as in g2048_ntmean.h.  acc is all zero before a call and all zero after it: a
 *              workspace of the table's shape with no memory across steps.  The caller zeroes it
 *              once.
 *        ea    int64 ea[T][16^m][2], 16-byte aligned: ea[t][i] = (E, A) of the entry lut[t][i],
 *              interleaved so that one 16-byte load fetches both, as in g2048_nttc.h.  ea carries
 *              across steps; a fresh one is all zero.
 *
 * Rate   rate(E, A) is g2048_nttc.h's, bit for bit:
 *          rate(E, A) = 2^16                                      if A == 0
 *                     = floor(((|E| >> s) << 16) / (A >> s))      otherwise,
 *                       s = max(0, bitlen(A) - 16), bitlen(A) = the number of bits of A
 *        a fixed-point fraction with 16 bits, 0 <= rate <= 2^16; with |E| <= A both shifted
 *        operands are below 2^16 and the division is a 32-bit unsigned one.
 *
 * One step.  policy, target, err, delta, the prev / has_prev commit and the domain are exactly
 * g2048_ntuple_td_step's:
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)               arithmetic shift (floor)
 * Hits, D and C are g2048_ntmean_step's: for every board with has_prev and delta != 0, each of its
 * 8 T pairs (g, t) hits the entry i = idx(prev, g, t) of tuple t (pairs that coincide on a
 * symmetric board are each a hit); D is the sum of delta over an entry's hits (int64,
 * |D| <= 8 n * 2^31) and C their number (1 <= C <= 8 n).  All reads of lut and of ea see them as
 * they were before the call.  For every entry hit at least once:
 *   m          = floor(D / C)                    mathematical floor; |m| <= 2^31
 *   step       = (m * rate(E, A)) >> 16          arithmetic shift (floor); |step| <= 2^31
 *   lut[t][i] += step                            modulo 2^32
 *   E         += m                               int64
 *   A         += |m|                             int64
 * An entry with m == 0 is left as it is, ea included.  Then prev = after(b, action) and
 * has_prev = 1 if legal(b) != 0; else has_prev = 0 and prev is left as it is.
 *
 * Consequences
 *   1. With ea all zero every rate is 2^16 and step = m: lut after the call is
 *      g2048_ntmean_step's, and every moved entry holds (E, A) = (m, |m|).
 *   2. A batch in which no two hits share an entry has C = 1 and m = delta everywhere: it is
 *      g2048_nttc_step from the same ea, lut and ea alike.
 *   3. A batch with every board repeated k times leaves the lut and the ea that the batch given
 *      once leaves: (k D, k C) has the quotient of (D, C).
 *   4. lr_num = 0 changes neither lut nor ea (only prev, has_prev and the outputs).
 *   5. |E| <= A is preserved: |E + m| <= |E| + |m| <= A + |m|.
 *   6. One call adds at most 2^31 to any A, whatever n is.
 *   7. acc is all zero after every call.
 *   The two floors compose: floor(-3 / 2) = -2, and -2 at rate 2^15 is a step of -1.
 *
 * Domain: that of g2048_ntuple_td_step (exponents <= 27, 0 <= lr_num <= 2^16, 0 <= lr_shift <= 31,
 * no table entry and no delta leaves int32), acc all zero on entry, and 0 <= |E| <= A < 2^62 for
 * every entry.  The updates keep |E| <= A if the caller starts from zeros (consequence 5).  One
 * step adds at most 2^31 to an A -- one |m| per entry per call, not g2048_nttc_step's
 * n * 8 * 2^31 -- so A stays inside the domain for 2^31 calls.
 */
#ifndef G2048_NTMEANTC_H
#define G2048_NTMEANTC_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTMEANTC_RATE_BITS 16
#define G2048_NTMEANTC_MAX_A (((int64_t)1 << 62) - 1)

/* Host only: rate(E, A) above, in [0, 2^16].  Outside the domain (A < 0, A > G2048_NTMEANTC_MAX_A
 * or |E| > A) it returns G2048_EINVAL. */
G2048_API int32_t g2048_ntmeantc_rate(int64_t E, int64_t A);

/* Bytes of the workspace acc for a spec (16 T 16^m; ea has the same size), or G2048_EINVAL for a
 * bad spec. */
G2048_API int64_t g2048_ntmeantc_acc_bytes(const g2048_ntuple_spec* spec);

/* One step (see above).  lut_dev int32[T][16^m] is read and updated; acc_dev int64[T][16^m][2]
 * (16-byte aligned) is all zero on entry and all zero again when the call's work has run; ea_dev
 * int64[T][16^m][2] (16-byte aligned, not acc_dev) is read and updated; boards_dev u8[n][16]
 * (16-byte aligned); prev_dev u8[n][16] (16-byte aligned) and has_prev_dev u8[n] are read and
 * updated; action_out_dev u8[n] and delta_out_dev i32[n] are required, err_out_dev i64[n] may be
 * NULL.  1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t (NULL = default).  Stream-ordered and
 * asynchronous: no allocation and no host sync, so a call may be captured into a hipGraph.  Bad
 * arguments return G2048_EINVAL before any device work.
 *
 * Three launches on the stream, g2048_ntmean_step's.  The first only reads lut: it writes action,
 * err and delta.  The second only adds (delta, 1) into acc (64-bit integer atomics).  The third
 * takes (D, C) of every hit entry out of acc with atomic exchanges, which leave zeros behind --
 * exactly one lane in the grid gets an entry's non-zero C back.  That lane owns the entry: it
 * forms m, loads the entry's (E, A), adds step into lut (a 32-bit integer atomic) and stores
 * (E + m, A + |m|).  No other lane of the call and no other launch touches that entry's ea, so ea
 * moves by plain 16-byte loads and stores and every read of it sees the state before the call.
 * The launch then commits prev / has_prev, recomputing after(board, action) from boards_dev and
 * action_out_dev.  delta_out_dev is the hand-over between the launches; there is no other
 * workspace. */
G2048_API int g2048_ntmeantc_step(const g2048_ntuple_spec* spec, int32_t* lut_dev,
                                  int64_t* acc_dev, int64_t* ea_dev, const uint8_t* boards_dev,
                                  int64_t n, uint8_t* prev_dev, uint8_t* has_prev_dev,
                                  int32_t lr_num, int32_t lr_shift, uint8_t* action_out_dev,
                                  int32_t* delta_out_dev, int64_t* err_out_dev, int device_id,
                                  void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntmeantc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTMEANTC_H */
