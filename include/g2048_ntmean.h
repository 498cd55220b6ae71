/* g2048_ntmean.h -- C ABI of batch-mean TD learning for the n-tuple value network
 * (libg2048_ntmean.so).
 *
 * g2048_ntuple_td_step adds, into every table entry, the SUM of the deltas that the boards of a
 * lock-step batch send it.  An early-game entry receives up to n of them in one step, so the rate
 * of one delta has to shrink with the batch (default_lr_shift keeps n * lr = 1/4), and an entry
 * that a single board touches -- a late-game position -- then moves n times more slowly than the
 * rule needs for stability.  The batch-mean rule moves every touched entry by the MEAN of the
 * deltas that hit it in this step: a hot entry moves by the batch's mean error, a rare entry by its
 * own.  Stability then depends on the number of entries that make up a value (8 T), not on n.
 * This library is that rule for the network of g2048_ntuple.h on gfx950 (csrc/g2048_ntmean.hip).
 * It is a library of its own: every other header and library keeps its ABI, and this library does
 * not link against another library of the project -- it takes the same spec and the same table.
 * Boards, moves, legal masks and status codes are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h: idx(b, g, t), V(b), q[a], after(b, a), legal(b), F = 10.
 *
 * State  lut   int32 lut[T][16^m], as in g2048_ntuple.h.
 *        acc   int64 acc[T][16^m][2], 16-byte aligned: acc[t][i] = (D, C) of the entry lut[t][i].
 *              acc is all zero before a call and all zero after it: a workspace of the table's
 *              shape with no memory across steps.  The caller zeroes it once.
 *
 * One step.  policy, target, err, delta, the prev / has_prev commit and the domain are exactly
 * g2048_ntuple_td_step's:
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)               arithmetic shift (floor)
 * All reads of lut see it as it was before the call.  For every board with has_prev and
 * delta != 0, each of its 8 T pairs (g, t) hits the entry i = idx(prev, g, t) of tuple t (pairs
 * that coincide on a symmetric board are each a hit, as in TD(0)).  For every entry hit at least
 * once:
 *   D = the sum of delta over its hits        int64; |D| <= 8 n * 2^31
 *   C = the number of its hits                1 <= C <= 8 n
 *   lut[t][i] += floor(D / C)                 mathematical floor, like the shifts;
 *                                             |floor(D / C)| <= 2^31, added modulo 2^32
 * then prev = after(b, action) and has_prev = 1 if legal(b) != 0; else has_prev = 0 and prev is
 * left as it is.
 *
 * Consequences.  A batch in which no two hits share an entry is the TD(0) step exactly.  A batch
 * with every board repeated k times leaves the table that the unrepeated batch leaves.  lr_num = 0
 * changes nothing but prev, has_prev and the outputs.  floor(-3 / 2) = -2.
 *
 * Domain: that of g2048_ntuple_td_step (exponents <= 27, 0 <= lr_num <= 2^16, 0 <= lr_shift <= 31,
 * no table entry and no delta leaves int32), and acc all zero on entry.
 */
#ifndef G2048_NTMEAN_H
#define G2048_NTMEAN_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace acc for a spec (16 T 16^m), or G2048_EINVAL for a bad spec. */
G2048_API int64_t g2048_ntmean_acc_bytes(const g2048_ntuple_spec* spec);

/* One batch-mean step (see above).  lut_dev int32[T][16^m] is read and updated; acc_dev
 * int64[T][16^m][2] (16-byte aligned) is all zero on entry and all zero again when the call's work
 * has run; boards_dev u8[n][16] (16-byte aligned); prev_dev u8[n][16] (16-byte aligned) and
 * has_prev_dev u8[n] are read and updated; action_out_dev u8[n] and delta_out_dev i32[n] are
 * required, err_out_dev i64[n] may be NULL.  1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t
 * (NULL = default).  Stream-ordered and asynchronous: no allocation and no host sync, so a call
 * may be captured into a hipGraph.  Bad arguments return G2048_EINVAL before any device work.
 *
 * Three launches on the stream, because the quotient of an entry needs every hit of the step and
 * nothing orders a read in one workgroup against an add in another.  The first only reads lut: it
 * writes action, err and delta.  The second only adds (delta, 1) into acc (64-bit integer
 * atomics).  The third takes (D, C) of every hit entry out of acc with atomic exchanges, which
 * leave zeros behind -- exactly one lane in the grid gets an entry's non-zero C back -- adds
 * floor(D / C) into lut (32-bit integer atomics) and commits prev / has_prev, recomputing
 * after(board, action) from boards_dev and action_out_dev.  Adds commute and every winner of an
 * exchange computes the same quotient, so the result does not depend on any order.
 * delta_out_dev is the hand-over between the launches; there is no other workspace. */
G2048_API int g2048_ntmean_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, int64_t* acc_dev,
                                const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                                uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                                uint8_t* action_out_dev, int32_t* delta_out_dev,
                                int64_t* err_out_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntmean_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTMEAN_H */
