/* g2048_stagemean.h -- C ABI of batch-mean TD learning for the multi-stage n-tuple value network
 * (libg2048_stagemean.so).
 *
 * g2048_ntstage_td_step adds, into every staged entry, the SUM of the deltas that the boards of a
 * lock-step batch send it, so its rate is sized for the hot early-game entries (n * lr = 1/4) and
 * the late stages' tables, which a handful of boards touch per step, barely move.  The batch-mean
 * rule of g2048_ntmean.h moves every touched entry by the MEAN of the deltas that hit it in this
 * step, at a rate that does not depend on the batch; it takes a single table only.  This library
 * is that rule on the staged table of g2048_ntstage.h, weight promotion included, on gfx950
 * (csrc/g2048_stagemean.hip).  It is a library of its own: every other header and library keeps
 * its ABI, and this library does not link against another library of the project -- it takes the
 * same spec, the same stage spec and the same table.  Boards, moves, legal masks and status codes
 * are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h (idx(b, g, t), q[a], after(b, a), legal(b), F = 10) and of
 * g2048_ntstage.h (S, stage(b), UNSET, val(s, t, i), V(b)).
 *
 * State  lut   int32 lut[S][T][16^m] with UNSET = INT32_MIN, as in g2048_ntstage.h.
 *        acc   int64 acc[S][T][16^m][2], 16-byte aligned: acc[s][t][i] = (D, C) of the staged
 *              entry lut[s][t][i].  acc is all zero before a call and all zero after it: a
 *              workspace of the table's shape with no memory across steps.  The caller zeroes it
 *              once.  16 bytes per staged entry: 2 GiB for the 4 x 6 set with two stages, at most
 *              16 GiB (S = 8, T = 8, m = 6).
 *
 * One step.  policy, target, err, delta, the prev / has_prev commit and the domain are exactly
 * g2048_ntstage_td_step's: every afterstate is valued at its own stage, V(prev) is taken under
 * stage(prev), lookups fall through, and every read sees the table as it was before the call.
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)               arithmetic shift (floor)
 *   promote  exactly as the staged TD step: for every board with has_prev (whatever its delta),
 *            with s = stage(prev), every lut[s][t][idx(prev, g, t)] that is UNSET becomes
 *            val(s, t, idx) of the pre-call table
 *   hit      every pair (g, t) of every board with has_prev and delta != 0 hits the staged entry
 *            (s, t, idx(prev, g, t)); pairs that coincide on a symmetric board are each a hit
 *   move     for every staged entry hit at least once:
 *              D = the sum of delta over its hits        int64; |D| <= 8 n * 2^31
 *              C = the number of its hits                1 <= C <= 8 n
 *              lut[s][t][i] = (its value after promotion) + floor(D / C)
 *                                                        mathematical floor, like the shifts;
 *                                                        |floor(D / C)| <= 2^31, modulo 2^32
 *   commit   prev = after(b, action) and has_prev = 1 if legal(b) != 0; else has_prev = 0 and
 *            prev is left as it is.
 *
 * Consequences.  S = 1 on a table without UNSET is g2048_ntmean_step exactly.  A batch in which
 * no two hits share a staged entry is g2048_ntstage_td_step exactly.  A batch with every board
 * repeated k times leaves the table that the unrepeated batch leaves.  lr_num = 0 promotes, moves
 * nothing and leaves acc zero.  Two boards at different stages that address the same (t, i)
 * accumulate separately: each stage's entry has its own (D, C) and starts from the pre-call val,
 * as in g2048_ntstage.h -- that a hot index is split by stage is the point of the combination.
 * floor(-3 / 2) = -2.
 *
 * Domain: that of g2048_ntstage_td_step (exponents <= 27, 0 <= lr_num <= 2^16, 0 <= lr_shift <=
 * 31, no table entry and no delta leaves int32, no entry is brought to exactly INT32_MIN), and
 * acc all zero on entry.
 */
#ifndef G2048_STAGEMEAN_H
#define G2048_STAGEMEAN_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"
#include "g2048_ntstage.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace acc for a spec and a stage spec (16 S T 16^m), or G2048_EINVAL for a bad
 * spec or a bad stage spec. */
G2048_API int64_t g2048_stagemean_acc_bytes(const g2048_ntuple_spec* spec,
                                            const g2048_ntstage_spec* stages);

/* One batch-mean step on the staged table (see above).  lut_dev int32[S][T][16^m] is read and
 * updated; acc_dev int64[S][T][16^m][2] (16-byte aligned) is all zero on entry and all zero again
 * when the call's work has run; boards_dev u8[n][16] (16-byte aligned); prev_dev u8[n][16]
 * (16-byte aligned) and has_prev_dev u8[n] are read and updated; action_out_dev u8[n] and
 * delta_out_dev i32[n] are required, err_out_dev i64[n] may be NULL.  1 <= n <= G2048_MAX_BOARDS,
 * `stream` a hipStream_t (NULL = default).  Stream-ordered and asynchronous: no allocation and no
 * host sync, so a call may be captured into a hipGraph.  Bad arguments (those of
 * g2048_ntstage_td_step, and acc_dev NULL or misaligned) return G2048_EINVAL before any device
 * work.
 *
 * Three launches on the stream, because the quotient of an entry needs every hit of the step and
 * nothing orders a read in one workgroup against an add in another.  The first reads the table,
 * writes action, err and delta, and stores the promoted values: the only table words it writes
 * are UNSET entries, each with the value it resolves to, so a concurrent read resolves to the
 * same number whether it sees the entry before or after.  The second only adds (delta, 1) into
 * acc (64-bit integer atomics).  The third takes (D, C) of every hit entry out of acc with atomic
 * exchanges, which leave zeros behind -- exactly one lane in the grid gets an entry's non-zero C
 * back -- adds floor(D / C) into lut (32-bit integer atomics into entries the first launch has
 * promoted, so never into UNSET) and commits prev / has_prev, recomputing after(board, action)
 * from boards_dev and action_out_dev.  Adds commute and every winner of an exchange computes the
 * same quotient, so the result does not depend on any order.  delta_out_dev is the hand-over
 * between the launches; acc is the only workspace. */
G2048_API int g2048_stagemean_step(const g2048_ntuple_spec* spec,
                                   const g2048_ntstage_spec* stages, int32_t* lut_dev,
                                   int64_t* acc_dev, const uint8_t* boards_dev, int64_t n,
                                   uint8_t* prev_dev, uint8_t* has_prev_dev, int32_t lr_num,
                                   int32_t lr_shift, uint8_t* action_out_dev,
                                   int32_t* delta_out_dev, int64_t* err_out_dev, int device_id,
                                   void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_stagemean_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_STAGEMEAN_H */
