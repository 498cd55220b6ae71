/* g2048_stagemeantc.h -- C ABI of temporal-coherence learning on the batch-mean rule for the
 * multi-stage n-tuple value network (libg2048_stagemeantc.so).
 *
 * g2048_stagemean_step moves every staged entry hit in a step by the mean floor(D / C) of its
 * hits, at one fixed rate.  The late stages see few boards per step and would gain most from a
 * rate per entry, and g2048_ntmeantc_step, which has one, takes a single table only.  This library
 * is the two together: the batch-mean rule on the staged table of g2048_ntstage.h, weight
 * promotion included, with every staged entry's one update per step scaled by rate(E, A) over
 * accumulators (E, A) of its own, on gfx950 (csrc/g2048_stagemeantc.hip).  It is a library of its
 * own: every other header and library keeps its ABI, and this library does not link against
 * another library of the project -- it takes the same spec, the same stage spec and the same
 * table.  Boards, moves, legal masks and status codes are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h (idx(b, g, t), q[a], after(b, a), legal(b), F = 10), of
 * g2048_ntstage.h (S, stage(b), UNSET, val(s, t, i), V(b)), of g2048_stagemean.h (D, C) and of
 * g2048_ntmeantc.h (m, E, A).
 *
 * State  lut   int32 lut[S][T][16^m] with UNSET = INT32_MIN, as in g2048_ntstage.h.
 *        acc   int64 acc[S][T][16^m][2], 16-byte aligned: acc[s][t][i] = (D, C) of the staged
 *              entry lut[s][t][i].  acc is all zero before a call and all zero after it: the
 *              workspace of g2048_stagemean.h, with no memory across steps.  The caller zeroes it
 *              once.
 *        ea    int64 ea[S][T][16^m][2], 16-byte aligned: ea[s][t][i] = (E, A) of the STAGED entry
 *              lut[s][t][i], interleaved so that one 16-byte load fetches both.  ea carries
 *              across steps; a fresh one is all zero.
 *        16 + 16 bytes per staged entry: 2 GiB + 2 GiB for the 4 x 6 set with two stages.
 *
 * Rate   rate(E, A) is g2048_nttc.h's, bit for bit:
 *          rate(E, A) = 2^16                                      if A == 0
 *                     = floor(((|E| >> s) << 16) / (A >> s))      otherwise,
 *                       s = max(0, bitlen(A) - 16), bitlen(A) = the number of bits of A
 *        a fixed-point fraction with 16 bits, 0 <= rate <= 2^16; with |E| <= A both shifted
 *        operands are below 2^16 and the division is a 32-bit unsigned one.
 *
 * One step.  policy, target, err, delta, promote, hit and commit are g2048_stagemean_step's, word
 * for word: every afterstate is valued at its own stage, V(prev) is taken under stage(prev),
 * lookups fall through, and every read of lut and of ea sees the state before the call.
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)               arithmetic shift (floor)
 *   promote  for every board with has_prev (whatever its delta), with s = stage(prev), every
 *            lut[s][t][idx(prev, g, t)] that is UNSET becomes val(s, t, idx) of the pre-call table
 *   hit      every pair (g, t) of every board with has_prev and delta != 0 hits the staged entry
 *            (s, t, idx(prev, g, t)), s = stage(prev); pairs that coincide on a symmetric board
 *            are each a hit
 *   move     for every staged entry hit at least once, with D the sum of delta over its hits
 *            (int64, |D| <= 8 n * 2^31) and C their number (1 <= C <= 8 n):
 *              m = floor(D / C)                          mathematical floor; |m| <= 2^31
 *              if m != 0:
 *                step         = (m * rate(E, A)) >> 16   arithmetic shift (floor); (E, A) =
 *                                                        ea[s][t][i] before the call
 *                lut[s][t][i] = (its value after promotion) + step          modulo 2^32
 *                E += m;  A += |m|                       int64
 *              if m == 0: the entry keeps its value after promotion and its ea is untouched
 *   commit   prev = after(b, action) and has_prev = 1 if legal(b) != 0; else has_prev = 0 and
 *            prev is left as it is.
 *
 * Promotion copies the weight only.  A promoted entry keeps its own (E, A): zeros if it never
 * moved, so it starts at the full rate.  This is Jaskowski's weight promotion -- a later stage
 * inherits what was learned, not how settled it was -- and there is no option for anything else.
 *
 * Consequences
 *   1. With ea all zero every rate is 2^16 and step = m: lut after the call is
 *      g2048_stagemean_step's, UNSET pattern included; every entry with m != 0 holds (m, |m|) and
 *      every other word of ea is still zero.
 *   2. S = 1 on a table without UNSET is g2048_ntmeantc_step from the same ea, lut and ea alike.
 *   3. With a zero ea, a batch whose staged hits are pairwise distinct (C = 1, m = delta) is
 *      g2048_ntstage_td_step.
 *   4. A batch with every board repeated k times leaves the lut and the ea that the batch given
 *      once leaves: (k D, k C) has the quotient of (D, C).
 *   5. lr_num = 0 promotes, moves nothing, leaves ea as it is and leaves acc zero.
 *   6. Two boards of different stages that address the same (t, i) keep separate (D, C) and
 *      separate (E, A): the same index can run at the full rate in one stage and slowly in
 *      another, which is the point of the combination.
 *   7. |E| <= A is preserved: |E + m| <= |E| + |m| <= A + |m|.  One call adds at most 2^31 to
 *      any A, whatever n is.
 *   8. acc is all zero after every call.
 *   9. The UNSET pattern after a call does not depend on ea.
 *   The two floors compose: floor(-3 / 2) = -2, and -2 at rate 2^15 is a step of -1.
 *
 * Domain: that of g2048_stagemean_step (exponents <= 27, 0 <= lr_num <= 2^16, 0 <= lr_shift <= 31,
 * no table entry and no delta leaves int32, no entry is brought to exactly INT32_MIN, acc all zero
 * on entry) and that of g2048_ntmeantc_step (0 <= |E| <= A < 2^62 for every staged entry).  The
 * updates keep |E| <= A if the caller starts from zeros, and A stays inside the domain for 2^31
 * calls (consequence 7).
 */
#ifndef G2048_STAGEMEANTC_H
#define G2048_STAGEMEANTC_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"
#include "g2048_ntstage.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_STAGEMEANTC_RATE_BITS 16
#define G2048_STAGEMEANTC_MAX_A (((int64_t)1 << 62) - 1)

/* Host only: rate(E, A) above, in [0, 2^16].  Outside the domain (A < 0, A >
 * G2048_STAGEMEANTC_MAX_A or |E| > A) it returns G2048_EINVAL. */
G2048_API int32_t g2048_stagemeantc_rate(int64_t E, int64_t A);

/* Bytes of the workspace acc for a spec and a stage spec (16 S T 16^m; ea has the same size), or
 * G2048_EINVAL for a bad spec or a bad stage spec. */
G2048_API int64_t g2048_stagemeantc_acc_bytes(const g2048_ntuple_spec* spec,
                                              const g2048_ntstage_spec* stages);

/* One step (see above): g2048_stagemean_step's arguments with ea_dev after acc_dev.  lut_dev
 * int32[S][T][16^m] is read and updated; acc_dev int64[S][T][16^m][2] (16-byte aligned) is all
 * zero on entry and all zero again when the call's work has run; ea_dev int64[S][T][16^m][2]
 * (16-byte aligned, sharing no byte with acc_dev) is read and updated; boards_dev u8[n][16]
 * (16-byte aligned); prev_dev u8[n][16] (16-byte aligned) and has_prev_dev u8[n] are read and
 * updated; action_out_dev u8[n] and delta_out_dev i32[n] are required, err_out_dev i64[n] may be
 * NULL.  1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t (NULL = default).  Stream-ordered and
 * asynchronous: no allocation and no host sync, so a call may be captured into a hipGraph.  Bad
 * arguments (those of g2048_stagemean_step; ea_dev NULL or misaligned; ea_dev overlapping acc_dev
 * anywhere within the 16 S T 16^m bytes of either) return G2048_EINVAL before any device work.
 *
 * Three launches on the stream, g2048_stagemean_step's.  The first reads the table, writes action,
 * err and delta, and stores the promoted values: the only table words it writes are UNSET entries,
 * each with the value it resolves to, so a concurrent read resolves to the same number whether it
 * sees the entry before or after.  The second only adds (delta, 1) into acc (64-bit integer
 * atomics).  The third takes (D, C) of every hit entry out of acc with atomic exchanges, which
 * leave zeros behind -- exactly one lane in the grid gets an entry's non-zero C back.  That lane
 * owns the staged entry: it forms m and, if m != 0, loads the entry's (E, A), adds step into lut
 * (a 32-bit integer atomic into an entry the first launch has promoted, so never into UNSET) and
 * stores (E + m, A + |m|).  No other lane of the call and no other launch touches that entry's ea,
 * so ea moves by plain 16-byte loads and stores and every read of it sees the state before the
 * call.  The launch then commits prev / has_prev, recomputing after(board, action) from boards_dev
 * and action_out_dev.  delta_out_dev is the hand-over between the launches; acc is the only
 * workspace. */
G2048_API int g2048_stagemeantc_step(const g2048_ntuple_spec* spec,
                                     const g2048_ntstage_spec* stages, int32_t* lut_dev,
                                     int64_t* acc_dev, int64_t* ea_dev, const uint8_t* boards_dev,
                                     int64_t n, uint8_t* prev_dev, uint8_t* has_prev_dev,
                                     int32_t lr_num, int32_t lr_shift, uint8_t* action_out_dev,
                                     int32_t* delta_out_dev, int64_t* err_out_dev, int device_id,
                                     void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_stagemeantc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_STAGEMEANTC_H */
