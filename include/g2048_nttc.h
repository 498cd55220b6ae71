/* g2048_nttc.h -- C ABI of temporal-coherence learning for the n-tuple value network
 * (libg2048_nttc.so).
 *
 * g2048_ntuple_td_step moves every table entry at one global, fixed rate.  Temporal-coherence
 * (TC) learning (Beal and Smith 1999; for 2048: Jaskowski, "Mastering 2048 with delayed temporal
 * coherence learning, multi-stage weight promotion, redundant encoding and carousel shaping",
 * 2017) gives each entry a rate of its own: an entry keeps the running sum E of the errors it saw
 * and the running sum A of their magnitudes and moves at |E| / A -- at full speed while its errors
 * agree in sign, slower once they start to cancel.  This library is that rule for the network of
 * g2048_ntuple.h on gfx950 (csrc/g2048_nttc.hip).  It is a library of its own: g2048.h,
 * g2048_search.h, g2048_ntuple.h, g2048_ntsearch.h and their libraries keep their ABI, and this
 * library does not link against libg2048_ntuple.so -- it takes the same spec and the same table.
 * Boards, moves, legal masks and status codes are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h: idx(b, g, t), V(b), q[a], after(b, a), legal(b), F = 10.
 *
 * State  lut   int32 lut[T][16^m], as in g2048_ntuple.h.
 *        ea    int64 ea[T][16^m][2], 16-byte aligned: ea[t][i][0] = E and ea[t][i][1] = A of the
 *              entry lut[t][i], interleaved so that one 16-byte load fetches both.  (int32 cannot
 *              hold A: a hot entry receives n deltas per step.)
 *
 * Rate   rate(E, A) = 2^16                                      if A == 0
 *                   = floor(((|E| >> s) << 16) / (A >> s))      otherwise,
 *                     s = max(0, bitlen(A) - 16), bitlen(A) = the number of bits of A
 *        a fixed-point fraction with 16 bits, 0 <= rate <= 2^16.  Both operands are shifted down
 *        to at most 16 bits, so with |E| <= A the division is a 32-bit unsigned one:
 *        (|E| >> s) << 16 <= (2^16 - 1) << 16 and 1 <= A >> s < 2^16.  rate(+-A, A) = 2^16.
 *
 * One TC step.  policy, target, err, delta, the prev / has_prev commit and the domain are
 * exactly g2048_ntuple_td_step's:
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)               arithmetic shift (floor)
 * All reads of lut and of ea see them as they were before the call.  For every board with
 * has_prev and delta != 0, each of its 8 T pairs (g, t) gives the entry i = idx(prev, g, t) of
 * tuple t (pairs that coincide are each applied, as in TD(0)), and that entry gets
 *   step       = (delta * rate(E, A)) >> 16      arithmetic shift (floor); fits int32: rate <= 2^16
 *   lut[t][i] += step                            modulo 2^32
 *   E         += delta                           int64
 *   A         += |delta|                         int64; |INT32_MIN| = 2^31
 * then prev = after(b, action) and has_prev = 1 if legal(b) != 0; else has_prev = 0 and prev is
 * left as it is.
 *
 * E and A accumulate delta, the error already scaled by lr_num / 2^lr_shift, not err itself.
 * The ratio |E| / A does not depend on that scale while the caller keeps lr_num and lr_shift
 * constant; a caller that changes them mid-run weights the later errors differently.  With a
 * fresh (all-zero) ea every rate is 2^16 and the first step equals g2048_ntuple_td_step's.
 *
 * Domain: that of g2048_ntuple_td_step (exponents <= 27, 0 <= lr_num <= 2^16, 0 <= lr_shift <= 31,
 * no table entry and no delta leaves int32) and 0 <= |E| <= A < 2^62 for every entry.  The updates
 * keep |E| <= A (the triangle inequality) if the caller starts from zeros, and it holds within a
 * call too because every read sees the state from before the call.  One step adds at most
 * n * 8 * 2^31 to an A.
 */
#ifndef G2048_NTTC_H
#define G2048_NTTC_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTTC_RATE_BITS 16
#define G2048_NTTC_MAX_A (((int64_t)1 << 62) - 1)

/* Host only: rate(E, A) above, in [0, 2^16].  Outside the domain (A < 0, A > G2048_NTTC_MAX_A or
 * |E| > A) it returns G2048_EINVAL. */
G2048_API int32_t g2048_nttc_rate(int64_t E, int64_t A);

/* Bytes of caller-owned device scratch that one g2048_nttc_step over n boards needs (the steps
 * of the 8 T pairs of every board: 32 T n), or G2048_EINVAL for a bad spec or n. */
G2048_API int64_t g2048_nttc_work_bytes(const g2048_ntuple_spec* spec, int64_t n);

/* One TC step (see above).  lut_dev int32[T][16^m] and ea_dev int64[T][16^m][2] (16-byte
 * aligned) are read and updated; boards_dev u8[n][16] (16-byte aligned); prev_dev u8[n][16]
 * (16-byte aligned) and has_prev_dev u8[n] are read and updated; action_out_dev u8[n] and
 * delta_out_dev i32[n] are required, err_out_dev i64[n] may be NULL; work_dev is
 * g2048_nttc_work_bytes(spec, n) bytes, 4-byte aligned.  1 <= n <= G2048_MAX_BOARDS, `stream` a
 * hipStream_t (NULL = default).  Stream-ordered and asynchronous: no allocation and no host sync,
 * so a call may be captured into a hipGraph.  Bad arguments return G2048_EINVAL before any device
 * work.
 *
 * Two launches on the stream.  The first only reads lut and ea: it writes action, err and delta
 * and, for every board that will add, the 8 T steps into work_dev.  The second only adds: step
 * into lut (32-bit integer atomics), delta and |delta| into ea (64-bit integer atomics) -- the
 * adds commute, so the result does not depend on their order -- and commits prev / has_prev,
 * recomputing after(board, action) from boards_dev and action_out_dev.  delta_out_dev and
 * work_dev are the hand-over between the two.  After the call only the documented outputs have
 * defined contents; work_dev does not. */
G2048_API int g2048_nttc_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, int64_t* ea_dev,
                              const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                              uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                              uint8_t* action_out_dev, int32_t* delta_out_dev,
                              int64_t* err_out_dev, void* work_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_nttc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTTC_H */
