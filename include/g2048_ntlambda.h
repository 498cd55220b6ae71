/* g2048_ntlambda.h -- C ABI of truncated TD(lambda) learning for the n-tuple value network
 * (libg2048_ntlambda.so).
 *
 * g2048_ntuple_td_step moves, with the error observed at step t, only the afterstate of step
 * t - 1.  TD(lambda) with eligibility traces truncated to the last H afterstates (for 2048:
 * Jaskowski, "Mastering 2048 with delayed temporal coherence learning, multi-stage weight
 * promotion, redundant encoding and carousel shaping", 2017, lambda = 0.5 and a horizon of 3) also
 * moves the afterstates of steps t - 2, t - 3, ... with weights lambda, lambda^2, ...  This
 * library is that rule with lambda = 2^-s for the network of g2048_ntuple.h on gfx950
 * (csrc/g2048_ntlambda.hip).  It is a library of its own: g2048.h, g2048_search.h,
 * g2048_ntuple.h, g2048_ntsearch.h, g2048_nttc.h and their libraries keep their ABI, and this
 * library does not link against libg2048_ntuple.so -- it takes the same spec and the same table.
 * Boards, moves, legal masks and status codes are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h: idx(b, g, t), V(b), q[a], after(b, a), legal(b), F = 10.
 *
 * Parameters
 *   horizon   H, 1 <= H <= G2048_NTLAMBDA_MAX_HORIZON (8): the afterstates a board remembers
 *   lam_shift s, 1 <= s <= 31 with (H - 1) s <= 31: lambda = 2^-s
 *
 * State  lut    int32 lut[T][16^m], as in g2048_ntuple.h.
 *        hist   u8 hist[H][n][16], 16-byte aligned: H planes of n boards, a ring per board.
 *        head   u8 head[n]: the plane that holds board i's latest afterstate.
 *        depth  u8 depth[n]: how many afterstates of board i's running episode the ring holds.
 *        All zeros is the fresh state.  The afterstate k steps back of board i, for
 *        k < depth[i], is plane (head[i] - k) mod H, row i.
 *
 * One step.  All reads of lut and of the state see them as they were before the call.  With
 * prev = the afterstate 0 steps back and has_prev = depth > 0, target, err and delta are
 * exactly g2048_ntuple_td_step's:
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)               arithmetic shift (floor)
 * For k = 0 .. depth - 1, with hist_k the afterstate k steps back:
 *   delta_k = sgn(delta) * (|delta| >> (k s))      the magnitude taken in 64 bits, so it rounds
 *                                                  toward zero (|INT32_MIN| = 2^31) and
 *                                                  delta_0 = delta
 *   if delta_k != 0:  lut[t][idx(hist_k, g, t)] += delta_k  for all 8 T pairs (g, t), modulo 2^32
 * Pairs that coincide are each applied, within one afterstate and across afterstates.
 * Then, if legal(b) != 0:  head = (head + 1) mod H, plane head row i = after(b, action),
 *                          depth = min(depth + 1, H);
 * otherwise:               depth = 0, and head and the planes are left as they are.
 *
 * With H = 1 this is g2048_ntuple_td_step exactly: plane 0 is prev, depth is has_prev, head
 * stays 0 and lam_shift has no effect.
 *
 * Domain: that of g2048_ntuple_td_step (exponents <= 27, 0 <= lr_num <= 2^16, 0 <= lr_shift <= 31,
 * no table entry and no delta leaves int32), head[i] < H and depth[i] <= H.  An entry that all of
 * a board's H afterstates share receives at most 8 T * 2 |delta| from that board in one step
 * (the weights sum to less than 2).
 */
#ifndef G2048_NTLAMBDA_H
#define G2048_NTLAMBDA_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTLAMBDA_MAX_HORIZON 8
#define G2048_NTLAMBDA_MAX_LAM_SHIFT 31

/* One TD(lambda) step (see above).  lut_dev int32[T][16^m] is read and updated; boards_dev
 * u8[n][16] (16-byte aligned); hist_dev u8[horizon][n][16] (16-byte aligned), head_dev u8[n] and
 * depth_dev u8[n] are read and updated; action_out_dev u8[n] and delta_out_dev i32[n] are
 * required, err_out_dev i64[n] may be NULL.  1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t
 * (NULL = default).  Stream-ordered and asynchronous: no allocation, no workspace and no host
 * sync, so a call may be captured into a hipGraph.  Bad arguments (a NULL pointer, a misaligned
 * one, a bad spec, horizon, lam_shift or (horizon - 1) lam_shift, a bad lr_num, lr_shift or n)
 * return G2048_EINVAL before any device work.
 *
 * Two launches on the stream.  The first only reads lut and the state: it writes action, err
 * and delta.  The second never reads lut: it adds delta_k into lut for the board's depth
 * afterstates (32-bit integer atomics, which commute, so the result does not depend on their
 * order) and commits head / plane / depth, recomputing after(board, action) from boards_dev and
 * action_out_dev.  delta_out_dev is the hand-over between the two. */
G2048_API int g2048_ntlambda_step(const g2048_ntuple_spec* spec, int32_t* lut_dev,
                                  const uint8_t* boards_dev, int64_t n, uint8_t* hist_dev,
                                  uint8_t* head_dev, uint8_t* depth_dev, int32_t horizon,
                                  int32_t lam_shift, int32_t lr_num, int32_t lr_shift,
                                  uint8_t* action_out_dev, int32_t* delta_out_dev,
                                  int64_t* err_out_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntlambda_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTLAMBDA_H */
