/* g2048_ntplay.h -- C ABI of the on-device n-tuple player (libg2048_ntplay.so): K moves of the
 * n-tuple policy, greedy or expectimax, played on an env's own buffers inside one launch.
 *
 * The other libraries of the family choose a move (g2048_ntuple_act, g2048_ntstage_act,
 * g2048_ntsearch_expectimax, g2048_stagesearch_expectimax) and leave the step to g2048_env_step,
 * so a game costs two launches and a host round trip per move.  This library plays the moves
 * itself: the boards stay in registers, the table is only read (csrc/g2048_ntplay.hip).  It is a
 * library of its own: the other headers and their libraries keep their ABI, and this one links
 * against none of them -- it reads the same spec, the same stage spec, the same table and the
 * buffers a g2048_env wraps.
 *
 * The rule, in integers throughout
 * --------------------------------
 * A call with k_steps = K and depth = d leaves board, meta (both rows), ep and clock byte for
 * byte as K iterations of
 *
 *     act = policy_d(board)            depth 1: g2048_ntuple_act / g2048_ntstage_act
 *                                      depth 2..3: g2048_ntsearch_expectimax /
 *                                                  g2048_stagesearch_expectimax
 *     g2048_env_step(actions = act)    the action-given step of include/g2048.h
 *
 * leave them, for both values of G2048_NO_AUTORESET and of G2048_P4_10 in env_flags.  Under
 * G2048_P4_10 the chance weights of the search follow the flag: (W, w4) = (10, 1), else (2, 1).
 * G2048_EGREEDY_FIXED is accepted and has no meaning here (no move is drawn).
 *
 * The action-given step of board i (global id gid = board_offset + i) at clock t, restated:
 *   u     = Philox4x32-10 block of (seed, subsequence gid, domain 0 (step draws), counter t):
 *           counter words {t_lo, t_hi, gid_lo, gid_hi | domain << 30}, key {seed_lo, seed_hi}
 *           with seed_lo = (uint32)seed, seed_hi = (uint32)(seed >> 32); one block per step.
 *           t = clock[i / 64] on entry + the number of moves already made in this call.
 *   legal = legal(board); done = (legal == 0)
 *   if !done and act is legal: score += gain(board, act); board = after(board, act); then one
 *           spawn: the k-th empty cell in row-major order, k = floor(u.z * n_empty / 2^32), a 4
 *           iff u.w < p4_thresh, p4_thresh = round(p(4) * 2^32) = 2147483648 or 429496730.
 *   if done: moves = (uint32)(t + 1) - start; ep[i] = {ep[i].episodes + 1, score, moves, the
 *           board's largest exponent}; and without G2048_NO_AUTORESET the board is re-dealt from
 *           the same block (cells u.z >> 28 and the floor(((u.z << 4) mod 2^32) * 15 / 2^32)-th
 *           of the 15 others; a 4 iff u.w < p4_thresh resp. (u.x << 2) mod 2^32 < p4_thresh),
 *           score = 0 and start = (uint32)(t + 1).
 *   meta row 0 is the score, row 1 the start; after the K steps clock[g] is K larger.
 * Under G2048_NO_AUTORESET a terminal board stays as it is and ends its episode again at every
 * later step: ep.episodes and the recomputed moves keep growing, exactly as the env's do.  R more
 * steps of a terminal board are therefore ep.episodes += R, moves = (uint32)(t + R) - start, the
 * other fields unchanged (the closed form; the library may take it when a whole wave is terminal).
 *
 * The latch.  fin u8[n] and result u32[n][4] are optional, together.  At the first terminal step
 * of board i at which fin[i] == 0, result[i] receives the four words that step writes to ep[i]
 * (episodes, score, moves, largest exponent) and fin[i] becomes 1.  A row with fin[i] != 0 on entry
 * is never written.  The table is never written; the replay ring, the episode log and the q-sum
 * of an env are not served: the caller must not use this library on an env with a log attached.
 *
 * Domain: the boards and the table of g2048_ntsearch.h / g2048_stagesearch.h (root exponents
 * <= 24 while depth > 1); every value of the search is an exact int64, as there.
 */
#ifndef G2048_NTPLAY_H
#define G2048_NTPLAY_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntstage.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTPLAY_MAX_DEPTH 3
#define G2048_NTPLAY_MAX_STEPS (1 << 20)

/* K = k_steps moves of the depth-`depth` policy of the table lut_dev int32[T][16^m] of `spec` on
 * the buffers of an env of n boards: board_dev u8[n][16] (16-byte aligned), meta_dev u32[2][n]
 * (4-byte aligned; row 0 score, row 1 start), ep_dev u32[n][4] (16-byte aligned), clock_dev
 * u64[ceil(n / 64)] (8-byte aligned); seed, board_offset and env_flags as given to
 * g2048_env_wrap.  fin_dev u8[n] and result_dev u32[n][4] (16-byte aligned) are both NULL or both
 * given.  1 <= n <= G2048_MAX_BOARDS, 1 <= k_steps <= G2048_NTPLAY_MAX_STEPS, 1 <= depth <=
 * G2048_NTPLAY_MAX_DEPTH.  Two launches (the moves, then the clocks), stream-ordered and
 * asynchronous: no allocation, no host sync, no atomics, so the call may be captured into a
 * hipGraph.  `stream` is a hipStream_t (NULL = default).  Bad arguments return G2048_EINVAL
 * before any device work. */
G2048_API int g2048_ntplay_steps(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                                 uint8_t* board_dev, uint32_t* meta_dev, uint32_t* ep_dev,
                                 uint64_t* clock_dev, int64_t n, uint64_t seed,
                                 uint64_t board_offset, uint32_t env_flags, int k_steps,
                                 int depth, uint8_t* fin_dev, uint32_t* result_dev, int device_id,
                                 void* stream);

/* The same over the staged table lut_dev int32[S][T][16^m] of `spec` and `stages`, every leaf
 * valued at its own stage, as g2048_stagesearch_expectimax takes it. */
G2048_API int g2048_ntplay_staged_steps(const g2048_ntuple_spec* spec,
                                        const g2048_ntstage_spec* stages, const int32_t* lut_dev,
                                        uint8_t* board_dev, uint32_t* meta_dev, uint32_t* ep_dev,
                                        uint64_t* clock_dev, int64_t n, uint64_t seed,
                                        uint64_t board_offset, uint32_t env_flags, int k_steps,
                                        int depth, uint8_t* fin_dev, uint32_t* result_dev,
                                        int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntplay_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTPLAY_H */
