/* g2048_search.h -- C ABI of the batched expectimax search player (libg2048_search.so).
 *
 * The reference reserves a slot for a searching player and leaves it empty
 * (Player.play_state_space_search_game, src/player.py:87-88).  This library fills it with a
 * depth-limited expectimax over the stochastic game, one wavefront per board on gfx950
 * (csrc/g2048_search.hip).  It is a library of its own: include/g2048.h and libg2048.so keep
 * their ABI.  Boards, moves, legal masks, status codes and flags are those of g2048.h.
 *
 * The search, in integer arithmetic (mathematical integers; every result is an int64)
 * -----------------------------------------------------------------------------------
 * A board b is 16 log2 exponents, row-major, 0 = empty.  gain(b, a) is the merge-score gain of
 * move a (the sum of the values of the tiles it creates), after(b, a) the slid board (no spawn),
 * legal(b) the legal mask.  Weights are int32: gain, empty, smooth, mono, corner, lost.
 *
 * Leaf heuristic  H(b) = empty * E - smooth * Sm - mono * Mo + corner * C
 *   E   number of empty cells
 *   Sm  sum of |e_x - e_y| over the 24 orthogonally adjacent cell pairs (empty = exponent 0)
 *   Mo  sum over the 8 lines (4 rows, 4 columns) of min(inc, dec), where over the line's three
 *       adjacent pairs inc = sum max(e_{k+1} - e_k, 0) and dec = sum max(e_k - e_{k+1}, 0)
 *   C   the largest exponent if one of the four corner cells holds it, else 0
 *
 * Vmax(b, d)    = -lost                                     if legal(b) == 0
 *               = H(b)                                      if d == 0
 *               = max over legal a of [ gain_w * gain(b, a) + Vchance(after(b, a), d - 1) ]
 * Vchance(s, d) = floor( sum over the empty cells c of s of
 *                        [ (W - w4) * Vmax(s with a 2 at c, d) + w4 * Vmax(s with a 4 at c, d) ]
 *                        / (W * n_empty) )                  floor toward -infinity
 *   (W, w4) = (2, 1) for p(4) = 0.5 (the default), (10, 1) for p(4) = 0.1 (G2048_P4_10).
 *
 * Root, depth >= 1 player moves:
 *   value[a] = gain_w * gain(b, a) + Vchance(after(b, a), depth - 1)   for a legal a
 *   value[a] = INT64_MIN                                               for an illegal a
 *   action   = the smallest a with the largest value among the legal moves; with no legal move
 *              action = 0 and all four values are INT64_MIN.
 *
 * Default weights: gain 256, empty 2048, smooth 256, mono 1024, corner 512, lost 1000000.
 *
 * Domain: 1 <= depth <= 4; exponents <= 30; 0 <= weight <= 2^24 and lost <= 2^30.  The kernel
 * computes in int64 and is exact while the chance node's numerator fits:
 *   150 * (gain_w * (depth * T + 8 * depth^2) + 2^24 * 1200) < 2^63,
 * with T the sum of the root board's tile values (a move's gain is at most the tile sum).  The
 * default weights satisfy this for every board of the domain; at gain_w = 2^24 it holds for
 * T <= 2^29.
 */
#ifndef G2048_SEARCH_H
#define G2048_SEARCH_H

#include <stdint.h>

#include "g2048.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_SEARCH_MAX_DEPTH 4
#define G2048_SEARCH_MAX_WEIGHT (1 << 24)
#define G2048_SEARCH_MAX_LOST (1 << 30)

typedef struct {
    int32_t gain, empty, smooth, mono, corner, lost;
} g2048_search_weights;

/* Writes the default weights (see above) into *w. */
G2048_API void g2048_search_default_weights(g2048_search_weights* w);

/* Expectimax over n boards: boards_dev u8[n][16] (16-byte aligned), values_out_dev i64[n][4]
 * (8-byte aligned, move order up/down/left/right), action_out_dev u8[n].  Either output may be
 * NULL, not both.  flags accepts G2048_P4_10 only; w == NULL means the default weights.
 * Stream-ordered and asynchronous: no allocation, no host sync, no workspace, so the call may be
 * captured into a hipGraph.  `stream` is a hipStream_t (NULL = default).  Bad arguments return
 * G2048_EINVAL before any device work. */
G2048_API int g2048_search_expectimax(const uint8_t* boards_dev, int64_t n, int depth,
                                      uint32_t flags, const g2048_search_weights* w,
                                      int64_t* values_out_dev, uint8_t* action_out_dev,
                                      int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_search_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_SEARCH_H */
