/* g2048_ntuple.h -- C ABI of the n-tuple value network (libg2048_ntuple.so).
 *
 * An n-tuple network (Szubert and Jaskowski, "Temporal difference learning of n-tuple networks
 * for the game 2048", CIG 2014) is a value function that is a sum of table lookups over small
 * groups of cells, shared across the 8 board symmetries, trained by afterstate TD(0).  This
 * library evaluates it, plays with it and trains it on gfx950 (csrc/g2048_ntuple.hip).  It is a
 * library of its own: include/g2048.h, include/g2048_search.h and their libraries keep their
 * ABI.  Boards, moves, legal masks and status codes are those of g2048.h.
 *
 * The network, in integer arithmetic (mathematical integers; every result is an exact integer)
 * --------------------------------------------------------------------------------------------
 * A board b is 16 log2 exponents, row-major, 0 = empty.  gain(b, a) is the merge-score gain of
 * move a (the sum of the values of the tiles it creates), after(b, a) the slid board (no spawn),
 * legal(b) the legal mask -- as in g2048_search.h.
 *
 * Spec   T tuples (1 <= T <= 8) of m cells each (1 <= m <= 6, every tuple the same m); cells are
 *        0..15 and distinct within a tuple.
 * Table  int32 lut[T][16^m], contiguous.  Values are fixed point with F = 10 fraction bits
 *        (G2048_NTUPLE_FRAC_BITS) in merge-score units.
 *
 * Symmetries  g = 0..7 with tr = g >> 2, fc = (g >> 1) & 1, fr = g & 1:
 *   g(b)[r][c]   = b'[fr ? 3 - r : r][fc ? 3 - c : c],  b' = b if tr == 0, else b'[r][c] = b[c][r]
 *   idx(b, g, t) = sum over k < m of min(g(b)[cell(t, k)], 15) << 4k
 *                  (exponents >= 16 are clamped in the index only)
 *   V(b)         = sum over t < T, g < 8 of lut[t][idx(b, g, t)]                 as an int64
 *                  (indices that coincide on a symmetric board count once per (g, t))
 *
 * Policy
 *   q[a]   = (gain(b, a) << F) + V(after(b, a))    for a legal a
 *   q[a]   = INT64_MIN                             for an illegal a
 *   action = the smallest a with the largest q; with no legal move action = 0 and after = b.
 *
 * TD step.  Per board there is state prev (u8[16]) and has_prev (u8).  All reads of the table see
 * it as it was before the call.
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0
 *   delta  = (int32)((err * lr_num) >> lr_shift)         arithmetic shift (floor)
 *   for every board with has_prev and delta != 0:
 *       lut[t][idx(prev, g, t)] += delta for all 8 T pairs (g, t)       additions modulo 2^32
 *   then prev = after(b, action) and has_prev = 1 if legal(b) != 0; else has_prev = 0 and prev
 *   is left as it is.
 * The caller then steps the environment with the returned actions; at a terminal board the
 * environment's own done / auto-reset takes over.
 *
 * Domain: exponents <= 27 (the merge gain is then exact in 32 bits; a 4x4 game cannot pass 17),
 * 0 <= lr_num <= 2^16, 0 <= lr_shift <= 31.  Every result is exact while no table entry and no
 * delta leaves int32; beyond that the additions wrap and the result is out of domain.
 */
#ifndef G2048_NTUPLE_H
#define G2048_NTUPLE_H

#include <stdint.h>

#include "g2048.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTUPLE_MAX_TUPLES 8
#define G2048_NTUPLE_MAX_CELLS 6
#define G2048_NTUPLE_FRAC_BITS 10
#define G2048_NTUPLE_MAX_LR_NUM (1 << 16)
#define G2048_NTUPLE_MAX_LR_SHIFT 31

typedef struct {
    int32_t n_tuples, n_cells;
    uint8_t cells[G2048_NTUPLE_MAX_TUPLES][G2048_NTUPLE_MAX_CELLS];
} g2048_ntuple_spec;

/* T * 16^m, the number of int32 entries of the table, or G2048_EINVAL for a bad spec. */
G2048_API int64_t g2048_ntuple_lut_entries(const g2048_ntuple_spec* spec);

/* Host only: out[g][t][k] = the cell of b that g(b)[cell(t, k)] reads, for g < 8, t < T, k < m
 * (entries with t >= T or k >= m are set to 0). */
G2048_API int g2048_ntuple_expand(const g2048_ntuple_spec* spec,
                                  uint8_t out[8][G2048_NTUPLE_MAX_TUPLES][G2048_NTUPLE_MAX_CELLS]);

/* All device entry points: boards_dev u8[n][16] (16-byte aligned), lut_dev int32[T][16^m],
 * 1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t (NULL = default).  Stream-ordered and
 * asynchronous: no allocation, no host sync, no workspace, so a call may be captured into a
 * hipGraph.  Bad arguments return G2048_EINVAL before any device work. */

/* values_out_dev i64[n] = V(board). */
G2048_API int g2048_ntuple_values(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                                  const uint8_t* boards_dev, int64_t n, int64_t* values_out_dev,
                                  int device_id, void* stream);

/* The policy: q_out_dev i64[n][4] (move order up/down/left/right), action_out_dev u8[n],
 * after_out_dev u8[n][16] (16-byte aligned) = after(board, action).  Each may be NULL, not all. */
G2048_API int g2048_ntuple_act(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                               const uint8_t* boards_dev, int64_t n, int64_t* q_out_dev,
                               uint8_t* action_out_dev, uint8_t* after_out_dev, int device_id,
                               void* stream);

/* One TD(0) step (see above): prev_dev u8[n][16] (16-byte aligned) and has_prev_dev u8[n] are
 * read and updated; action_out_dev u8[n] and delta_out_dev i32[n] are required, err_out_dev
 * i64[n] may be NULL.  Two launches on the stream: the first only reads the table and writes
 * action, err and delta; the second only adds into the table (32-bit integer atomics, so the
 * result does not depend on their order) and commits prev / has_prev, recomputing
 * after(board, action) from boards_dev and action_out_dev.  delta_out_dev is the hand-over
 * between the two. */
G2048_API int g2048_ntuple_td_step(const g2048_ntuple_spec* spec, int32_t* lut_dev,
                                   const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                                   uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                                   uint8_t* action_out_dev, int32_t* delta_out_dev,
                                   int64_t* err_out_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntuple_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTUPLE_H */
