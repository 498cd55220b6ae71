/* g2048_ntsearch.h -- C ABI of the expectimax search over the n-tuple value network
 * (libg2048_ntsearch.so).
 *
 * Strong 2048 programs run an expectimax whose leaves are the learned afterstate values of an
 * n-tuple network (Szubert and Jaskowski, CIG 2014; Yeh et al. 2016; Jaskowski 2017).  This
 * library is that search for the network of g2048_ntuple.h, one wavefront per board on gfx950
 * (csrc/g2048_ntsearch.hip).  It is a library of its own: include/g2048.h, g2048_search.h,
 * g2048_ntuple.h and their libraries keep their ABI, and this library does not link against
 * libg2048_ntuple.so -- it reads the same spec and the same table.  Boards, moves, legal masks,
 * status codes and flags are those of g2048.h.
 *
 * The search, in integer arithmetic (mathematical integers; every result is an exact int64)
 * ------------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h: gain(b, a) the merge-score gain of move a, after(b, a) the slid
 * board (no spawn), legal(b) the legal mask, V(s) the network's value of s (the sum of its 8 T
 * table entries), F = 10 (G2048_NTUPLE_FRAC_BITS).  (W, w4) as in g2048_search.h: (2, 1) for
 * p(4) = 0.5 (the default), (10, 1) for p(4) = 0.1 (G2048_P4_10).
 *
 * Vmax(b, d)   = 0                                              if legal(b) == 0
 *                                                               (the TD target of a terminal board)
 *              = max over legal a of [ (gain(b, a) << F) + Vafter(after(b, a), d - 1) ]
 * Vafter(s, 0) = V(s)
 * Vafter(s, d) = floor( sum over the empty cells c of s of
 *                       [ (W - w4) * Vmax(s with a 2 at c, d) + w4 * Vmax(s with a 4 at c, d) ]
 *                       / (W * n_empty) )                       floor toward -infinity
 *
 * Root, 1 <= depth <= 3 player moves:
 *   value[a] = (gain(b, a) << F) + Vafter(after(b, a), depth - 1)   for a legal a
 *   value[a] = INT64_MIN                                            for an illegal a
 *   action   = the smallest a with the largest value; with no legal move action = 0 and all
 *              four values are INT64_MIN.
 *
 * The afterstate of a legal move always has an empty cell (a tile travelled or two merged), so
 * the divisor W * n_empty is never zero.  Depth 1 has no chance node: its value and action are
 * exactly g2048_ntuple_act's q and action.
 *
 * Domain: root exponents <= 24.  A player move raises the largest exponent by at most one, so
 * with depth <= 3 every board in the tree stays <= 27, where the 32-bit merge gain is exact (as
 * in g2048_ntuple.h).  The spec limits are those of g2048_ntuple.h (T <= 8, m <= 6).
 *
 * No overflow: |V| <= 8 * 8 * 2^31 = 2^37.  A move's gain is at most 2^31, so (gain << F) adds
 * at most 2^41 per ply and every Vmax and Vafter of the tree lies within 3 * 2^41 + 2^37 < 2^43.
 * A chance node sums at most 16 cells with total weight W <= 10 each: |numerator| < 160 * 2^43
 * < 2^51, far below 2^63.
 */
#ifndef G2048_NTSEARCH_H
#define G2048_NTSEARCH_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTSEARCH_MAX_DEPTH 3
#define G2048_NTSEARCH_MAX_EXPONENT 24

/* Expectimax over n boards with the table lut_dev int32[T][16^m] of `spec` at the leaves:
 * boards_dev u8[n][16] (16-byte aligned), values_out_dev i64[n][4] (8-byte aligned, move order
 * up/down/left/right), action_out_dev u8[n].  Either output may be NULL, not both.  flags accepts
 * G2048_P4_10 only.  1 <= n <= G2048_MAX_BOARDS, 1 <= depth <= G2048_NTSEARCH_MAX_DEPTH.
 * Stream-ordered and asynchronous: no allocation, no host sync, no workspace, so the call may be
 * captured into a hipGraph.  `stream` is a hipStream_t (NULL = default).  Bad arguments return
 * G2048_EINVAL before any device work. */
G2048_API int g2048_ntsearch_expectimax(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                                        const uint8_t* boards_dev, int64_t n, int depth,
                                        uint32_t flags, int64_t* values_out_dev,
                                        uint8_t* action_out_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntsearch_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTSEARCH_H */
