/* g2048_stagesearch.h -- C ABI of the expectimax search over the multi-stage n-tuple network
 * (libg2048_stagesearch.so).
 *
 * g2048_ntsearch.h searches with one table at the leaves; g2048_ntstage.h gives every stage of
 * the game, by largest tile, a table of its own.  This library is the search of the first over
 * the value function of the second: every leaf is valued at ITS OWN stage (a merge inside the
 * tree can raise the largest tile, so a leaf can sit in a later stage than the root), and an
 * entry that is UNSET falls through to the stage below, as everywhere in g2048_ntstage.h.  One
 * wavefront per board on gfx950 (csrc/g2048_stagesearch.hip).  It is a library of its own: the
 * other headers and their libraries keep their ABI, and this one links against none of them --
 * it reads the same spec, the same stage spec and the same table.
 *
 * Definition, in mathematical integers (every result is an exact int64)
 * ---------------------------------------------------------------------
 * Spec, symmetries g, idx(b, g, t) (the index clamps an exponent at 15), gain, after, legal,
 * F = 10 and the move order are those of g2048_ntuple.h; stage(b), val(s, t, i) and UNSET those
 * of g2048_ntstage.h; (W, w4) = (2, 1) for p(4) = 0.5 (the default) and (10, 1) for p(4) = 0.1
 * (G2048_P4_10), as in g2048_ntsearch.h.
 *
 * V(s)         = sum over t < T, g < 8 of val(stage(s), t, idx(s, g, t))
 *                stage(s) from s's own largest exponent (the true one, not the clamped one)
 * Vmax(b, d)   = 0                                              if legal(b) == 0
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
 * The table is only read: the search promotes nothing.
 *
 * Three identities follow from the definition:
 *   1. Depth 1 has no chance node: its value and action are exactly g2048_ntstage_act's q and
 *      action.
 *   2. With S = 1 and a table without UNSET, V is g2048_ntuple.h's V, and the call is
 *      g2048_ntsearch_expectimax exactly.
 *   3. A table whose stage 0 is a single table (without INT32_MIN entries) and whose other
 *      stages are all UNSET resolves every val to the single table's entry, whatever the stage:
 *      it searches exactly as that single table does.
 *
 * Domain: root exponents <= 24.  A player move raises the largest exponent by at most one, so
 * with depth <= 3 every board in the tree stays <= 27, the largest bound a stage spec may hold
 * and the range where the 32-bit merge gain is exact.
 *
 * No overflow: the argument of g2048_ntsearch.h, unchanged.  |val| <= 2^31, so |V| <= 8 * 8 *
 * 2^31 = 2^37; a move's gain is at most 2^31, so (gain << F) adds at most 2^41 per ply and every
 * Vmax and Vafter of the tree lies within 3 * 2^41 + 2^37 < 2^43.  A chance node sums at most 16
 * cells with total weight W <= 10 each: |numerator| < 160 * 2^43 < 2^51, far below 2^63.
 */
#ifndef G2048_STAGESEARCH_H
#define G2048_STAGESEARCH_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntstage.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_STAGESEARCH_MAX_DEPTH 3
#define G2048_STAGESEARCH_MAX_EXPONENT 24

/* Expectimax over n boards with the staged table lut_dev int32[S][T][16^m] of `spec` and `stages`
 * at the leaves: boards_dev u8[n][16] (16-byte aligned), values_out_dev i64[n][4] (8-byte
 * aligned, move order up/down/left/right), action_out_dev u8[n].  Either output may be NULL, not
 * both.  flags accepts G2048_P4_10 only.  1 <= n <= G2048_MAX_BOARDS, 1 <= depth <=
 * G2048_STAGESEARCH_MAX_DEPTH.  Stream-ordered and asynchronous: no allocation, no host sync, no
 * workspace, so the call may be captured into a hipGraph.  `stream` is a hipStream_t (NULL =
 * default).  Bad arguments (those of g2048_ntstage.h's calls and of g2048_ntsearch_expectimax:
 * spec, stage spec, alignment, depth, flags, both outputs NULL) return G2048_EINVAL before any
 * device work. */
G2048_API int g2048_stagesearch_expectimax(const g2048_ntuple_spec* spec,
                                           const g2048_ntstage_spec* stages,
                                           const int32_t* lut_dev, const uint8_t* boards_dev,
                                           int64_t n, int depth, uint32_t flags,
                                           int64_t* values_out_dev, uint8_t* action_out_dev,
                                           int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_stagesearch_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_STAGESEARCH_H */
