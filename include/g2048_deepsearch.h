/* g2048_deepsearch.h -- C ABI of the wide expectimax over the n-tuple value networks
 * (libg2048_deepsearch.so): depths up to 5, one tree spread over many wavefronts.
 *
 * g2048_ntsearch.h and g2048_stagesearch.h give one wavefront to one board and stop at three
 * player moves.  That is the right mapping for tens of thousands of boards and the wrong one for
 * playing a game or evaluating a few hundred: one board at depth 3 is one wave of the 8 192 a
 * gfx950 holds.  This library runs the same search with the top of the tree expanded breadth-first
 * into a workspace: every board of the frontier is then a root of its own for the per-wave walk,
 * and the values are backed up level by level.  Because Vafter floors once per chance node and
 * Vmax is a plain maximum, the tree splits exactly there: the result is the same int64 as the
 * recursion, bit for bit, whatever the split.  It is a library of its own (csrc/
 * g2048_deepsearch.hip): the other headers and their libraries keep their ABI, and this one links
 * against none of them -- it reads the same spec, the same stage spec and the same tables.
 *
 * Definition, in mathematical integers (every result is an exact int64)
 * ---------------------------------------------------------------------
 * gain, after, legal, F = 10 and the move order are those of g2048_ntuple.h; (W, w4) = (2, 1) for
 * p(4) = 0.5 (the default) and (10, 1) for p(4) = 0.1 (G2048_P4_10).  V(s) is g2048_ntuple.h's
 * (the sum of the 8 T table entries of s) for g2048_deepsearch_expectimax, and g2048_ntstage.h's
 * for g2048_deepsearch_staged_expectimax: every leaf valued at ITS OWN stage, stage(s) from s's
 * own largest exponent, an UNSET entry falling through to the stage below (0 below stage 0).
 *
 * Vmax(b, d)   = 0                                              if legal(b) == 0
 *              = max over legal a of [ (gain(b, a) << F) + Vafter(after(b, a), d - 1) ]
 * Vafter(s, 0) = V(s)
 * Vafter(s, d) = floor( sum over the empty cells c of s of
 *                       [ (W - w4) * Vmax(s with a 2 at c, d) + w4 * Vmax(s with a 4 at c, d) ]
 *                       / (W * n_empty) )                       floor toward -infinity
 *
 * Root, 1 <= depth <= 5 player moves:
 *   value[a] = (gain(b, a) << F) + Vafter(after(b, a), depth - 1)   for a legal a
 *   value[a] = INT64_MIN                                            for an illegal a
 *   action   = the smallest a with the largest value; with no legal move action = 0 and all
 *              four values are INT64_MIN.
 *
 * For depth <= 3 this is g2048_ntsearch_expectimax / g2048_stagesearch_expectimax exactly.
 *
 * The split.  top_plies in {0, 1, 2} player moves are expanded breadth-first; the rest, sub =
 * depth - top_plies in 1..3, is the per-wave walk.  Level 0 holds the n roots.  A max-node board b
 * in slot q of level j has 128 slots of level j + 1:
 *   slot(q, a, tile, cell) = q * 128 + a * 32 + tile * 16 + cell      tile 0 = a 2, tile 1 = a 4
 * It holds after(b, a) with the tile at `cell` if a is legal for b and `cell` is empty in
 * after(b, a), and a sentinel otherwise (all 16 bytes 0xFF; every slot below a sentinel is a
 * sentinel).  Level 1 has 128 slots per root and level 2 has 16 384.  The call then
 *   1. expands level j into level j + 1 for j = 0 .. top_plies - 1 (one launch each),
 *   2. computes Vmax(board, sub) of every slot of level top_plies that is no sentinel (one
 *      launch; a board without a legal move gives 0),
 *   3. backs up, deepest level first (one launch each): the max node in slot q of level j takes
 *        value[a] = (gain << F) + floor( sum over the empty cells c of after(b, a) of
 *                   [ (W - w4) * Vmax(slot(q, a, 0, c)) + w4 * Vmax(slot(q, a, 1, c)) ]
 *                   / (W * n_empty) )
 *      and Vmax = the largest value[a] over its legal moves, 0 with none; at level 0 the four
 *      value[a] and the action are the result.
 * With top_plies = 0 there is no workspace and the roots go to the per-wave walk directly: the
 * mapping of the two other search libraries, kept so that every split can be compared inside one
 * library.  Every slot a launch reads was written by an earlier launch of the same call, so the
 * result does not depend on what the workspace held.  The launches are ordered by the stream: no
 * atomics, no cooperative launch, nothing waits on another workgroup.
 *
 * Workspace: each slot holds a 16-byte board and an 8-byte Vmax, so
 *   g2048_deepsearch_workspace_bytes(n, 0) = 0
 *   g2048_deepsearch_workspace_bytes(n, 1) = n * 128 * 24           =   3 072 n
 *   g2048_deepsearch_workspace_bytes(n, 2) = n * (128 + 16 384) * 24 = 396 288 n
 *
 * Domain: root exponents <= 22.  A player move raises the largest exponent by at most one, so
 * with depth <= 5 every board in the tree stays <= 27, the largest bound a stage spec may hold
 * and the range where the 32-bit merge gain is exact.  The spec limits are those of
 * g2048_ntuple.h (T <= 8, m <= 6) and g2048_ntstage.h.
 *
 * No overflow: |V| <= 8 * 8 * 2^31 = 2^37.  A move's gain is at most 2^31, so (gain << F) adds at
 * most 2^41 per ply and every Vmax and Vafter of the tree lies within 5 * 2^41 + 2^37 < 2^44.  A
 * chance node sums at most 16 cells with total weight W <= 10 each: |numerator| < 160 * 2^44
 * < 2^52, far below 2^63.
 */
#ifndef G2048_DEEPSEARCH_H
#define G2048_DEEPSEARCH_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntstage.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_DEEPSEARCH_MAX_DEPTH 5
#define G2048_DEEPSEARCH_MAX_EXPONENT 22
#define G2048_DEEPSEARCH_MAX_TOP_PLIES 2
#define G2048_DEEPSEARCH_MAX_SUB_DEPTH 3

/* The bytes a call over n boards with `top_plies` needs (see above; 0 for top_plies = 0).
 * G2048_EINVAL for n outside [1, G2048_MAX_BOARDS] or top_plies outside [0, 2].  No GPU needed. */
G2048_API int64_t g2048_deepsearch_workspace_bytes(int64_t n, int top_plies);

/* Expectimax over n boards with the table lut_dev int32[T][16^m] of `spec` at the leaves:
 * boards_dev u8[n][16] (16-byte aligned), values_out_dev i64[n][4] (8-byte aligned, move order
 * up/down/left/right), action_out_dev u8[n].  Either output may be NULL, not both.  flags accepts
 * G2048_P4_10 only.  1 <= n <= G2048_MAX_BOARDS, 1 <= depth <= G2048_DEEPSEARCH_MAX_DEPTH,
 * 0 <= top_plies <= 2 and 1 <= depth - top_plies <= 3.  With top_plies > 0 workspace_dev is
 * device memory, 16-byte aligned, of at least g2048_deepsearch_workspace_bytes(n, top_plies)
 * bytes (workspace_bytes says how many it has); with top_plies = 0 it is not looked at and may be
 * NULL.  Stream-ordered and asynchronous: no allocation, no host sync, 2 top_plies + 1
 * launches on `stream` (a hipStream_t, NULL = default), so the call may be captured into a
 * hipGraph as one chain.  Bad arguments return G2048_EINVAL before any device work. */
G2048_API int g2048_deepsearch_expectimax(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                                          const uint8_t* boards_dev, int64_t n, int depth,
                                          int top_plies, uint32_t flags, int64_t* values_out_dev,
                                          uint8_t* action_out_dev, void* workspace_dev,
                                          int64_t workspace_bytes, int device_id, void* stream);

/* The same over the staged table lut_dev int32[S][T][16^m] of `spec` and `stages`: every leaf is
 * valued at its own stage and UNSET falls through (g2048_stagesearch.h's V).  The further bad
 * arguments are those of g2048_ntstage.h's calls. */
G2048_API int g2048_deepsearch_staged_expectimax(const g2048_ntuple_spec* spec,
                                                 const g2048_ntstage_spec* stages,
                                                 const int32_t* lut_dev, const uint8_t* boards_dev,
                                                 int64_t n, int depth, int top_plies,
                                                 uint32_t flags, int64_t* values_out_dev,
                                                 uint8_t* action_out_dev, void* workspace_dev,
                                                 int64_t workspace_bytes, int device_id,
                                                 void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_deepsearch_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_DEEPSEARCH_H */
