/* g2048_ntstage.h -- C ABI of the multi-stage n-tuple value network (libg2048_ntstage.so).
 *
 * One table has to value an opening board and a board with a 4096 tile on it.  A multi-stage
 * network (Wu et al. 2014; Yeh et al. 2016; Jaskowski 2017) gives every stage of the game, by
 * largest tile, a table of its own, and weight promotion starts each entry of a later stage from
 * the value the earlier stage learned.  This library evaluates, plays and trains such a network
 * on gfx950 (csrc/g2048_ntstage.hip).  It is a library of its own: the other headers and their
 * libraries keep their ABI, and this one links against none of them.
 *
 * Spec, symmetries g, idx(b, g, t), gain, after, legal, F = 10 fraction bits, the move order and
 * the domain are those of g2048_ntuple.h.  Every value is a mathematical integer.
 *
 * Stages  g2048_ntstage_spec: 1 <= n_stages = S <= 8; bounds[0 .. S-2] are strictly increasing
 *         exponents in 1..27, unused entries are 0.
 *   M(b)     = the largest exponent on b (a symmetry does not change it)
 *   stage(b) = the number of k < S - 1 with M(b) >= bounds[k]
 *
 * Table   int32 lut[S][T][16^m], contiguous, at most 8 * 8 * 2^24 = 2^30 entries.  One value is
 *         not a number: G2048_NTSTAGE_UNSET = INT32_MIN means "never written".
 *   val(s, t, i) = lut[s][t][i]   if it is not UNSET
 *                = val(s-1, t, i) if s > 0
 *                = 0              otherwise
 *   A fresh network is all UNSET and values every board at 0.  A table whose stage 0 is a trained
 *   g2048_ntuple table and whose other stages are UNSET values every board as that table does.
 *
 * Value and policy
 *   V(b)   = sum over t < T, g < 8 of val(stage(b), t, idx(b, g, t))           as an int64
 *   q[a]   = (gain(b, a) << F) + V(after(b, a))   for a legal a; the stage is the AFTERSTATE's
 *            (a merge can raise it)
 *   q[a]   = INT64_MIN                            for an illegal a
 *   action = the smallest a with the largest q; with no legal move action = 0 and after = b.
 *
 * TD step.  Per board there is state prev (u8[16]) and has_prev (u8), as in
 * g2048_ntuple_td_step.  All reads see the table as it was before the call.
 *   target = the largest legal q, or 0 if legal(b) == 0
 *   err    = has_prev ? target - V(prev) : 0              V(prev) under stage(prev)
 *   delta  = (int32)((err * lr_num) >> lr_shift)          arithmetic shift (floor)
 *   for every board with has_prev (whatever its delta), with s = stage(prev):
 *       promote: every lut[s][t][idx(prev, g, t)] that is UNSET becomes val(s, t, idx) as before
 *       the call
 *   for every board with has_prev and delta != 0:
 *       lut[s][t][idx(prev, g, t)] += delta for all 8 T pairs (g, t), modulo 2^32, coinciding
 *       pairs each applied
 *   then prev = after(b, action) and has_prev = 1 if legal(b) != 0; else has_prev = 0 and prev
 *   is left as it is.
 * Promotion writes the value the entry already resolves to, so it changes no val of the pre-call
 * table, and two boards that promote the same entry write the same number: the result does not
 * depend on the order in which boards are processed.  If a stage-1 board and a stage-2 board
 * address the same (t, i) in one call and both entries are UNSET, each ends at val(0, t, i) plus
 * its own deltas; the stage-2 entry does not see the stage-1 entry's new value.  An entry that
 * the adds bring to exactly INT32_MIN is out of domain, like a wrapped entry.  With S = 1 and a
 * table without UNSET the step is g2048_ntuple_td_step exactly.
 */
#ifndef G2048_NTSTAGE_H
#define G2048_NTSTAGE_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTSTAGE_MAX_STAGES 8
#define G2048_NTSTAGE_MAX_BOUND 27
#define G2048_NTSTAGE_UNSET INT32_MIN

typedef struct {
    int32_t n_stages;
    uint8_t bounds[G2048_NTSTAGE_MAX_STAGES - 1];
} g2048_ntstage_spec;

/* S * T * 16^m, the number of int32 entries of the table, or G2048_EINVAL for a bad spec or a
 * bad stage spec. */
G2048_API int64_t g2048_ntstage_lut_entries(const g2048_ntuple_spec* spec,
                                            const g2048_ntstage_spec* stages);

/* All device entry points: boards_dev u8[n][16] (16-byte aligned), lut_dev int32[S][T][16^m],
 * 1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t (NULL = default).  Stream-ordered and
 * asynchronous: no allocation, no host sync, no workspace, so a call may be captured into a
 * hipGraph.  Bad arguments (n_stages out of range, bounds not strictly increasing or outside
 * 1..27, a non-zero unused bound among them) return G2048_EINVAL before any device work. */

/* values_out_dev i64[n] = V(board). */
G2048_API int g2048_ntstage_values(const g2048_ntuple_spec* spec,
                                   const g2048_ntstage_spec* stages, const int32_t* lut_dev,
                                   const uint8_t* boards_dev, int64_t n, int64_t* values_out_dev,
                                   int device_id, void* stream);

/* The policy: q_out_dev i64[n][4] (move order up/down/left/right), action_out_dev u8[n],
 * after_out_dev u8[n][16] (16-byte aligned) = after(board, action).  Each may be NULL, not all. */
G2048_API int g2048_ntstage_act(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                                const int32_t* lut_dev, const uint8_t* boards_dev, int64_t n,
                                int64_t* q_out_dev, uint8_t* action_out_dev,
                                uint8_t* after_out_dev, int device_id, void* stream);

/* One TD(0) step (see above): prev_dev u8[n][16] (16-byte aligned) and has_prev_dev u8[n] are
 * read and updated; action_out_dev u8[n] and delta_out_dev i32[n] are required, err_out_dev
 * i64[n] may be NULL.  Two launches on the stream.  The first reads the table, writes action, err
 * and delta, and stores the promoted values: the only table words it writes are UNSET entries,
 * each with the value it resolves to, so a concurrent read resolves to the same number whether
 * it sees the entry before or after.  The second only adds into the table (32-bit integer
 * atomics into entries that are no longer UNSET, so the result does not depend on their order)
 * and commits prev / has_prev.  delta_out_dev is the hand-over between the two. */
G2048_API int g2048_ntstage_td_step(const g2048_ntuple_spec* spec,
                                    const g2048_ntstage_spec* stages, int32_t* lut_dev,
                                    const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                                    uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                                    uint8_t* action_out_dev, int32_t* delta_out_dev,
                                    int64_t* err_out_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntstage_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTSTAGE_H */
