/* g2048_stagedelay.h -- C ABI of delayed TD(lambda) on the staged batch-mean temporal-coherence
 * rule for the multi-stage n-tuple value network (libg2048_stagedelay.so).
 *
 * g2048_ntlambda_step runs the EAGER truncated lambda-return: every step walks a board's ring of
 * H afterstates and adds H sets of updates, on a single table under the summed rule.
 * g2048_stagemeantc_step is the strongest rule of the family -- staged table, batch mean, a rate
 * per entry -- and has no lambda.  This library is the DELAYED form of the lambda-return
 * (Jaskowski 2017) on that rule: an afterstate is updated once, when it leaves a window of H
 * steps, by the lambda-weighted sum of the H errors seen while it sat in the window.  A board
 * still makes about one set of table hits per step, and every hit stays one sample "this
 * afterstate should move by delta", so the mean over an entry's hits keeps its meaning (eager
 * traces would mix delta, delta / 2 and delta / 4 of one board into one mean).  On gfx950
 * (csrc/g2048_stagedelay.hip).  It is a library of its own: every other header and library keeps
 * its ABI, and this library does not link against another library of the project -- it takes the
 * same spec, the same stage spec and the same table.  Boards, moves, legal masks and status codes
 * are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h (idx(b, g, t), q[a], after(b, a), legal(b), F = 10), of
 * g2048_ntstage.h (S, stage(b), UNSET, val(s, t, i), V(b)), of g2048_stagemean.h (D, C), of
 * g2048_ntmeantc.h / g2048_nttc.h (m, E, A, rate) and of g2048_ntlambda.h (H, s, the ring).
 *
 * Parameters  horizon H, 1 <= H <= 8; lam_shift s, 1 <= s <= 31 and (H - 1) s <= 31: lambda =
 *             2^-s.  These are g2048_ntlambda_step's bounds.  lr_num and lr_shift as everywhere.
 *
 * State  lut, acc, ea  exactly as in g2048_stagemeantc.h.
 *        hist   u8 hist[H][n][16], 16-byte aligned: H planes of n afterstates.
 *        head   u8 head[n]: the plane of board i's latest afterstate.
 *        depth  u8 depth[n]: how many afterstates of the running episode the ring holds.
 *        g      int64 g[H][n], 8-byte aligned: g[p][i] is the error sum collected so far for the
 *               afterstate in plane p, row i.
 *        All zeros is the fresh state.  "k steps back" is plane (head - k) mod H, for k < depth.
 *
 * One step.  Every read of lut, ea, hist, head, depth and g sees the state before the call.
 *   prev     the afterstate 0 steps back; has_prev = depth > 0
 *   policy, target, err = has_prev ? target - V(prev) : 0 and promote are g2048_stagemean_step's,
 *            word for word: promotion is applied to the entries of prev at stage(prev), for every
 *            board with has_prev, whatever comes later
 *   collect  for k = 0 .. depth - 1:  G_k = g_k + sgn(err) (|err| >> (k s)); the magnitude is
 *            taken in 64 bits, so the shift rounds toward zero
 *   applied  every k < depth           if legal(b) == 0   (the episode ends: the window empties)
 *            k = H - 1 only            otherwise, if depth == H   (the oldest one leaves)
 *            none                      otherwise
 *   delta_k  = (int32)((G_k * lr_num) >> lr_shift) for an applied k, arithmetic shift (floor)
 *   hit      for an applied k with delta_k != 0, every pair (g, t) hits the staged entry
 *            (stage(hist_k), t, idx(hist_k, g, t)) with delta_k; pairs that coincide are each a
 *            hit, within an afterstate and across the afterstates of one board or of many
 *   move     for every staged entry hit at least once, g2048_stagemeantc_step's move, word for
 *            word: m = floor(D / C); step = (m rate(E, A)) >> 16 added to the entry's value after
 *            promotion; E += m, A += |m|; m == 0 leaves the entry and its ea untouched
 *   commit   if legal(b) != 0: head = (head + 1) mod H, that plane's row becomes after(b, action)
 *            and its g becomes 0, depth = min(depth + 1, H), and every kept slot stores its G_k;
 *            otherwise depth = 0, and planes, head and g stay as they are.
 *
 * Outputs  action_out u8[n]; delta_out i32[H][n], required and also the hand-over between the
 *          launches: plane k, row i is delta_k if k is applied for board i in this call, else 0;
 *          err_out i64[n] may be NULL.
 *
 * Consequences
 *   1. H = 1 is g2048_stagemeantc_step exactly: plane 0 is prev, depth is has_prev, and lut, ea
 *      and acc are equal after every call.  g (which stays zero) and s have no effect.
 *   2. The effective update of an afterstate that leaves a full window is
 *      lr * sum over k < H of lambda^k err_k, each err_k taken against the table of its own call.
 *      With H = 2, s = 31 and |err| < 2^31 the second term is 0: the staged batch-mean TC step,
 *      delayed by one call.
 *   3. A non-terminal call makes at most one set of 8 T hits per board, a terminal call depth
 *      sets.
 *   4. Every entry a call adds into was promoted when its afterstate was prev, in this call or an
 *      earlier one, so no add lands on UNSET.
 *   5. As in g2048_stagemeantc.h: acc is all zero after every call; |E| <= A is preserved; the
 *      UNSET pattern after a call depends neither on ea nor on g; a batch given k times leaves
 *      the state the batch given once leaves.
 *   6. The result does not depend on the order in which boards or lanes are processed.
 *
 * Domain: that of g2048_stagemeantc_step; head < H and depth <= H (the kernels clamp both, as
 * g2048_ntlambda.hip does, so a corrupted ring cannot index past the planes); |err| < 2^42, so
 * |G| < 2^43 and G * lr_num stays below 2^60; every delta_k fits int32; no entry of an afterstate
 * in the ring at k >= 1 is UNSET at its stage -- true when the ring was built by this library's
 * calls on this table, so a caller that replaces the table must reset the ring.
 */
#ifndef G2048_STAGEDELAY_H
#define G2048_STAGEDELAY_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"
#include "g2048_ntstage.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_STAGEDELAY_MAX_HORIZON 8
#define G2048_STAGEDELAY_MAX_LAM_SHIFT 31 /* also the bound of (horizon - 1) * lam_shift */
#define G2048_STAGEDELAY_RATE_BITS 16
#define G2048_STAGEDELAY_MAX_A (((int64_t)1 << 62) - 1)

/* Host only: rate(E, A) of g2048_stagemeantc.h, in [0, 2^16].  Outside the domain (A < 0, A >
 * G2048_STAGEDELAY_MAX_A or |E| > A) it returns G2048_EINVAL. */
G2048_API int32_t g2048_stagedelay_rate(int64_t E, int64_t A);

/* Bytes of the workspace acc for a spec and a stage spec (16 S T 16^m; ea has the same size), or
 * G2048_EINVAL for a bad spec or a bad stage spec. */
G2048_API int64_t g2048_stagedelay_acc_bytes(const g2048_ntuple_spec* spec,
                                             const g2048_ntstage_spec* stages);

/* One step (see above): g2048_stagemeantc_step's arguments with hist_dev, head_dev, depth_dev,
 * g_dev, horizon and lam_shift in the place of prev_dev and has_prev_dev.  lut_dev, acc_dev and
 * ea_dev as there; boards_dev u8[n][16] (16-byte aligned); hist_dev u8[H][n][16] (16-byte
 * aligned), head_dev u8[n], depth_dev u8[n] and g_dev i64[H][n] (8-byte aligned) are read and
 * updated; action_out_dev u8[n] and delta_out_dev i32[H][n] are required, err_out_dev i64[n] may
 * be NULL.  1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t (NULL = default).  Stream-ordered
 * and asynchronous: no allocation and no host sync, so a call may be captured into a hipGraph;
 * head, depth and g live in device memory for that reason.  Bad arguments (NULL or misaligned
 * pointers; ea_dev overlapping acc_dev; horizon, lam_shift or (horizon - 1) * lam_shift out of
 * range; bad lr, n, spec or stages) return G2048_EINVAL before any device work.
 *
 * Three launches on the stream, as in the batch-mean family.
 *   The first reads the table and the ring, writes action, err and the H planes of delta, and
 *   stores the promoted values (see g2048_stagemeantc.h on why that needs no ordering).  It also
 *   collects: lane k of a non-terminal board's group stores G_k of the kept slot k into g, and the
 *   lane of slot H - 1 -- the plane the commit writes next -- stores its 0.  That lane is the only
 *   reader and the only writer of that word in the call, so every read of g sees the state before
 *   the call; the third launch could not form G_k, since err_out may be NULL and a kept slot's
 *   delta plane holds 0.  A terminal board's g is not written.
 *   The second only adds (delta_k, 1) into acc, walking each board's applied slots.
 *   The third takes (D, C) out by atomic exchange, the owning lane moves the entry and its ea
 *   (g2048_stagemeantc.h), and after the barrier that ends all reads of the ring lane 0 of a
 *   board's group commits hist, head and depth.
 * No float anywhere; the only atomics are the family's 32-bit and 64-bit integer adds and
 * exchanges. */
G2048_API int g2048_stagedelay_step(const g2048_ntuple_spec* spec,
                                    const g2048_ntstage_spec* stages, int32_t* lut_dev,
                                    int64_t* acc_dev, int64_t* ea_dev, const uint8_t* boards_dev,
                                    int64_t n, uint8_t* hist_dev, uint8_t* head_dev,
                                    uint8_t* depth_dev, int64_t* g_dev, int32_t horizon,
                                    int32_t lam_shift, int32_t lr_num, int32_t lr_shift,
                                    uint8_t* action_out_dev, int32_t* delta_out_dev,
                                    int64_t* err_out_dev, int device_id, void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_stagedelay_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_STAGEDELAY_H */
