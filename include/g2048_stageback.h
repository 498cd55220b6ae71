/* g2048_stageback.h -- C ABI of backward episode learning on the staged batch-mean
 * temporal-coherence rule for the multi-stage n-tuple value network (libg2048_stageback.so).
 *
 * Every other learner of the family is forward and online: an afterstate is updated against its
 * successor in the call that produces the successor, so what the terminal position teaches moves
 * one step towards the start of the game per later visit.  g2048_stagedelay_step carries an error
 * backwards over a window of at most 8 steps.  This library is BACKWARD learning (Matsuzaki 2017,
 * the paper g2048_ntrestart.h takes its restart pool from): an episode is recorded while it is
 * played, and once it has ended it is learned from its last afterstate to its first, each
 * afterstate against the successor that was updated in the call before.  A replaying board makes
 * one set of 8 T hits per call, and every hit stays one sample "this afterstate should move by
 * delta", so the batch mean of g2048_stagemeantc.h keeps its meaning.  On gfx950
 * (csrc/g2048_stageback.hip).  It is a library of its own: every other header and library keeps
 * its ABI, and this library does not link against another library of the project -- it takes the
 * same spec, the same stage spec and the same table.  Boards, moves, legal masks and status codes
 * are those of g2048.h.
 *
 * The rule, in integer arithmetic (mathematical integers; every result is an exact integer)
 * -----------------------------------------------------------------------------------------
 * Notation of g2048_ntuple.h (idx(b, g, t), q[a], after(b, a), gain(b, a), legal(b), F = 10), of
 * g2048_ntstage.h (S, stage(b), UNSET, val(s, t, i), V(b)), of g2048_stagemean.h (D, C) and of
 * g2048_stagemeantc.h (m, E, A, rate).
 *
 * Parameter  horizon L: how many afterstates of an episode are kept.  1 <= L <= 2^20 and
 *            n L <= 2^31.  lr_num and lr_shift as everywhere.
 *
 * State  lut, acc, ea  exactly as in g2048_stagemeantc.h.
 *        traj   u8 traj[n][2][L][16], 16-byte aligned: per board two buffers of L afterstates.
 *        gain   i32 gain[n][2][L]: the merge gain of the move that produced the afterstate in the
 *               same slot.  A gain is at most 2^31 (eight merges of two 27s); the plane holds its
 *               32-bit pattern and the kernels read it as unsigned.
 *        cur    u8 cur[n]: the buffer being recorded.  Only bit 0 counts; the other buffer is the
 *               replay buffer.
 *        rec    u32 rec[n]: afterstates recorded in the running episode.
 *        rep_n, rep_k  u32 [n]: the length of the episode being replayed, and how many of its
 *               afterstates are already updated.
 *        All zeros is the fresh state.  The k-th afterstate of an episode (k from 0) lives in
 *        slot k mod L, so a longer episode keeps its last L.  The layout is board-major so that
 *        the two afterstates of a replay, slots j and j + 1, are usually one 32-byte sector.
 *
 * One call.  Every read of lut, ea, traj, gain and the counters sees the state before the call.
 *   play     q, action and after(b, action) are g2048_ntstage_act's, word for word, on the
 *            pre-call table; with no legal move action = 0
 *   replay   board i replays iff rep_k < min(rep_n, L).  Then j = rep_n - 1 - rep_k, x = slot
 *            j mod L of the replay buffer, and
 *              target = 0                                      if rep_k == 0 (x is the last one)
 *                     = (gain of slot (j + 1) mod L << F) + V(y)   otherwise, y that slot's
 *                                                              afterstate
 *              err    = target - V(x)
 *              delta  = (int32)((err * lr_num) >> lr_shift)    arithmetic shift (floor)
 *            V at each board's own stage, with fall-through.  A board that does not replay has
 *            err = delta = 0.
 *   promote, hit, move  are g2048_stagemeantc_step's, word for word, with x in the place of prev
 *            and "replays" in the place of has_prev: x's entries at stage(x) are promoted whatever
 *            delta is; every pair (g, t) of a replaying board with delta != 0 hits the staged entry
 *            (stage(x), t, idx(x, g, t)); every hit entry moves once by m = floor(D / C) scaled by
 *            its rate(E, A), E += m, A += |m|; m == 0 leaves the entry and its ea untouched
 *   commit   a replaying board gets rep_k += 1.
 *            if legal(b) != 0: after(b, action) and gain(b, action) go to slot rec mod L of
 *              buffer cur, and rec += 1
 *            if legal(b) == 0 and rec > 0, the episode closes: cur ^= 1, rep_n = rec, rep_k = 0,
 *              rec = 0; what was left of an older replay is dropped, after its transition of this
 *              call was made
 *            if legal(b) == 0 and rec == 0: nothing more changes.
 *
 * Outputs  action_out u8[n] and delta_out i32[n], required; x_out u8[n][16], required, 16-byte
 *          aligned: row i is written iff board i replays; replay_out u8[n], required: 1 iff board
 *          i replays, else 0; err_out i64[n] may be NULL.  delta_out, x_out and replay_out are also
 *          the hand-over between the launches.
 *
 * Consequences
 *   1. A call in which no board replays leaves lut, ea and acc untouched; its actions are
 *      g2048_ntstage_act's.
 *   2. A call in which every replaying board has rep_k == 0 leaves lut and ea as
 *      g2048_stagemeantc_step leaves them, given any terminal board, prev = x and has_prev =
 *      replays.
 *   3. An episode of M afterstates is replayed in min(M, L) calls, newest first, and then the
 *      board idles.  Its afterstate j is valued against the table that already holds the update
 *      of j + 1.
 *   4. Every call makes at most one set of 8 T hits per board, and no add lands on UNSET, because
 *      x is promoted in the call that hits it.  A caller may therefore replace the table without
 *      resetting the state, unlike the ring of g2048_stagedelay.h.
 *   5. acc is all zero after every call; |E| <= A is preserved; the result depends on no order of
 *      boards or lanes; a batch given k times in lock-step leaves what the batch given once
 *      leaves.
 *   6. Recording writes buffer cur & 1 and replay reads buffer (cur & 1) ^ 1, so they never share
 *      a byte.
 *
 * Domain: that of g2048_stagemeantc_step; rec < 2^32 - 1.  The kernels take cur & 1 and every
 * slot mod L, and a board with rep_k >= min(rep_n, L) idles, so corrupted counters cannot index
 * outside a board's own planes.
 */
#ifndef G2048_STAGEBACK_H
#define G2048_STAGEBACK_H

#include <stdint.h>

#include "g2048.h"
#include "g2048_ntuple.h"
#include "g2048_ntstage.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_STAGEBACK_MAX_HORIZON (1 << 20)
#define G2048_STAGEBACK_MAX_SLOTS ((int64_t)1 << 31) /* the bound of n * horizon */
#define G2048_STAGEBACK_RATE_BITS 16
#define G2048_STAGEBACK_MAX_A (((int64_t)1 << 62) - 1)

/* Host only: rate(E, A) of g2048_stagemeantc.h, in [0, 2^16].  Outside the domain (A < 0, A >
 * G2048_STAGEBACK_MAX_A or |E| > A) it returns G2048_EINVAL. */
G2048_API int32_t g2048_stageback_rate(int64_t E, int64_t A);

/* Bytes of the workspace acc for a spec and a stage spec (16 S T 16^m; ea has the same size), or
 * G2048_EINVAL for a bad spec or a bad stage spec. */
G2048_API int64_t g2048_stageback_acc_bytes(const g2048_ntuple_spec* spec,
                                            const g2048_ntstage_spec* stages);

/* Bytes of traj for n boards and a horizon: 32 n L (gain is a quarter of that, 8 n L), or
 * G2048_EINVAL for n outside [1, G2048_MAX_BOARDS], a horizon outside [1,
 * G2048_STAGEBACK_MAX_HORIZON] or n * horizon above G2048_STAGEBACK_MAX_SLOTS. */
G2048_API int64_t g2048_stageback_traj_bytes(int64_t n, int32_t horizon);

/* One call (see above): g2048_stagemeantc_step's arguments with the trajectory, its counters and
 * the horizon in the place of prev_dev and has_prev_dev, and three more outputs.  lut_dev, acc_dev
 * and ea_dev as there; boards_dev u8[n][16] (16-byte aligned); traj_dev u8[n][2][L][16] (16-byte
 * aligned), gain_dev i32[n][2][L] (4-byte aligned), cur_dev u8[n] and rec_dev, rep_n_dev,
 * rep_k_dev u32[n] (4-byte aligned) are read and updated; action_out_dev u8[n], delta_out_dev
 * i32[n], x_out_dev u8[n][16] (16-byte aligned) and replay_out_dev u8[n] are required,
 * err_out_dev i64[n] may be NULL.  1 <= n <= G2048_MAX_BOARDS, `stream` a hipStream_t (NULL =
 * default).  Stream-ordered and asynchronous: no allocation and no host sync, so a call may be
 * captured into a hipGraph; the counters live in device memory for that reason.  Bad arguments
 * (those of g2048_stagemeantc_step; any of the new pointers NULL or misaligned; horizon or
 * n * horizon out of range) return G2048_EINVAL before any device work.
 *
 * Three launches on the stream, as in the batch-mean family.
 *   The first is g2048_ntstage_act's policy with a second set of lookups: of a replaying board's
 *   32 lanes, the 8 of move 0 gather x's entries and store the promoted values (see
 *   g2048_stagemeantc.h on why that needs no ordering), the 8 of move 1 gather y's.  One lane per
 *   board reads the counters and hands them to the others, writes action, delta, err, x_out and
 *   replay_out, and commits the counters; the lane that holds after(b, action) records it with its
 *   gain.  That board's lanes are the only readers and writers of its counters and planes in the
 *   call, all of one wave, their loads before their stores, and the buffer they read is not the
 *   one they write: every read of traj, gain and the counters sees the state before the call.
 *   The second only adds (delta, 1) into acc for the entries of x_out, as g2048_stagemeantc_step's
 *   second does for prev.
 *   The third takes (D, C) out by atomic exchange and the owning lane moves the entry and its ea
 *   (g2048_stagemeantc.h).  The second and the third need neither the trajectory nor the counters.
 * No float anywhere; the only atomics are the family's 32-bit and 64-bit integer adds and
 * exchanges. */
G2048_API int g2048_stageback_step(const g2048_ntuple_spec* spec,
                                   const g2048_ntstage_spec* stages, int32_t* lut_dev,
                                   int64_t* acc_dev, int64_t* ea_dev, const uint8_t* boards_dev,
                                   int64_t n, uint8_t* traj_dev, int32_t* gain_dev,
                                   uint8_t* cur_dev, uint32_t* rec_dev, uint32_t* rep_n_dev,
                                   uint32_t* rep_k_dev, int32_t horizon, int32_t lr_num,
                                   int32_t lr_shift, uint8_t* action_out_dev,
                                   int32_t* delta_out_dev, uint8_t* x_out_dev,
                                   uint8_t* replay_out_dev, int64_t* err_out_dev, int device_id,
                                   void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_stageback_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_STAGEBACK_H */
