/* g2048_ntrestart.h -- C ABI of the per-board restart pool for n-tuple self-play
 * (libg2048_ntrestart.so).
 *
 * Every self-play trainer starts every episode from a freshly dealt board, so boards with a large
 * tile are the rare ones and the tables (or entries) that value them see a fraction of the
 * updates.  Carousel shaping (Jaskowski 2017) and the restart strategy (Matsuzaki 2017) answer
 * that: do not always start at the opening, start from a position an earlier game reached.  This
 * library keeps, per board, a device-resident pool of snapshots of that board's own games, one
 * per largest-tile level, and one call after the env's step records snapshots and replaces
 * freshly re-dealt boards with one of them, by a fixed rotation of levels
 * (csrc/g2048_ntrestart.hip).  It is a library of its own: the other headers and their libraries
 * keep their ABI, and this one links against none of them.  It takes no env handle, only the
 * env's caller-owned buffers, as g2048_env_wrap (g2048.h) exposes them.
 *
 * Everything is per board: board i reads and writes row i of every buffer and nothing else, in
 * integer arithmetic.  There are no atomics and no traffic between boards, so the result does not
 * depend on the order in which boards are processed; it is checked bit for bit against
 * tests/ntrestart_ref.py.
 *
 * State (caller-owned device buffers, n boards; all zeros is the fresh state):
 *   snap   g2048_ntrestart_slot snap[n][16], 16-byte aligned: slot e of board i holds a position
 *          of board i's own play whose largest exponent is e.
 *   valid  u16 valid[n]: bit e is set iff slot e of board i holds a snapshot.
 *   top    u8 top[n]: the largest exponent the running episode of board i has been captured at.
 *   turn   u32 turn[n]: the number of episodes board i has finished, plus a caller-chosen offset.
 * The rotation: levels u8[L], 1 <= L <= G2048_NTRESTART_MAX_ROTATION (8), every entry in 0..15;
 * 0 means "start fresh".
 *
 * One call, g2048_ntrestart_apply, after an env step that wrote done.  The env's buffers are
 * those of g2048.h: board u8[n][16], meta u32[2][n] (meta[0][i] = score, meta[1][i] = start, the
 * low 32 bits of the step clock at which the running episode began), clock u64[ceil(n / 64)].
 * Per board i, with M(b) the largest exponent on b and now = the low 32 bits of clock[i >> 6]:
 *
 *   done[i] == 0  (the board moved on)
 *     if M(board[i]) > top[i]:  slot M = {board[i], meta[0][i], (u32)(now - meta[1][i])},
 *                               bit M of valid[i] is set, top[i] = M
 *     restored_out[i] = 0
 *   done[i] != 0  (the env has just logged the episode and re-dealt the board)
 *     e = levels[turn[i] % L];  turn[i] += 1   (modulo 2^32)
 *     if e != 0 and bit e of valid[i] is set:
 *         board[i] = the slot's board, meta[0][i] = the slot's score,
 *         meta[1][i] -= the slot's moves (modulo 2^32), top[i] = e, restored_out[i] = e
 *     otherwise the fresh board is left alone, top[i] = M(board[i]) and restored_out[i] = 0
 *     The slot is kept: the episode that restarts from it overwrites a higher slot when it
 *     climbs, and a later fresh episode overwrites this one.
 *
 * A move raises M by at most one, so an episode captures every level it passes; a fresh board
 * starts at M = 1 or 2, so slot 1 may stay unset, and slot 0 always does.
 *
 * Consequences
 *   - The env derives moves as clock - start, so the score and the move count of a restarted
 *     episode continue from the snapshot: the episode log records the whole virtual game (the
 *     snapshot's past and the play since the restart), and ep[:, 3] is its largest tile.
 *   - The learners drop their previous afterstates at a terminal board: g2048_ntuple_td_step,
 *     g2048_nttc_step and g2048_ntstage_td_step set has_prev = 0 when legal(b) == 0
 *     ("else has_prev = 0" in g2048_ntuple.h, g2048_nttc.h and g2048_ntstage.h), and
 *     g2048_ntlambda_step sets depth = 0 ("otherwise: depth = 0" in g2048_ntlambda.h), which
 *     empties the ring.  The restored board is therefore a first board to them, exactly as a
 *     fresh one is, and no TD error crosses the restart.
 *   - The call reads the table of no network.
 *
 * Domain: exponents <= 15 (the domain of the n-tuple tables, 16 values per cell).  A board with a
 * larger exponent is never captured (top is left as it is), so no slot index leaves 0..15.
 */
#ifndef G2048_NTRESTART_H
#define G2048_NTRESTART_H

#include <stdint.h>

#include "g2048.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTRESTART_LEVELS 16
#define G2048_NTRESTART_MAX_ROTATION 8
#define G2048_NTRESTART_SLOT_BYTES 32

typedef struct {
    uint8_t board[16];
    uint32_t score;
    uint32_t moves;
    uint32_t pad[2]; /* written as 0 */
} g2048_ntrestart_slot;

/* Host only: the bytes of the four state buffers of n boards together,
 * n * (16 * 32 + 2 + 1 + 4), or G2048_EINVAL for n outside [1, G2048_MAX_BOARDS]. */
G2048_API int64_t g2048_ntrestart_state_bytes(int64_t n);

/* The call defined above.  levels is a host array of n_levels = L bytes, copied by value into the
 * launch.  board_dev and snap_dev are 16-byte, clock_dev 8-byte, meta_dev and turn_dev 4-byte and
 * valid_dev 2-byte aligned; restored_out_dev u8[n] may be NULL; 1 <= n <= G2048_MAX_BOARDS;
 * `stream` is a hipStream_t (NULL = default).  Stream-ordered and asynchronous, one launch: no
 * allocation, no host sync, no workspace, so the call may be captured into a hipGraph.  Bad
 * arguments (L outside 1..8, a level above 15, n out of range, a NULL or misaligned pointer)
 * return G2048_EINVAL before any device work. */
G2048_API int g2048_ntrestart_apply(const uint8_t* levels, int32_t n_levels, uint8_t* board_dev,
                                    uint32_t* meta_dev, const uint64_t* clock_dev,
                                    const uint8_t* done_dev, g2048_ntrestart_slot* snap_dev,
                                    uint16_t* valid_dev, uint8_t* top_dev, uint32_t* turn_dev,
                                    uint8_t* restored_out_dev, int64_t n, int device_id,
                                    void* stream);

/* Thread-local message of this library's last failure. */
G2048_API const char* g2048_ntrestart_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTRESTART_H */
