// g2048_ntplay.hip -- the on-device n-tuple player for gfx950 (libg2048_ntplay.so): K moves of the
// greedy or expectimax policy of an n-tuple table, played on an env's buffers in one launch.
//
// The rule is defined in include/g2048_ntplay.h and checked byte for byte against K iterations of
// the family's own policy call + g2048_env_step (tests/test_ntplay_gpu.py) and against
// tests/ntplay_ref.py.  Every value is an integer.  The table is only read.  No atomics, no LDS,
// no scratch, no allocation, no host sync: the two launches of a call are ordered by its stream.
//
//   k_play   k_search's root body (g2048_ntsearch_dev.hpp) inside a loop of K moves, on the same
//       lane layout: one board per wave at depths 2-3 (lane 16a + c owns first move a and spawn
//       cell c), two boards per wave at depth 1 (lane 32s + 8a + g gathers symmetry g of
//       after(board s, a)); vmax / vafter / row_sum / best_move / first_ply are the shared ones,
//       with FlatLeaf or StagedLeaf.  best_move hands the action to every lane of the board's
//       span, and every one of those lanes then applies the env's action-given step (restated
//       from g2048.hip's step_one) to its own register copy of the board, score, start and ep:
//       redundant and span-uniform, so nothing crosses lanes or memory between two moves.  The
//       Philox block of a move depends on the clock and the board id alone and is issued ahead of
//       the move's gathers; its key is the env seed, a kernel argument in SGPRs.
//       A wave loads everything it needs (boards, score, start, ep, fin, its group's clock word)
//       before its first store and stores once, after its last move, from one lane per board.  A
//       dead half-wave (odd n at depth 1) plays a copy of board n - 1 and stores nothing.  Under
//       G2048_NO_AUTORESET a wave whose boards are all terminal leaves the loop through the
//       closed form of the header (a wave vote, so the exit is wave-uniform).
//   k_tick   clock[g] += K.  k_play only reads the clocks: the waves of one 64-board group start
//       at different times, so the clocks move in a launch of their own, after it in the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_ntplay.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntsearch_dev.hpp"
#include "g2048_stageleaf_dev.hpp"

#ifndef G2048_NTPLAY_LEAF_TUPLES
#define G2048_NTPLAY_LEAF_TUPLES 2  // tuples per burst of 8 gathers each
#endif

namespace {

using namespace g2048;
using namespace g2048::nt;

// the env's buffers and what its step derives from the env's flags
struct PlayArgs {
    uint4* board;
    uint32_t* score;  // meta row 0
    uint32_t* start;  // meta row 1
    uint4* ep;
    const uint64_t* clock;
    uint8_t* fin;   // NULL: no latch
    uint4* result;
    uint64_t board_offset;
    uint32_t p4_thresh;
    uint32_t autoreset;
    int32_t k_steps;
};

// A 64-bit value as the wave's first lane holds it, in SGPRs.  readfirstlane returns an int: each
// half goes through uint32_t before widening, so a low word >= 2^31 cannot reach the high word.
__device__ __forceinline__ uint64_t first_lane_u64(uint64_t c) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)c);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(c >> 32));
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// The seed comes first: the leading scalar arguments arrive in SGPRs, where the Philox key has to
// be.  The by-value structs come last, as in k_search.
template <int DEPTH, int NT, class Leaf>
static __global__ __launch_bounds__(SEARCH_BLOCK) void k_play(
    const int32_t* __restrict__ lut, int64_t n, uint32_t seed_lo, uint32_t seed_hi, PlayArgs A,
    Search<Leaf> p) {
    constexpr uint32_t PER = boards_per_wave(DEPTH), ROW = 16u / PER, SPAN = 4u * ROW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (lane / ROW) & 3u, c = lane & (ROW - 1u), head = lane & (SPAN - 1u);
    // the wave's unit, formed through readfirstlane so that the test below is a scalar branch
    const int64_t u = (int64_t)blockIdx.x * SEARCH_WAVES +
                      ((uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6);
    if (u >= (n + PER - 1) / PER) return;  // whole waves: every vote below is a full wave's
    const int64_t i = u * PER + lane / SPAN;
    const bool live = i < n;  // a dead half keeps its lanes for the shuffles and the votes
    const int64_t bi = live ? i : n - 1;
    const uint64_t gid = A.board_offset + (uint64_t)bi;

    Board b = load_board(A.board, bi);
    uint32_t score = A.score[bi], start = A.start[bi];
    uint4 ep = A.ep[bi];
    bool fin = A.fin != nullptr ? A.fin[bi] != 0 : true;  // without a latch nothing is latched
    // boards 2u and 2u + 1 lie in one 64-board group, and so does the copy a dead half plays
    const uint64_t t0 = first_lane_u64(A.clock[bi >> 6]);

    uint4 res = make_uint4(0u, 0u, 0u, 0u);
    bool latched = false, ended = false;
    const int K = A.k_steps;
    for (int k = 0; k < K; ++k) {
        const uint64_t t = t0 + (uint64_t)k;
        // the step's block: it needs neither the gathers nor the action
        const uint4 w = draw(seed_lo, seed_hi, gid, DOMAIN_STEP, t);
        const uint32_t legal = legal_mask(b);
        if (!A.autoreset && __all(legal == 0u)) {
            // every board of the wave is terminal and stays so: the K - k steps left, at once
            const uint32_t mx = max_exp(b);
            if (!fin) {
                res = make_uint4(ep.x + 1u, score, (uint32_t)t + 1u - start, mx);
                fin = latched = true;
            }
            ep = make_uint4(ep.x + (uint32_t)(K - k), score, (uint32_t)(t0 + (uint64_t)K) - start,
                            mx);
            ended = true;
            break;
        }
        // ---- the policy: k_search's root body
        const bool ok = (legal >> a) & 1u;
        Board s = b;
        const uint32_t gain = apply_move(s, a);
        int64_t v;
        if constexpr (DEPTH == 1) {
            const int64_t sum = row_sum<ROW>(p.first_ply(lut, p.nt, s, nibbles(sym(s, c)), ok));
            v = ok ? ((int64_t)gain << F) + sum : INT64_MIN;
        } else {
            int64_t sum = 0;
            if (ok && cell_empty(s, c)) {
#pragma unroll 1
                for (uint32_t e = 1; e <= 2u; ++e) {
                    Board child = s;
                    set_cell(child, c, e);
                    sum += (int64_t)(e == 1u ? p.c2 : p.c4) * vmax<DEPTH - 1, NT>(lut, p, child);
                }
            }
            sum = row_sum<ROW>(sum);  // the chance node of move a
            const int32_t ne = __popc(empties(s));
            v = ok ? ((int64_t)gain << F) + floor_quot(sum, p.W * max(ne, 1)) : INT64_MIN;
        }
        const uint32_t act = best_move<ROW>(v, lane).act;
        // ---- the env's action-given step, on this lane's own copy
        const bool done = legal == 0u;
        if (!done && ((legal >> act) & 1u)) {
            score += apply_move(b, act);
            spawn(b, w.z, w.w, A.p4_thresh);
        }
        if (done) {
            const uint32_t t1 = (uint32_t)t + 1u;  // this terminal step included
            ep = make_uint4(ep.x + 1u, score, t1 - start, max_exp(b));
            ended = true;
            if (!fin) {
                res = ep;
                fin = latched = true;
            }
            if (A.autoreset) {
                b = fresh_board(w, A.p4_thresh);  // the step's own block
                score = 0u;
                start = t1;
            }
        }
    }
    if (!live || head != 0u) return;
    A.board[i] = make_uint4(b.r0, b.r1, b.r2, b.r3);
    A.score[i] = score;
    if (ended) {
        A.ep[i] = ep;
        if (A.autoreset) A.start[i] = start;
    }
    if (latched) {
        A.result[i] = res;
        A.fin[i] = 1;
    }
}

constexpr int TICK_BLOCK = 256;

static __global__ __launch_bounds__(TICK_BLOCK) void k_tick(uint64_t* __restrict__ clock,
                                                           int64_t groups, uint64_t k) {
    const int64_t g = (int64_t)blockIdx.x * TICK_BLOCK + threadIdx.x;
    if (g < groups) clock[g] += k;
}

thread_local std::string g_err;

inline uint32_t p4_thresh(uint32_t flags) {
    return (flags & G2048_P4_10) ? 429496730u : 2147483648u;  // round(p * 2^32)
}

// An entry point past check_common / check_staged.
template <class Leaf>
int play_launch(const char* who, const Params& nt, const Leaf& leaf, const int32_t* lut_dev,
                uint8_t* board, uint32_t* meta, uint32_t* ep, uint64_t* clock, int64_t n,
                uint64_t seed, uint64_t board_offset, uint32_t flags, int k_steps, int depth,
                uint8_t* fin, uint32_t* result, int device_id, void* stream) {
    constexpr int NT = G2048_NTPLAY_LEAF_TUPLES;
    if (meta == nullptr) return refuse(g_err, "%s: meta_dev is NULL", who);
    if (((uintptr_t)meta & 3u) != 0)
        return refuse(g_err, "%s: meta_dev must be 4-byte aligned", who);
    if (ep == nullptr) return refuse(g_err, "%s: ep_dev is NULL", who);
    if (((uintptr_t)ep & 15u) != 0) return refuse(g_err, "%s: ep_dev must be 16-byte aligned", who);
    if (clock == nullptr) return refuse(g_err, "%s: clock_dev is NULL", who);
    if (((uintptr_t)clock & 7u) != 0)
        return refuse(g_err, "%s: clock_dev must be 8-byte aligned", who);
    if (flags & ~(uint32_t)(G2048_P4_10 | G2048_EGREEDY_FIXED | G2048_NO_AUTORESET))
        return refuse(g_err, "%s: env_flags = 0x%x holds an unknown flag", who, flags);
    if (k_steps < 1 || k_steps > G2048_NTPLAY_MAX_STEPS)
        return refuse(g_err, "%s: k_steps = %d outside [1, %d]", who, k_steps,
                      G2048_NTPLAY_MAX_STEPS);
    if (depth < 1 || depth > G2048_NTPLAY_MAX_DEPTH)
        return refuse(g_err, "%s: depth = %d outside [1, %d]", who, depth, G2048_NTPLAY_MAX_DEPTH);
    if ((fin == nullptr) != (result == nullptr))
        return refuse(g_err, "%s: fin_dev and result_dev are given together or not at all", who);
    if (((uintptr_t)result & 15u) != 0)
        return refuse(g_err, "%s: result_dev must be 16-byte aligned", who);

    Search<Leaf> p;
    static_cast<Leaf&>(p) = leaf;
    p.nt = nt;
    p.W = (flags & G2048_P4_10) ? 10 : 2;
    p.c4 = 1;
    p.c2 = p.W - p.c4;
    PlayArgs A;
    A.board = reinterpret_cast<uint4*>(board);
    A.score = meta;
    A.start = meta + n;
    A.ep = reinterpret_cast<uint4*>(ep);
    A.clock = clock;
    A.fin = fin;
    A.result = reinterpret_cast<uint4*>(result);
    A.board_offset = board_offset;
    A.p4_thresh = p4_thresh(flags);
    A.autoreset = (flags & G2048_NO_AUTORESET) ? 0u : 1u;
    A.k_steps = k_steps;
    const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);

    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    // a wave per board (per two boards at depth 1): n <= G2048_MAX_BOARDS keeps the grid in 2^29
    const int64_t per_block = SEARCH_WAVES * boards_per_wave(depth);
    const dim3 grid((uint32_t)((n + per_block - 1) / per_block)), block(SEARCH_BLOCK);
    switch (depth) {
    case 1: k_play<1, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, n, seed_lo, seed_hi, A, p); break;
    case 2: k_play<2, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, n, seed_lo, seed_hi, A, p); break;
    default: k_play<3, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, n, seed_lo, seed_hi, A, p); break;
    }
    G_HIP(hipGetLastError());
    const int64_t groups = (n + G2048_CLOCK_GROUP - 1) / G2048_CLOCK_GROUP;
    k_tick<<<dim3((uint32_t)((groups + TICK_BLOCK - 1) / TICK_BLOCK)), dim3(TICK_BLOCK), 0, st>>>(
        clock, groups, (uint64_t)k_steps);
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // namespace

extern "C" {

const char* g2048_ntplay_last_error(void) { return g_err.c_str(); }

int g2048_ntplay_steps(const g2048_ntuple_spec* spec, const int32_t* lut_dev, uint8_t* board_dev,
                       uint32_t* meta_dev, uint32_t* ep_dev, uint64_t* clock_dev, int64_t n,
                       uint64_t seed, uint64_t board_offset, uint32_t env_flags, int k_steps,
                       int depth, uint8_t* fin_dev, uint32_t* result_dev, int device_id,
                       void* stream) {
    const char* who = "ntplay_steps";
    const int rc = check_common(g_err, who, spec, lut_dev, board_dev, n);
    if (rc != G2048_OK) return rc;
    return play_launch(who, make_params(*spec), FlatLeaf{}, lut_dev, board_dev, meta_dev, ep_dev,
                       clock_dev, n, seed, board_offset, env_flags, k_steps, depth, fin_dev,
                       result_dev, device_id, stream);
}

int g2048_ntplay_staged_steps(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                              const int32_t* lut_dev, uint8_t* board_dev, uint32_t* meta_dev,
                              uint32_t* ep_dev, uint64_t* clock_dev, int64_t n, uint64_t seed,
                              uint64_t board_offset, uint32_t env_flags, int k_steps, int depth,
                              uint8_t* fin_dev, uint32_t* result_dev, int device_id,
                              void* stream) {
    const char* who = "ntplay_staged_steps";
    const int rc = check_staged(g_err, who, spec, stages, lut_dev, board_dev, n);
    if (rc != G2048_OK) return rc;
    return play_launch(who, make_params(*spec), StagedLeaf{make_stage_params(*spec, *stages)},
                       lut_dev, board_dev, meta_dev, ep_dev, clock_dev, n, seed, board_offset,
                       env_flags, k_steps, depth, fin_dev, result_dev, device_id, stream);
}

}  // extern "C"
