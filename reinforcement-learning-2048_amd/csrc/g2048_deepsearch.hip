// g2048_deepsearch.hip -- the wide expectimax over the n-tuple value networks for gfx950
// (libg2048_deepsearch.so): depths up to 5, one tree spread over many wavefronts.
//
// The search, the slot layout and the three steps are defined in include/g2048_deepsearch.h and
// checked bit for bit against tests/deepsearch_ref.py.  Every value is an int64.  No float, no
// atomics, no cooperative launch: the launches of one call are ordered by its stream.
//
//   k_expand   One wave per max node of level j, grid-stride.  Lane 16a + c slides the node's
//       board by a and writes the two slots (a 2 and a 4 at cell c) of level j + 1: the spawned
//       board, or the sentinel where a is illegal, c is occupied or the node is a sentinel itself.
//       All 128 slots of a node are written, so nothing below depends on the workspace's past.
//   k_sub      One wave per slot of the frontier (two slots per wave at sub = 1), grid-stride:
//       Vmax(board, sub).  The lane layout, the chance node and the leaves are k_search's
//       (g2048_ntsearch_dev.hpp: vmax, vafter, row_sum, best_move and the leaf policy), so one
//       source serves the flat and the staged table; what is this kernel's is where the board
//       comes from and what is kept (the largest value, 0 without a legal move).  A sentinel costs
//       its wave one 16-byte load and a wave-uniform branch; its Vmax is never read.
//   k_backup   One wave per max node, lane 16a + c as at k_search's root: the lane reads the Vmax
//       of its two slots, the 16 lanes of a move sum by shuffles, one floor_quot finishes the
//       chance node and (gain << F), recomputed from the node's own board, is added.  Below
//       level 0 the node keeps the maximum; at level 0 the four values and the action go out.
//   top_plies = 0 is g2048_ntsearch_dev.hpp's search_launch on the roots, unchanged.
//
// Every slot index is an int64: level 2 of n boards has 16 384 n slots.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_deepsearch.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntsearch_dev.hpp"
#include "g2048_stageleaf_dev.hpp"

#ifndef G2048_DEEPSEARCH_LEAF_TUPLES
#define G2048_DEEPSEARCH_LEAF_TUPLES 2  // tuples per burst of 8 gathers each
#endif

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int64_t FAN = 128;            // slots of level j + 1 per slot of level j
constexpr int64_t SLOT_BYTES = 16 + 8;  // a board and its Vmax
constexpr uint32_t NO_BOARD = 0xFFFFFFFFu;

__device__ __forceinline__ bool is_sentinel(const Board& b) { return (b.r0 & 0xFFu) == 0xFFu; }

// the wave's index and the number of waves of the grid
__device__ __forceinline__ int64_t first_wave() {
    return (int64_t)blockIdx.x * SEARCH_WAVES + (threadIdx.x >> 6);
}
__device__ __forceinline__ int64_t wave_stride() { return (int64_t)gridDim.x * SEARCH_WAVES; }

static __global__ __launch_bounds__(SEARCH_BLOCK) void k_expand(
    const uint4* __restrict__ nodes, int64_t n_nodes, uint4* __restrict__ slots) {
    const uint32_t lane = threadIdx.x & 63u, a = lane >> 4, c = lane & 15u;
    for (int64_t q = first_wave(); q < n_nodes; q += wave_stride()) {
        const Board b = load_board(nodes, q);
        Board s = b;
        apply_move(s, a);
        const bool put = !is_sentinel(b) && ((legal_mask(b) >> a) & 1u) && cell_empty(s, c);
        uint4* out = slots + q * FAN + a * 32u + c;
#pragma unroll
        for (uint32_t e = 1; e <= 2u; ++e) {
            Board child = s;
            set_cell(child, c, e);
            out[(e - 1u) * 16u] = put ? make_uint4(child.r0, child.r1, child.r2, child.r3)
                                      : make_uint4(NO_BOARD, NO_BOARD, NO_BOARD, NO_BOARD);
        }
    }
}

// The by-value struct comes last, as in k_search: the arguments in front of it arrive in SGPRs.
template <int SUB, int NT, class Leaf>
static __global__ __launch_bounds__(SEARCH_BLOCK) void k_sub(
    const int32_t* __restrict__ lut, const uint4* __restrict__ slots, int64_t n_slots,
    int64_t* __restrict__ vmax_out, Search<Leaf> p) {
    constexpr uint32_t PER = boards_per_wave(SUB), ROW = 16u / PER, SPAN = 4u * ROW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (lane / ROW) & 3u, c = lane & (ROW - 1u), head = lane & (SPAN - 1u);
    const int64_t units = (n_slots + PER - 1) / PER;
    for (int64_t u = first_wave(); u < units; u += wave_stride()) {
        const int64_t i = u * PER + lane / SPAN;
        const bool in = i < n_slots;
        Board b = load_board(slots, in ? i : n_slots - 1);
        const bool live = in && !is_sentinel(b);
        if (__all(!live)) continue;  // wave-uniform: every lane of a half holds the same board
        // a dead half keeps its lanes for the shuffles and the vote, on a board that gathers
        // nothing
        if (!live) b = Board{0u, 0u, 0u, 0u};
        const uint32_t legal = legal_mask(b);
        const bool ok = (legal >> a) & 1u;
        Board s = b;
        const uint32_t gain = apply_move(s, a);
        int64_t v;
        if constexpr (SUB == 1) {
            const int64_t sum = row_sum<ROW>(p.first_ply(lut, p.nt, s, nibbles(sym(s, c)), ok));
            v = ok ? ((int64_t)gain << F) + sum : INT64_MIN;
        } else {
            int64_t sum = 0;
            if (ok && cell_empty(s, c)) {
#pragma unroll 1
                for (uint32_t e = 1; e <= 2u; ++e) {
                    Board child = s;
                    set_cell(child, c, e);
                    sum += (int64_t)(e == 1u ? p.c2 : p.c4) * vmax<SUB - 1, NT>(lut, p, child);
                }
            }
            sum = row_sum<ROW>(sum);
            const int32_t ne = __popc(empties(s));
            v = ok ? ((int64_t)gain << F) + floor_quot(sum, p.W * max(ne, 1)) : INT64_MIN;
        }
        const Best m = best_move<ROW>(v, lane);
        if (live && head == 0u) vmax_out[i] = legal != 0u ? m.best : 0;
    }
}

// ROOT: the nodes are the caller's boards and the four values and the action go out; otherwise
// the nodes are slots (sentinels among them) and each keeps its Vmax.
template <bool ROOT>
static __global__ __launch_bounds__(SEARCH_BLOCK) void k_backup(
    const uint4* __restrict__ nodes, int64_t n_nodes, const int64_t* __restrict__ child_vmax,
    int64_t* __restrict__ vmax_out, int64_t* __restrict__ values, uint8_t* __restrict__ action,
    int32_t c2, int32_t c4, int32_t W) {
    const uint32_t lane = threadIdx.x & 63u, a = lane >> 4, c = lane & 15u;
    for (int64_t q = first_wave(); q < n_nodes; q += wave_stride()) {
        const Board b = load_board(nodes, q);
        if constexpr (!ROOT) {
            if (is_sentinel(b)) continue;  // wave-uniform
        }
        const uint32_t legal = legal_mask(b);
        const bool ok = (legal >> a) & 1u;
        Board s = b;
        const uint32_t gain = apply_move(s, a);
        int64_t sum = 0;
        if (ok && cell_empty(s, c)) {
            const int64_t* v = child_vmax + q * FAN + a * 32u + c;
            sum = (int64_t)c2 * v[0] + (int64_t)c4 * v[16];
        }
        sum = row_sum<16u>(sum);
        const int32_t ne = __popc(empties(s));
        const int64_t v = ok ? ((int64_t)gain << F) + floor_quot(sum, W * max(ne, 1)) : INT64_MIN;
        const Best m = best_move<16u>(v, lane);
        if constexpr (ROOT) {
            if (values != nullptr && lane < 4u)
                values[q * 4 + lane] =
                    lane == 0u ? m.q0 : lane == 1u ? m.q1 : lane == 2u ? m.q2 : m.q3;
            if (action != nullptr && lane == 0u) action[q] = (uint8_t)m.act;
        } else {
            if (lane == 0u) vmax_out[q] = legal != 0u ? m.best : 0;
        }
    }
}

thread_local std::string g_err;

// slots of levels 1 .. top of n boards
int64_t slots_of(int64_t n, int top) {
    return top == 0 ? 0 : top == 1 ? n * FAN : n * (FAN + FAN * FAN);
}

// a wave per unit up to 8 blocks per CU, the rest by grid stride (search_launch's grid)
dim3 wave_grid(int64_t units) {
    const int64_t blocks = (units + SEARCH_WAVES - 1) / SEARCH_WAVES;
    return dim3((uint32_t)(blocks < 2048 ? blocks : 2048));
}

// An entry point past check_common / check_staged.
template <class Leaf>
int deep_launch(const char* who, const Params& nt, const Leaf& leaf, const int32_t* lut_dev,
                const uint8_t* boards_dev, int64_t n, int depth, int top, uint32_t flags,
                int64_t* values, uint8_t* action, void* workspace, int64_t workspace_bytes,
                int device_id, void* stream) {
    constexpr int NT = G2048_DEEPSEARCH_LEAF_TUPLES;
    if (depth < 1 || depth > G2048_DEEPSEARCH_MAX_DEPTH)
        return refuse(g_err, "%s: depth = %d outside [1, %d]", who, depth,
                      G2048_DEEPSEARCH_MAX_DEPTH);
    if (top < 0 || top > G2048_DEEPSEARCH_MAX_TOP_PLIES)
        return refuse(g_err, "%s: top_plies = %d outside [0, %d]", who, top,
                      G2048_DEEPSEARCH_MAX_TOP_PLIES);
    const int sub = depth - top;
    if (sub < 1 || sub > G2048_DEEPSEARCH_MAX_SUB_DEPTH)
        return refuse(g_err, "%s: sub = depth - top_plies = %d outside [1, %d] (depth = %d)", who,
                      sub, G2048_DEEPSEARCH_MAX_SUB_DEPTH, depth);
    if ((flags & ~(uint32_t)G2048_P4_10) != 0u)
        return refuse(g_err, "%s: flags = 0x%x (only G2048_P4_10 is accepted)", who, flags);
    if (values == nullptr && action == nullptr)
        return refuse(g_err, "%s: both outputs are NULL", who);
    if (((uintptr_t)values & 7u) != 0)
        return refuse(g_err, "%s: values_out_dev must be 8-byte aligned", who);
    if (top == 0)
        return search_launch<NT>(g_err, who, G2048_DEEPSEARCH_MAX_SUB_DEPTH, nt, leaf, lut_dev,
                                 boards_dev, n, depth, flags, values, action, device_id, stream);
    const int64_t need = slots_of(n, top) * SLOT_BYTES;
    if (workspace == nullptr) return refuse(g_err, "%s: workspace_dev is NULL", who);
    if (((uintptr_t)workspace & 15u) != 0)
        return refuse(g_err, "%s: workspace_dev must be 16-byte aligned", who);
    if (workspace_bytes < need)
        return refuse(g_err, "%s: workspace_bytes = %lld is smaller than the %lld that n = %lld "
                      "and top_plies = %d need", who, (long long)workspace_bytes, (long long)need,
                      (long long)n, top);
    Search<Leaf> p;
    static_cast<Leaf&>(p) = leaf;
    p.nt = nt;
    p.W = (flags & G2048_P4_10) ? 10 : 2;
    p.c4 = 1;
    p.c2 = p.W - p.c4;

    // the boards of levels 1 .. top, then their Vmax: every part starts 16-byte aligned
    const int64_t n1 = n * FAN, n2 = top == 2 ? n1 * FAN : 0;
    uint4* const board1 = reinterpret_cast<uint4*>(workspace);
    uint4* const board2 = board1 + n1;
    int64_t* const vmax1 = reinterpret_cast<int64_t*>(board2 + n2);
    int64_t* const vmax2 = vmax1 + n1;
    const uint4* const roots = reinterpret_cast<const uint4*>(boards_dev);
    const uint4* const front = top == 2 ? board2 : board1;
    int64_t* const fv = top == 2 ? vmax2 : vmax1;
    const int64_t n_front = top == 2 ? n2 : n1;

    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(SEARCH_BLOCK);
    k_expand<<<wave_grid(n), block, 0, st>>>(roots, n, board1);
    if (top == 2) k_expand<<<wave_grid(n1), block, 0, st>>>(board1, n1, board2);
    const dim3 grid = wave_grid((n_front + boards_per_wave(sub) - 1) / boards_per_wave(sub));
    switch (sub) {
    case 1: k_sub<1, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, front, n_front, fv, p); break;
    case 2: k_sub<2, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, front, n_front, fv, p); break;
    default: k_sub<3, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, front, n_front, fv, p); break;
    }
    if (top == 2)
        k_backup<false><<<wave_grid(n1), block, 0, st>>>(board1, n1, vmax2, vmax1, nullptr, nullptr,
                                                         p.c2, p.c4, p.W);
    k_backup<true><<<wave_grid(n), block, 0, st>>>(roots, n, vmax1, nullptr, values, action, p.c2,
                                                   p.c4, p.W);
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // namespace

extern "C" {

const char* g2048_deepsearch_last_error(void) { return g_err.c_str(); }

int64_t g2048_deepsearch_workspace_bytes(int64_t n, int top_plies) {
    const char* who = "deepsearch_workspace_bytes";
    if (n < 1 || n > G2048_MAX_BOARDS)
        return refuse(g_err, "%s: n = %lld outside [1, G2048_MAX_BOARDS]", who, (long long)n);
    if (top_plies < 0 || top_plies > G2048_DEEPSEARCH_MAX_TOP_PLIES)
        return refuse(g_err, "%s: top_plies = %d outside [0, %d]", who, top_plies,
                      G2048_DEEPSEARCH_MAX_TOP_PLIES);
    return slots_of(n, top_plies) * SLOT_BYTES;
}

int g2048_deepsearch_expectimax(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                                const uint8_t* boards_dev, int64_t n, int depth, int top_plies,
                                uint32_t flags, int64_t* values_out_dev, uint8_t* action_out_dev,
                                void* workspace_dev, int64_t workspace_bytes, int device_id,
                                void* stream) {
    const char* who = "deepsearch_expectimax";
    const int rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    return deep_launch(who, make_params(*spec), FlatLeaf{}, lut_dev, boards_dev, n, depth,
                       top_plies, flags, values_out_dev, action_out_dev, workspace_dev,
                       workspace_bytes, device_id, stream);
}

int g2048_deepsearch_staged_expectimax(const g2048_ntuple_spec* spec,
                                       const g2048_ntstage_spec* stages, const int32_t* lut_dev,
                                       const uint8_t* boards_dev, int64_t n, int depth,
                                       int top_plies, uint32_t flags, int64_t* values_out_dev,
                                       uint8_t* action_out_dev, void* workspace_dev,
                                       int64_t workspace_bytes, int device_id, void* stream) {
    const char* who = "deepsearch_staged_expectimax";
    const int rc = check_staged(g_err, who, spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    return deep_launch(who, make_params(*spec), StagedLeaf{make_stage_params(*spec, *stages)},
                       lut_dev, boards_dev, n, depth, top_plies, flags, values_out_dev,
                       action_out_dev, workspace_dev, workspace_bytes, device_id, stream);
}

}  // extern "C"
