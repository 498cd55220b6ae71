// g2048_ntsearch_dev.hpp -- the expectimax tree walk over an n-tuple value network, shared by the
// search libraries: g2048_ntsearch.hip (one table), g2048_stagesearch.hip (a staged table) and
// g2048_deepsearch.hip (either, one tree over many waves).
// One copy, so the chance node, the tie rule and the grid-stride loop cannot drift.
//   device  the tree (vmax, vafter, leaf_value), the kernel (k_search) and the flat leaf (FlatLeaf)
//   host    everything of an entry point after the checks of its spec, table and boards
//           (search_launch)
// Header-only and internal to each library, as g2048_ntuple_dev.hpp: nothing here is exported.
// The staged leaf needs g2048_ntstage_dev.hpp and so lives in g2048_stageleaf_dev.hpp, not here:
// the flat library does not follow the stage header.  g2048_deepsearch.hip builds its own kernels
// on the same tree (vmax, vafter, the leaf policies) and launches k_search through search_launch.
//
// The search is defined in include/g2048_ntsearch.h; every value is an int64.  No float anywhere.
//
// Tree walk (the mapping of g2048_search.hip).  One wavefront per board, grid-stride over boards.
// Lane 16a + c owns first move a and spawn cell c: it slides the root by a and -- if a is legal
// and cell c of the slid board is empty -- evaluates Vmax of its two spawned boards (a 2 and a 4
// at c) depth - 1 player moves deep by a per-lane recursion whose depth is a template parameter
// (registers only: no stack, no LDS).  The 16 lanes of a move sum their weighted values by four
// xor-shuffles, one floor division finishes the chance node, the four root values are read from
// lanes 0 / 16 / 32 / 48.  Depth 1 has no chance node and only 4 leaves per board: there a wave
// takes two boards and the 8 lanes of a move split the leaf, lane 32s + 8a + g gathering
// symmetry g of after(board s, a) -- the layout of the policy kernels (g2048_ntuple_dev.hpp's
// policy_lane).  At every depth the greedy move is that header's best_move, with 16 or 8 lanes
// per move; the index helpers, the host plumbing and the argument checks are its as well.
//
// Leaves.  Below the root one lane owns a leaf, so it walks all 8 symmetries itself.  On the
// packed nibble word (nibble 4r + c = min(b[r][c], 15)) a row flip reverses the four 16-bit
// groups and a column flip reverses the nibbles inside each group, so one transpose (8 v_perm),
// two packs and a few perms / shifts give the 8 words; the spec's own cell lists then index all
// of them (g2048_ntuple_dev.hpp's entry).  The tuple count is a run-time, wave-uniform loop
// (one kernel per depth, not per (T, depth)): a tuple's six shifts are one scalar 8-byte load.
// Each trip of the loop issues the gathers of LEAF_TUPLES tuples x 8 symmetries before the first
// is used; that many stay in flight per lane.  LEAF_TUPLES is each library's build-time knob and
// arrives here as a template argument.
//
// What a table is to the tree is its leaf policy, a struct with three members and nothing else:
//   at(s)                       what the lane has to know about the leaf s before it gathers
//   burst<NT>(lut, p, x, t0, at)   the sum of tuples t0 .. t0 + NT - 1 over the 8 packed
//                               symmetries x[g]: 8 NT gathers, all issued before the first is
//                               used (t0 is wave-uniform), settled
//   first_ply(lut, p, s, nib, ok)  the depth-1 lane's share of V(s): its T gathers at the packed
//                               symmetry nib (0 unless ok), before the sum over the move's lanes
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

namespace g2048 {
namespace nt {

// The kernels' by-value argument: the table's params, what the leaf policy carries, the chance
// weights.  The leaf policy is a base, so one without state (FlatLeaf) takes no room in the
// argument block, and it is the second base, so the params keep offset 0.
struct SearchTable {
    Params nt;
};
template <class Leaf>
struct Search : SearchTable, Leaf {
    int32_t c2, c4, W;  // chance weights of a 2 (W - w4) and of a 4 (w4); W
};

// The leaf of the single table: nothing to know about a leaf, nothing to settle.
struct FlatLeaf {
    struct At {};
    __device__ __forceinline__ At at(const Board&) const { return At{}; }

    template <int NT>
    __device__ __forceinline__ int64_t burst(const int32_t* __restrict__ lut, const Params& p,
                                             const uint64_t (&x)[8], int t0, At) const {
        int32_t v[NT][8];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int g = 0; g < 8; ++g) v[j][g] = lut[entry(p, x[g], t0 + j)];
        }
        int64_t sum = 0;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int g = 0; g < 8; ++g) sum += v[j][g];
        }
        return sum;
    }

    // policy_lane's layout: T loads in flight
    __device__ __forceinline__ int64_t first_ply(const int32_t* __restrict__ lut, const Params& p,
                                                 const Board&, uint64_t nib, bool ok) const {
        const int T = (int)p.n_tuples;
        int32_t e[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t) e[t] = (ok && t < T) ? lut[entry(p, nib, t)] : 0;
        int64_t sum = 0;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) sum += e[t];
        return sum;
    }
};

// bit 4r + c set iff cell (r, c) is empty
__device__ __forceinline__ uint32_t empties(const Board& b) {
    const uint32_t rows[4] = {b.r0, b.r1, b.r2, b.r3};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t z = z80(rows[r]) >> 7;  // bit 8c = cell (r, c) is empty
        m |= ((z & 1u) | ((z >> 7) & 2u) | ((z >> 14) & 4u) | ((z >> 21) & 8u)) << (4u * r);
    }
    return m;
}

__device__ __forceinline__ int64_t floor_quot(int64_t num, int32_t den) {  // den > 0
    const int64_t q = num / den;
    return q - (int64_t)(num % den < 0);
}

// the two halves of the packed board with their 16-bit groups swapped
__device__ __forceinline__ uint32_t swap_groups(uint32_t w) { return perm(w, w, 0x01000302u); }
// the four nibbles of each 16-bit group in reverse order
__device__ __forceinline__ uint32_t reverse_nibbles(uint32_t w) {
    const uint32_t x = ((w & 0x0F0F0F0Fu) << 4) | ((w >> 4) & 0x0F0F0F0Fu);
    return perm(x, x, 0x02030001u);  // the two bytes of each group swapped
}
// rows reversed: group r <- group 3 - r
__device__ __forceinline__ uint64_t flip_rows(uint64_t x) {
    return ((uint64_t)swap_groups((uint32_t)x) << 32) | swap_groups((uint32_t)(x >> 32));
}
// columns reversed: nibble c of every group <- nibble 3 - c
__device__ __forceinline__ uint64_t flip_cols(uint64_t x) {
    return ((uint64_t)reverse_nibbles((uint32_t)(x >> 32)) << 32) | reverse_nibbles((uint32_t)x);
}

// V(s), all 8 T gathers by one lane
template <int NT, class Leaf>
__device__ __forceinline__ int64_t leaf_value(const int32_t* __restrict__ lut,
                                              const Search<Leaf>& p, const Board& s) {
    const auto at = p.at(s);
    uint64_t x[8];  // x[g] = the packed g(s), g = 4 tr + 2 fc + fr
    x[0] = nibbles(s);
    x[4] = nibbles(transpose(s));
#pragma unroll
    for (int tr = 0; tr < 8; tr += 4) {
        x[tr + 1] = flip_rows(x[tr]);
        x[tr + 2] = flip_cols(x[tr]);
        x[tr + 3] = flip_cols(x[tr + 1]);
    }
    const int T = (int)p.nt.n_tuples;
    int64_t sum = 0;
    int t = 0;
    // whole bursts, then the tuples left over one at a time: no first load sits behind a test
#pragma unroll 1
    for (; t + NT <= T; t += NT) sum += p.template burst<NT>(lut, p.nt, x, t, at);
    if constexpr (NT > 1) {
#pragma unroll 1
        for (; t < T; ++t) sum += p.template burst<1>(lut, p.nt, x, t, at);
    }
    return sum;
}

template <int D, int NT, class Leaf>
__device__ __forceinline__ int64_t vmax(const int32_t* __restrict__ lut, const Search<Leaf>& p,
                                        const Board& b);

// Vafter(s, D): the leaf value at D == 0, else the chance node whose children are searched D more
// player moves deep
template <int D, int NT, class Leaf>
__device__ __forceinline__ int64_t vafter(const int32_t* __restrict__ lut, const Search<Leaf>& p,
                                          const Board& s) {
    if constexpr (D == 0) {
        return leaf_value<NT>(lut, p, s);
    } else {
        const uint32_t em = empties(s);
        int64_t sum = 0;
        // one loop over (cell, tile) pairs: bits 0-15 spawn a 2, bits 16-31 a 4
#pragma unroll 1
        for (uint32_t it = em | (em << 16); it != 0u; it &= it - 1u) {
            const uint32_t bit = __ffs(it) - 1u;
            const bool four = bit >= 16u;
            Board c = s;
            set_cell(c, bit & 15u, four ? 2u : 1u);
            sum += (int64_t)(four ? p.c4 : p.c2) * vmax<D, NT>(lut, p, c);
        }
        return floor_quot(sum, p.W * max((int32_t)__popc(em), 1));
    }
}

// Vmax(b, D), D >= 1
template <int D, int NT, class Leaf>
__device__ __forceinline__ int64_t vmax(const int32_t* __restrict__ lut, const Search<Leaf>& p,
                                        const Board& b) {
    const uint32_t legal = legal_mask(b);
    if (legal == 0u) return 0;
    int64_t best = INT64_MIN;
#pragma unroll 1
    for (uint32_t a = 0; a < 4u; ++a) {
        if (!((legal >> a) & 1u)) continue;
        Board s = b;
        const uint32_t g = apply_move(s, a);
        const int64_t v = ((int64_t)g << F) + vafter<D - 1, NT>(lut, p, s);
        best = v > best ? v : best;
    }
    return best;
}

// sum over the ROW (16 or 8) lanes of a move
template <uint32_t ROW>
__device__ __forceinline__ int64_t row_sum(int64_t v) {
    if constexpr (ROW == 16u) v += __shfl_xor(v, 8);
    return group_sum(v);
}

constexpr int SEARCH_BLOCK = 256, SEARCH_WAVES = SEARCH_BLOCK / 64;
// boards per wave: depth 1 has 4 leaves of 8 symmetries per board, so two boards fill a wave
// (g2048_ntuple_dev.hpp's policy_lane layout); deeper searches give a board the whole wave
constexpr int boards_per_wave(int depth) { return depth == 1 ? 2 : 1; }

// static, as every kernel template of the family's headers.  The by-value struct comes last: it
// is never preloaded, and the five arguments in front of it arrive in SGPRs.
template <int DEPTH, int NT, class Leaf>
static __global__ __launch_bounds__(SEARCH_BLOCK) void k_search(
    const int32_t* __restrict__ lut, const uint4* __restrict__ boards, int64_t n,
    int64_t* __restrict__ values, uint8_t* __restrict__ action, Search<Leaf> p) {
    constexpr uint32_t PER = boards_per_wave(DEPTH), ROW = 16u / PER, SPAN = 4u * ROW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (lane / ROW) & 3u, c = lane & (ROW - 1u), head = lane & (SPAN - 1u);
    const int64_t stride = (int64_t)gridDim.x * SEARCH_WAVES, units = (n + PER - 1) / PER;
    // every lane of a wave makes the same trips (u is the wave's), so a leaf's first_ply may vote
    for (int64_t u = (int64_t)blockIdx.x * SEARCH_WAVES + (threadIdx.x >> 6); u < units;
         u += stride) {
        const int64_t i = u * PER + lane / SPAN;
        const bool live = i < n;  // a dead half keeps its lanes for the shuffles and the vote
        const Board b = load_board(boards, live ? i : n - 1);
        const bool ok = (legal_mask(b) >> a) & 1u;
        Board s = b;
        const uint32_t gain = apply_move(s, a);
        int64_t v;
        if constexpr (DEPTH == 1) {
            // lane 8a + g gathers symmetry g of the leaf after(b, a)
            const int64_t sum = row_sum<ROW>(p.first_ply(lut, p.nt, s, nibbles(sym(s, c)), ok));
            v = ok ? ((int64_t)gain << F) + sum : INT64_MIN;
        } else {
            int64_t sum = 0;
            if (ok && cell_empty(s, c)) {
                // the 2 and the 4 through one copy of the recursion's code
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
        const Best m = best_move<ROW>(v, lane);
        if (!live) continue;
        if (values != nullptr && head < 4u)
            values[i * 4 + head] = head == 0u ? m.q0 : head == 1u ? m.q1 : head == 2u ? m.q2 : m.q3;
        if (action != nullptr && head == 0u) action[i] = (uint8_t)m.act;
    }
}

// An entry point past check_common / check_staged: the checks of depth, flags and outputs, the
// chance weights and the launch on the caller's device.  `g_err` is the library's message, which
// G_HIP writes; `max_depth` is the library's own G2048_*_MAX_DEPTH (k_search goes to depth 3).
template <int NT, class Leaf>
inline int search_launch(std::string& g_err, const char* who, int max_depth, const Params& nt,
                         const Leaf& leaf, const int32_t* lut_dev, const uint8_t* boards_dev,
                         int64_t n, int depth, uint32_t flags, int64_t* values, uint8_t* action,
                         int device_id, void* stream) {
    if (depth < 1 || depth > max_depth)
        return refuse(g_err, "%s: depth = %d outside [1, %d]", who, depth, max_depth);
    if ((flags & ~(uint32_t)G2048_P4_10) != 0u)
        return refuse(g_err, "%s: flags = 0x%x (only G2048_P4_10 is accepted)", who, flags);
    if (values == nullptr && action == nullptr)
        return refuse(g_err, "%s: both outputs are NULL", who);
    if (((uintptr_t)values & 7u) != 0)
        return refuse(g_err, "%s: values_out_dev must be 8-byte aligned", who);
    Search<Leaf> p;
    static_cast<Leaf&>(p) = leaf;
    p.nt = nt;
    p.W = (flags & G2048_P4_10) ? 10 : 2;
    p.c4 = 1;
    p.c2 = p.W - p.c4;

    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    // a wave per board (per two boards at depth 1) up to 8 blocks per CU, the rest by grid stride
    const int64_t per_block = SEARCH_WAVES * boards_per_wave(depth);
    const int64_t blocks = (n + per_block - 1) / per_block;
    const dim3 grid((uint32_t)(blocks < 2048 ? blocks : 2048)), block(SEARCH_BLOCK);
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    switch (depth) {
    case 1: k_search<1, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, boards, n, values, action, p); break;
    case 2: k_search<2, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, boards, n, values, action, p); break;
    default: k_search<3, NT, Leaf><<<grid, block, 0, st>>>(lut_dev, boards, n, values, action, p); break;
    }
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // namespace nt
}  // namespace g2048
