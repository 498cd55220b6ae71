// g2048_stagesearch.hip -- expectimax search over the multi-stage n-tuple network for gfx950
// (libg2048_stagesearch.so).
//
// The search is defined in include/g2048_stagesearch.h: g2048_ntsearch.h's tree with
// g2048_ntstage.h's V at the leaves.  Every value is an int64 and the result is checked bit for
// bit against tests/stagesearch_ref.py.  No float anywhere.  The table is only read.
//
// Tree walk: that of g2048_ntsearch.hip, unchanged.  One wavefront per board, grid-stride over
// boards; lane 16a + c owns first move a and spawn cell c and evaluates Vmax of its two spawned
// boards by a per-lane recursion whose depth is a template parameter (registers only); the 16
// lanes of a move sum by xor-shuffles, one floor division finishes the chance node.  Depth 1 has
// no chance node: a wave takes two boards, lane 32s + 8a + g gathers symmetry g of
// after(board s, a) -- the layout of g2048_ntstage.hip's k_stage_policy.
//
// What is new is the leaf.
//   Stage   The lane that owns a leaf takes stage(leaf) from the leaf's own bytes
//       (g2048_ntstage_dev.hpp: the packed max and seven compares against the bounds bytes, which
//       ride in the params struct, wave-uniform) and adds stage * T * 16^m to every index of the
//       leaf; the sum is < 2^30.  The stage uses the true exponents, the index the clamped ones.
//   Fall-through   After a burst of LEAF_TUPLES x 8 gathers the values that came back UNSET are
//       read again one stage down, in rounds r = 1 .. stage.  A round issues all its re-reads
//       before the first is used and the loop ends as soon as the lane holds no UNSET; what is
//       UNSET at stage 0 is 0.  Below the root every lane walks its own subtree, so leaves run
//       under divergence and the loop's exit is per lane (the learner's is a wave vote).  A
//       round recomputes its indices from the eight packed words x[g], which are live anyway: no
//       index is held across the rounds.  UNSET is INT32_MIN, so "the burst holds an UNSET" is
//       one test of the smallest of its values (v_min3_i32): a burst without UNSET pays for
//       that alone and skips the rounds and the UNSET -> 0 selects.
//   Depth 1   All lanes of a wave reach the leaf together, so there the rounds are whole-wave
//       rounds ended by a vote, as in k_stage_policy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stagesearch.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"

#ifndef G2048_STAGESEARCH_LEAF_TUPLES
#define G2048_STAGESEARCH_LEAF_TUPLES 2
#endif

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int LEAF_TUPLES = G2048_STAGESEARCH_LEAF_TUPLES;  // tuples per burst of 8 gathers each

struct Search {
    Params nt;
    StageParams sp;
    int32_t c2, c4, W;  // chance weights of a 2 (W - w4) and of a 4 (w4); W
};

// stage(b), kept below S for any bytes: a board outside the domain (an exponent byte that
// reaches the 255 of an unused bound) must not index past the table
__device__ __forceinline__ uint32_t leaf_stage(const Board& b, const StageParams& sp) {
    return min(stage_of(b, sp), sp.n_stages - 1u);
}

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

// the smallest of a burst's values: UNSET is INT32_MIN, so the burst holds an UNSET iff this is
// UNSET (8 NT / 2 v_min3_i32 instead of a compare per value)
template <int NT>
__device__ __forceinline__ int32_t smallest(const int32_t (&v)[NT][8]) {
    int32_t lo = v[0][0];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int g = 0; g < 8; ++g) lo = min(lo, v[j][g]);
    }
    return lo;
}

// the sum of val(st, t, .) for tuples t0 .. t0 + NT - 1 over the 8 packed symmetries x[g]: 8 NT
// gathers at the leaf's stage (top = st * stride), all issued before the first is used, then --
// only in a lane whose burst holds an UNSET -- the fall-through rounds of that lane (t0 is
// wave-uniform, st and the rounds are not)
template <int NT>
__device__ __forceinline__ int64_t burst(const int32_t* __restrict__ lut, const Search& p,
                                         const uint64_t (&x)[8], int t0, uint32_t st,
                                         uint32_t top) {
    int32_t v[NT][8];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int g = 0; g < 8; ++g) v[j][g] = lut[top + entry(p.nt, x[g], t0 + j)];
    }
    if (smallest<NT>(v) == UNSET) {
#pragma unroll 1
        for (uint32_t r = 1; r <= st; ++r) {
            const uint32_t base = top - r * p.sp.stride;  // r <= st: never below stage 0
            int32_t w[NT][8];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
#pragma unroll
                for (int g = 0; g < 8; ++g)
                    w[j][g] = v[j][g] == UNSET ? lut[base + entry(p.nt, x[g], t0 + j)] : v[j][g];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
#pragma unroll
                for (int g = 0; g < 8; ++g) v[j][g] = w[j][g];
            }
            if (smallest<NT>(v) != UNSET) break;
        }
        // what is UNSET at stage 0 is 0
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int g = 0; g < 8; ++g) v[j][g] = v[j][g] == UNSET ? 0 : v[j][g];
        }
    }
    int64_t sum = 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int g = 0; g < 8; ++g) sum += v[j][g];
    }
    return sum;
}

// V(s) at s's own stage, all 8 T gathers and their fall-through by one lane
__device__ __forceinline__ int64_t leaf_value(const int32_t* __restrict__ lut, const Search& p,
                                              const Board& s) {
    const uint32_t st = leaf_stage(s, p.sp);
    const uint32_t top = st * p.sp.stride;
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
    // whole bursts, then the tuples left over one at a time: no first-round load sits behind a test
#pragma unroll 1
    for (; t + LEAF_TUPLES <= T; t += LEAF_TUPLES) sum += burst<LEAF_TUPLES>(lut, p, x, t, st, top);
    if constexpr (LEAF_TUPLES > 1) {
#pragma unroll 1
        for (; t < T; ++t) sum += burst<1>(lut, p, x, t, st, top);
    }
    return sum;
}

template <int D>
__device__ __forceinline__ int64_t vmax(const int32_t* __restrict__ lut, const Search& p,
                                        const Board& b);

// Vafter(s, D): the leaf value at D == 0, else the chance node whose children are searched D more
// player moves deep
template <int D>
__device__ __forceinline__ int64_t vafter(const int32_t* __restrict__ lut, const Search& p,
                                          const Board& s) {
    if constexpr (D == 0) {
        return leaf_value(lut, p, s);
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
            sum += (int64_t)(four ? p.c4 : p.c2) * vmax<D>(lut, p, c);
        }
        return floor_quot(sum, p.W * max((int32_t)__popc(em), 1));
    }
}

// Vmax(b, D), D >= 1
template <int D>
__device__ __forceinline__ int64_t vmax(const int32_t* __restrict__ lut, const Search& p,
                                        const Board& b) {
    const uint32_t legal = legal_mask(b);
    if (legal == 0u) return 0;
    int64_t best = INT64_MIN;
#pragma unroll 1
    for (uint32_t a = 0; a < 4u; ++a) {
        if (!((legal >> a) & 1u)) continue;
        Board s = b;
        const uint32_t g = apply_move(s, a);
        const int64_t v = ((int64_t)g << F) + vafter<D - 1>(lut, p, s);
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

constexpr int BLOCK = 256, WAVES = BLOCK / 64;
// boards per wave: depth 1 has 4 leaves of 8 symmetries per board, so two boards fill a wave
// (g2048_ntuple_dev.hpp's policy_lane layout); deeper searches give a board the whole wave
constexpr int boards_per_wave(int depth) { return depth == 1 ? 2 : 1; }

template <int DEPTH>
__global__ __launch_bounds__(BLOCK) void k_stagesearch(const int32_t* __restrict__ lut,
                                                       const uint4* __restrict__ boards,
                                                       int64_t n, int64_t* __restrict__ values,
                                                       uint8_t* __restrict__ action, Search p) {
    constexpr uint32_t PER = boards_per_wave(DEPTH), ROW = 16u / PER, SPAN = 4u * ROW;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (lane / ROW) & 3u, c = lane & (ROW - 1u), head = lane & (SPAN - 1u);
    const int64_t stride = (int64_t)gridDim.x * WAVES, units = (n + PER - 1) / PER;
    // every lane of a wave makes the same trips (u is the wave's), so the vote below is whole
    for (int64_t u = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); u < units; u += stride) {
        const int64_t i = u * PER + lane / SPAN;
        const bool live = i < n;  // a dead half keeps its lanes for the shuffles and the vote
        const Board b = load_board(boards, live ? i : n - 1);
        const bool ok = (legal_mask(b) >> a) & 1u;
        Board s = b;
        const uint32_t gain = apply_move(s, a);
        int64_t v;
        if constexpr (DEPTH == 1) {
            // k_stage_policy's lane: 8a + g gathers symmetry g of the leaf after(b, a) at that
            // afterstate's stage, T loads in flight; the fall-through in whole-wave rounds
            const uint64_t nib = nibbles(sym(s, c));
            const int T = (int)p.nt.n_tuples;
            const uint32_t st = leaf_stage(s, p.sp);
            const uint32_t top = st * p.sp.stride;
            // a lane that gathers nothing holds 0, never UNSET: it asks for no round.  The
            // index sits behind the wave-uniform t < T with its load (T indices, not MAXT).
            uint32_t e[MAXT];
            int32_t q[MAXT];
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                e[t] = 0u, q[t] = 0;
                if (t < T) {
                    e[t] = top + entry(p.nt, nib, t);
                    q[t] = ok ? lut[e[t]] : 0;
                }
            }
            for (uint32_t r = 1; r < p.sp.n_stages; ++r) {
                bool need = false;
#pragma unroll
                for (int t = 0; t < MAXT; ++t) need |= q[t] == UNSET && st >= r;
                if (!__any(need)) break;
                const uint32_t down = r * p.sp.stride;
                int32_t w[MAXT];
#pragma unroll
                for (int t = 0; t < MAXT; ++t)
                    w[t] = (q[t] == UNSET && st >= r) ? lut[e[t] - down] : q[t];
#pragma unroll
                for (int t = 0; t < MAXT; ++t) q[t] = w[t];
            }
            int64_t sum = 0;
#pragma unroll
            for (int t = 0; t < MAXT; ++t) sum += q[t] == UNSET ? 0 : q[t];
            sum = row_sum<ROW>(sum);
            v = ok ? ((int64_t)gain << F) + sum : INT64_MIN;
        } else {
            int64_t sum = 0;
            if (ok && cell_empty(s, c)) {
                // the 2 and the 4 through one copy of the recursion's code
#pragma unroll 1
                for (uint32_t e = 1; e <= 2u; ++e) {
                    Board child = s;
                    set_cell(child, c, e);
                    sum += (int64_t)(e == 1u ? p.c2 : p.c4) * vmax<DEPTH - 1>(lut, p, child);
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

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_stagesearch_last_error(void) { return g_err.c_str(); }

int g2048_stagesearch_expectimax(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                                 const int32_t* lut_dev, const uint8_t* boards_dev, int64_t n,
                                 int depth, uint32_t flags, int64_t* values_out_dev,
                                 uint8_t* action_out_dev, int device_id, void* stream) {
    const char* who = "stagesearch_expectimax";
    int rc = check_spec(g_err, who, spec);
    if (rc != G2048_OK) return rc;
    rc = check_stages(g_err, who, stages);
    if (rc != G2048_OK) return rc;
    rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (depth < 1 || depth > G2048_STAGESEARCH_MAX_DEPTH)
        return refuse(g_err, "%s: depth = %d outside [1, %d]", who, depth,
                      G2048_STAGESEARCH_MAX_DEPTH);
    if ((flags & ~(uint32_t)G2048_P4_10) != 0u)
        return refuse(g_err, "%s: flags = 0x%x (only G2048_P4_10 is accepted)", who, flags);
    if (values_out_dev == nullptr && action_out_dev == nullptr)
        return refuse(g_err, "%s: both outputs are NULL", who);
    if (((uintptr_t)values_out_dev & 7u) != 0)
        return refuse(g_err, "%s: values_out_dev must be 8-byte aligned", who);
    Search p;
    p.nt = make_params(*spec);
    p.sp = make_stage_params(*spec, *stages);
    p.W = (flags & G2048_P4_10) ? 10 : 2;
    p.c4 = 1;
    p.c2 = p.W - p.c4;

    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    // a wave per board (per two boards at depth 1) up to 8 blocks per CU, the rest by grid stride
    const int64_t per_block = WAVES * boards_per_wave(depth);
    const int64_t blocks = (n + per_block - 1) / per_block;
    const dim3 grid((uint32_t)(blocks < 2048 ? blocks : 2048)), block(BLOCK);
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    switch (depth) {
    case 1: k_stagesearch<1><<<grid, block, 0, st>>>(lut_dev, boards, n, values_out_dev, action_out_dev, p); break;
    case 2: k_stagesearch<2><<<grid, block, 0, st>>>(lut_dev, boards, n, values_out_dev, action_out_dev, p); break;
    default: k_stagesearch<3><<<grid, block, 0, st>>>(lut_dev, boards, n, values_out_dev, action_out_dev, p); break;
    }
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
