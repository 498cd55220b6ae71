// g2048_ntuple_dev.hpp -- the base internal header of the n-tuple family: what every library that
// reads the table of include/g2048_ntuple.h shares.  The narrower shared headers build on it:
// g2048_ntstage_dev.hpp (the stage rule), g2048_ntmean_dev.hpp (the batch-mean step) and
// g2048_ntsearch_dev.hpp (the expectimax tree walk).
//   device  board -> table indices (include/g2048_ntuple.h: symmetries, the clamp to 15, idx);
//           the afterstate policy's lane layout 32s + 8a + g (policy_lane), the sum over a group
//           (group_sum), the argmax over the four moves (best_move), err and delta (td_error);
//           the flat policy kernel itself (k_policy: act, and the first launch of every flat TD
//           step); the temporal-coherence rate (tc_rate); the update kernels' LDS merge table
//           (clear_keys, claim_slot) and their common tail (commit_prev); the ring position of
//           the two ring libraries (Ring, load_ring, plane_back).  The update kernels' gathers
//           and the payload of the merge table stay in the .hip files.
//   host    the error writer (refuse), G_HIP, DeviceGuard, DISPATCH_T, grid_for, and the
//           validation of a spec, of the arguments every device entry point has and of those
//           the learning steps share (check_spec, check_common, check_td_args), of a device
//           pointer (check_ptr), of (E, A) in front of the rate (checked_rate) and of the
//           batch-mean step's acc and ea (table_bytes, check_acc, check_ea).
// Header-only and internal to each library: nothing here is exported, and the libraries do not
// link against each other.  Each .hip keeps its own thread_local g_err, which G_HIP writes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/g2048_ntuple.h"
#include "g2048_board.hpp"

namespace g2048 {
namespace nt {

constexpr int MAXT = G2048_NTUPLE_MAX_TUPLES, MAXM = G2048_NTUPLE_MAX_CELLS;
constexpr int F = G2048_NTUPLE_FRAC_BITS;

struct Params {
    uint32_t entries;   // 16^m
    uint32_t n_tuples;  // T
    // byte k of sh[t] = 4 * cell(t, k): the nibble's bit position in the packed board (0 past
    // the tuple's m cells).  One 8-byte word per tuple, so a wave-uniform run-time t is one
    // scalar load and the shifts stay scalar operands.
    uint64_t sh[MAXT];
};

// g(b) of the header: transpose if g & 4, then flip the columns if g & 2 and the rows if g & 1
__device__ __forceinline__ Board sym(const Board& b, uint32_t g) {
    const Board t = transpose(b);
    const bool tr = (g & 4u) != 0u, fc = (g & 2u) != 0u, fr = (g & 1u) != 0u;
    const uint32_t x0 = tr ? t.r0 : b.r0, x1 = tr ? t.r1 : b.r1;
    const uint32_t x2 = tr ? t.r2 : b.r2, x3 = tr ? t.r3 : b.r3;
    const uint32_t y0 = fr ? x3 : x0, y1 = fr ? x2 : x1, y2 = fr ? x1 : x2, y3 = fr ? x0 : x3;
    constexpr uint32_t REV = 0x00010203u;  // byte c <- byte 3 - c
    Board o;
    o.r0 = fc ? perm(y0, y0, REV) : y0;
    o.r1 = fc ? perm(y1, y1, REV) : y1;
    o.r2 = fc ? perm(y2, y2, REV) : y2;
    o.r3 = fc ? perm(y3, y3, REV) : y3;
    return o;
}

// four exponent bytes (< 128) -> four nibbles min(e, 15), byte c at bits 4c
__device__ __forceinline__ uint32_t pack_row(uint32_t w) {
    const uint32_t big = (w + 0x70707070u) & K80;  // e + 112 >= 128 iff e >= 16
    const uint32_t c = bsel(expand80(big), 0x0F0F0F0Fu, w);
    const uint32_t x = c | (c >> 4);
    return (x & 0xFFu) | ((x >> 8) & 0xFF00u);
}

// nibble 4r + c = min(b[r][c], 15)
__device__ __forceinline__ uint64_t nibbles(const Board& b) {
    const uint32_t lo = pack_row(b.r0) | (pack_row(b.r1) << 16);
    const uint32_t hi = pack_row(b.r2) | (pack_row(b.r3) << 16);
    return ((uint64_t)hi << 32) | lo;
}

// t * 16^m + idx of tuple t on the packed board; < T * 16^m <= 2^27
__device__ __forceinline__ uint32_t entry(const Params& p, uint64_t nib, int t) {
    // all six positions, branch-free: sh is 0 past the tuple's m cells and the mask drops them
    const uint64_t sh = p.sh[t];
    uint32_t idx = 0;
#pragma unroll
    for (int k = 0; k < MAXM; ++k)
        idx |= ((uint32_t)(nib >> ((uint32_t)(sh >> (8 * k)) & 63u)) & 15u) << (4 * k);
    return (uint32_t)t * p.entries + (idx & (p.entries - 1u));
}

__device__ __forceinline__ Board load_board(const uint4* p, int64_t i) {
    const uint4 w = p[i];
    return Board{w.x, w.y, w.z, w.w};
}

// sum over the 8 lanes of a group
__device__ __forceinline__ int64_t group_sum(int64_t v) {
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// ------------------------------------------------------------------ device: afterstate policy
// The policy kernels' lane: 2 boards per wave, lane 32s + 8a + g holds after(board s, a) under
// symmetry g.  A dead half-wave (i >= n) keeps its lanes for the shuffles and reads board n - 1.
struct PolicyLane {
    int64_t i, bi;       // the board; the board read (bi = i where live)
    uint32_t lane, a, g;
    bool live, ok;       // i < n; move a is legal
    uint32_t legal, gain;
    Board b, s;          // the board and after(b, a)
    uint64_t nib;        // nibbles(g(s))
};

template <int BLOCK>
__device__ __forceinline__ PolicyLane policy_lane(const uint4* __restrict__ boards, int64_t n) {
    PolicyLane l;
    l.lane = threadIdx.x & 63u;
    const int64_t wave = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    l.i = wave * 2 + (l.lane >> 5);
    l.a = (l.lane >> 3) & 3u;
    l.g = l.lane & 7u;
    l.live = l.i < n;
    l.bi = l.live ? l.i : n - 1;
    l.b = load_board(boards, l.bi);
    l.legal = legal_mask(l.b);
    l.ok = ((l.legal >> l.a) & 1u) != 0u;
    l.s = l.b;
    l.gain = apply_move(l.s, l.a);
    l.nib = nibbles(sym(l.s, l.g));
    return l;
}

// The four moves' values and the greedy move, from the value q of this lane's move.  A move has
// ROW lanes (8: two boards per wave, 16: one), move a's value is read from the first of them.
// The smallest a with the largest q wins; an illegal move holds INT64_MIN and a legal move's q is
// far above it, so with no legal move the action stays 0.
struct Best {
    int64_t q0, q1, q2, q3, best;
    uint32_t act;
};

template <uint32_t ROW>
__device__ __forceinline__ Best best_move(int64_t q, uint32_t lane) {
    const uint32_t base = lane & ~(4u * ROW - 1u);
    Best m;
    m.q0 = __shfl(q, base), m.q1 = __shfl(q, base + ROW);
    m.q2 = __shfl(q, base + 2u * ROW), m.q3 = __shfl(q, base + 3u * ROW);
    m.act = 0;
    m.best = m.q0;
    if (m.q1 > m.best) { m.act = 1; m.best = m.q1; }
    if (m.q2 > m.best) { m.act = 2; m.best = m.q2; }
    if (m.q3 > m.best) { m.act = 3; m.best = m.q3; }
    return m;
}

// err and delta of the learning steps: the target is the best q (0 on a terminal board), and a
// board without a previous afterstate learns nothing
struct TdError {
    int64_t err;
    int32_t delta;
};

__device__ __forceinline__ TdError td_error(int64_t best, int64_t psum, bool hp, uint32_t legal,
                                            int32_t lr_num, int32_t lr_shift) {
    const int64_t target = legal != 0u ? best : 0;
    const int64_t err = hp ? target - psum : 0;
    return TdError{err, (int32_t)((err * (int64_t)lr_num) >> lr_shift)};
}

// The policy kernel: 2 boards per wave, 8 per block of POLICY_BLOCK threads.  A lane's T gathers
// are all issued before the first is used.  With TD (the first launch of a TD step) the groups
// a == 0 also gather V(prev) in the same burst, and the launch writes action, delta and err only:
// q_out and after_out are not looked at, action_out is not null.  Only reads lut.  The TD step's
// arguments come first, act's two further outputs last: the leading ones arrive preloaded in
// SGPRs, and the TD launch's argument block is laid out as if the last two were not there.
// static, as every kernel template of the family's headers: each library has its own copy, as
// it had of the kernels in its unnamed namespace, and exports no kernel handle.
constexpr int POLICY_BLOCK = 256;

template <int T, bool TD>
static __global__ __launch_bounds__(POLICY_BLOCK) void k_policy(
    const int32_t* __restrict__ lut, const uint4* __restrict__ boards, int64_t n,
    uint8_t* __restrict__ action_out, const uint4* __restrict__ prev,
    const uint8_t* __restrict__ has_prev, int32_t lr_num, int32_t lr_shift,
    int32_t* __restrict__ delta_out, int64_t* __restrict__ err_out, Params p,
    int64_t* __restrict__ q_out, uint4* __restrict__ after_out) {
    const PolicyLane l = policy_lane<POLICY_BLOCK>(boards, n);
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[entry(p, l.nib, t)] : 0;
    bool hp = false;
    if constexpr (TD) {
        hp = has_prev[l.bi] != 0;
        const uint64_t pnib = nibbles(sym(load_board(prev, l.bi), l.g));
#pragma unroll
        for (int t = 0; t < T; ++t) pv[t] = (hp && l.a == 0u) ? lut[entry(p, pnib, t)] : 0;
    }
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const Best m = best_move<8>(l.ok ? ((int64_t)l.gain << F) + sum : INT64_MIN, l.lane);
    if constexpr (TD) {
#pragma unroll
        for (int t = 0; t < T; ++t) psum += pv[t];
        psum = group_sum(psum);  // V(prev) in the group a == 0
    }
    if (!l.live) return;
    if constexpr (TD) {
        if ((l.lane & 31u) == 0u) {
            const TdError td = td_error(m.best, psum, hp, l.legal, lr_num, lr_shift);
            action_out[l.i] = (uint8_t)m.act;
            delta_out[l.i] = td.delta;
            if (err_out != nullptr) err_out[l.i] = td.err;
        }
    } else {
        if (q_out != nullptr && (l.lane & 31u) < 4u) {
            const uint32_t k = l.lane & 3u;
            q_out[l.i * 4 + k] = k == 0u ? m.q0 : k == 1u ? m.q1 : k == 2u ? m.q2 : m.q3;
        }
        if (action_out != nullptr && (l.lane & 31u) == 0u) action_out[l.i] = (uint8_t)m.act;
        // the lane (a == action, g == 0) holds after(b, action); with no legal move after = b
        if (after_out != nullptr && l.a == m.act && l.g == 0u) {
            const Board o = l.legal != 0u ? l.s : l.b;
            after_out[l.i] = make_uint4(o.r0, o.r1, o.r2, o.r3);
        }
    }
}

// ------------------------------------------------------------------ device: temporal coherence
// rate(E, A) of include/g2048_nttc.h, g2048_ntmeantc.h and g2048_stagemeantc.h with RATE_BITS
// fraction bits: each library passes its own header's constant.  In the domain
// (|E| <= A < 2^62) both shifted operands are below 2^16 and the divisor is at least 1: a 32-bit
// unsigned division.
template <int RATE_BITS>
__host__ __device__ __forceinline__ uint32_t tc_rate(int64_t E, int64_t A) {
    if (A == 0) return 1u << RATE_BITS;
    const uint64_t a = (uint64_t)A, e = E < 0 ? 0ull - (uint64_t)E : (uint64_t)E;
    const int bits = 64 - __builtin_clzll(a);
    const int s = bits > RATE_BITS ? bits - RATE_BITS : 0;
    const uint32_t num = (uint32_t)(e >> s) << RATE_BITS, den = (uint32_t)(a >> s);
    return num / den;
}

// ------------------------------------------------------------------ device: update kernels
// The LDS merge table in front of the atomics: the entry index is the key of an open-addressed
// table of 2^SLOT_BITS slots, linear probing.  Each kernel keeps its payload arrays beside `keys`
// and adds into the slot it claimed; after PROBES slots taken by other keys the add goes straight
// to memory.
constexpr uint32_t PROBES = 4;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;  // entry indices are < 2^27
// slots are < 2^13; that it equals NO_KEY is a coincidence, the two are never compared
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr uint32_t HASH_MUL = 0x9E3779B1u;  // 2^32 / golden ratio (Fibonacci hashing)

// every slot free; a block of THREADS threads (the caller's barrier follows)
template <int SLOT_BITS, int THREADS>
__device__ __forceinline__ void clear_keys(uint32_t* keys) {
    for (uint32_t s = threadIdx.x; s < (1u << SLOT_BITS); s += THREADS) keys[s] = NO_KEY;
}

// the slot that holds key e, claimed if it was free; NO_SLOT after PROBES slots of other keys
template <int SLOT_BITS>
__device__ __forceinline__ uint32_t claim_slot(uint32_t* keys, uint32_t e) {
    const uint32_t home = (e * HASH_MUL) >> (32 - SLOT_BITS);
#pragma unroll
    for (uint32_t probe = 0; probe < PROBES; ++probe) {
        const uint32_t slot = (home + probe) & ((1u << SLOT_BITS) - 1u);
        const uint32_t old = atomicCAS(&keys[slot], NO_KEY, e);
        if (old == NO_KEY || old == e) return slot;
    }
    return NO_SLOT;
}

// The update kernels' tail, for lane 0 of a live board's group: prev <- after(board, action) and
// has_prev <- 1, or has_prev <- 0 on a terminal board.  The caller puts a barrier between its
// last read of prev[i] / has_prev[i] and this.
__device__ __forceinline__ void commit_prev(const uint4* __restrict__ boards, int64_t i,
                                            const uint8_t* __restrict__ action,
                                            uint4* __restrict__ prev,
                                            uint8_t* __restrict__ has_prev) {
    const Board b = load_board(boards, i);
    const bool any = legal_mask(b) != 0u;
    if (any) {
        Board s = b;
        apply_move(s, (uint32_t)action[i] & 3u);
        prev[i] = make_uint4(s.r0, s.r1, s.r2, s.r3);
    }
    has_prev[i] = any ? 1 : 0;
}

// ------------------------------------------------------------------ device: the ring
// The ring libraries (g2048_ntlambda.hip, g2048_stagedelay.hip) keep a board's last H afterstates
// in H planes of n rows.  The ring position of a board, clamped into the domain (head < H,
// depth <= H) so that a state the caller corrupted cannot index past the planes.
struct Ring {
    uint32_t head, depth;
};

__device__ __forceinline__ Ring load_ring(const uint8_t* __restrict__ head,
                                          const uint8_t* __restrict__ depth, int64_t i,
                                          uint32_t H) {
    return Ring{min((uint32_t)head[i], H - 1u), min((uint32_t)depth[i], H)};
}

// the plane k steps back from `head`, k < H
__device__ __forceinline__ uint32_t plane_back(uint32_t head, uint32_t k, uint32_t H) {
    return head >= k ? head - k : head + H - k;
}

// ------------------------------------------------------------------ host: errors and launches
// Each library keeps its own thread-local message; these write the reason into `err`.
inline int refuse(std::string& err, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int refuse(std::string& err, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return G2048_EINVAL;
}

// a failed HIP call: its text into g_err, G2048_EHIP to the caller.  Requires a std::string
// named g_err in scope where it is used: each including .hip defines its own thread_local one.
#define G_HIP(expr)                                                                            \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            ::g2048::nt::refuse(g_err, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                                __LINE__);                                                     \
            return G2048_EHIP;                                                                 \
        }                                                                                      \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// CALL with the tuple count as the constant TT (a checked spec has 1..8 tuples)
#define DISPATCH_T(T_, CALL)                       \
    switch (T_) {                                  \
    case 1: { constexpr int TT = 1; CALL; } break; \
    case 2: { constexpr int TT = 2; CALL; } break; \
    case 3: { constexpr int TT = 3; CALL; } break; \
    case 4: { constexpr int TT = 4; CALL; } break; \
    case 5: { constexpr int TT = 5; CALL; } break; \
    case 6: { constexpr int TT = 6; CALL; } break; \
    case 7: { constexpr int TT = 7; CALL; } break; \
    default: { constexpr int TT = 8; CALL; } break; \
    }

// blocks for n boards at `per` boards per block
inline dim3 grid_for(int64_t n, int per) { return dim3((uint32_t)((n + per - 1) / per)); }
// the policy kernels' grid: 2 boards per wave
inline dim3 policy_grid(int64_t n) { return grid_for(n, POLICY_BLOCK / 32); }

// ------------------------------------------------------------------ host: validation

inline int check_spec(std::string& err, const char* who, const g2048_ntuple_spec* spec) {
    if (spec == nullptr) return refuse(err, "%s: spec is NULL", who);
    if (spec->n_tuples < 1 || spec->n_tuples > MAXT)
        return refuse(err, "%s: n_tuples = %d outside [1, %d]", who, spec->n_tuples, MAXT);
    if (spec->n_cells < 1 || spec->n_cells > MAXM)
        return refuse(err, "%s: n_cells = %d outside [1, %d]", who, spec->n_cells, MAXM);
    for (int t = 0; t < spec->n_tuples; ++t) {
        uint32_t seen = 0;
        for (int k = 0; k < spec->n_cells; ++k) {
            const uint32_t c = spec->cells[t][k];
            if (c >= 16u)
                return refuse(err, "%s: tuple %d cell %d = %u is not a board cell (0..15)", who, t,
                              k, c);
            if ((seen >> c) & 1u)
                return refuse(err, "%s: tuple %d holds cell %u twice (repeated cell)", who, t, c);
            seen |= 1u << c;
        }
    }
    return G2048_OK;
}

inline Params make_params(const g2048_ntuple_spec& spec) {
    Params p = {};
    p.entries = 1u << (4 * spec.n_cells);
    p.n_tuples = (uint32_t)spec.n_tuples;
    for (int t = 0; t < spec.n_tuples; ++t)
        for (int k = 0; k < spec.n_cells; ++k)
            p.sh[t] |= (uint64_t)(4u * spec.cells[t][k]) << (8 * k);
    return p;
}

// the checks every device entry point shares
inline int check_common(std::string& err, const char* who, const g2048_ntuple_spec* spec,
                        const int32_t* lut, const uint8_t* boards, int64_t n) {
    const int rc = check_spec(err, who, spec);
    if (rc != G2048_OK) return rc;
    if (lut == nullptr) return refuse(err, "%s: lut_dev is NULL", who);
    if (((uintptr_t)lut & 3u) != 0) return refuse(err, "%s: lut_dev must be 4-byte aligned", who);
    if (boards == nullptr) return refuse(err, "%s: boards_dev is NULL", who);
    if (((uintptr_t)boards & 15u) != 0)
        return refuse(err, "%s: boards_dev must be 16-byte aligned", who);
    if (n < 1 || n > G2048_MAX_BOARDS)
        return refuse(err, "%s: n = %lld outside [1, G2048_MAX_BOARDS]", who, (long long)n);
    return G2048_OK;
}

// the checks the learning steps share past check_common
inline int check_td_args(std::string& err, const char* who, const uint8_t* prev,
                         const uint8_t* has_prev, int32_t lr_num, int32_t lr_shift,
                         const uint8_t* action_out, const int32_t* delta_out,
                         const int64_t* err_out) {
    if (prev == nullptr || has_prev == nullptr)
        return refuse(err, "%s: prev_dev / has_prev_dev is NULL", who);
    if (((uintptr_t)prev & 15u) != 0)
        return refuse(err, "%s: prev_dev must be 16-byte aligned", who);
    if (lr_num < 0 || lr_num > G2048_NTUPLE_MAX_LR_NUM)
        return refuse(err, "%s: lr_num = %d outside [0, %d]", who, lr_num,
                      G2048_NTUPLE_MAX_LR_NUM);
    if (lr_shift < 0 || lr_shift > G2048_NTUPLE_MAX_LR_SHIFT)
        return refuse(err, "%s: lr_shift = %d outside [0, %d]", who, lr_shift,
                      G2048_NTUPLE_MAX_LR_SHIFT);
    if (action_out == nullptr || delta_out == nullptr)
        return refuse(err, "%s: action_out_dev / delta_out_dev is NULL", who);
    if (((uintptr_t)delta_out & 3u) != 0)
        return refuse(err, "%s: delta_out_dev must be 4-byte aligned", who);
    if (((uintptr_t)err_out & 7u) != 0)
        return refuse(err, "%s: err_out_dev must be 8-byte aligned", who);
    return G2048_OK;
}

// a device pointer with its alignment, a power of two
inline int check_ptr(std::string& err, const char* who, const char* name, const void* ptr,
                     unsigned align) {
    if (ptr == nullptr) return refuse(err, "%s: %s is NULL", who, name);
    if (((uintptr_t)ptr & (uintptr_t)(align - 1u)) != 0)
        return refuse(err, "%s: %s must be %u-byte aligned", who, name, align);
    return G2048_OK;
}

// what every exported *_rate returns: rate(E, A) in the domain, a refusal outside it.  Each
// library passes its own header's RATE_BITS and MAX_A.
template <int RATE_BITS, int64_t MAX_A>
inline int32_t checked_rate(std::string& err, const char* who, int64_t E, int64_t A) {
    static_assert(MAX_A == ((int64_t)1 << 62) - 1, "the message below says 2^62");
    if (A < 0 || A > MAX_A)
        return refuse(err, "%s: A = %lld outside [0, 2^62)", who, (long long)A);
    if (E > A || E < -A)
        return refuse(err, "%s: |E| = |%lld| exceeds A = %lld", who, (long long)E, (long long)A);
    return (int32_t)tc_rate<RATE_BITS>(E, A);
}

// ------------------------------------------------------------------ host: acc and ea
// The batch-mean step's two tables beside lut (g2048_ntmean_dev.hpp).  Their checks stand here so
// that g2048_ntstage_dev.hpp can run them behind its own.
// bytes of acc, and of ea: 16 per entry of every stage
inline int64_t table_bytes(const g2048_ntuple_spec& spec, int n_stages = 1) {
    return (int64_t)n_stages * ((int64_t)spec.n_tuples << (4 * spec.n_cells)) * 2 *
           (int64_t)sizeof(int64_t);
}

inline int check_acc(std::string& err, const char* who, const int64_t* acc) {
    return check_ptr(err, who, "acc_dev", acc, 16);
}

// acc and ea are two tables of `bytes` each: the same one, or two that share a part, would hand
// the exchanges of (D, C) an entry's (E, A)
inline int check_ea(std::string& err, const char* who, const int64_t* ea, const int64_t* acc,
                    int64_t bytes) {
    const int rc = check_ptr(err, who, "ea_dev", ea, 16);
    if (rc != G2048_OK) return rc;
    const uintptr_t a = (uintptr_t)acc, b = (uintptr_t)ea;
    if ((a < b ? b - a : a - b) < (uintptr_t)bytes)
        return refuse(err, "%s: ea_dev overlaps acc_dev", who);
    return G2048_OK;
}

}  // namespace nt
}  // namespace g2048
