// g2048_ntuple.hip -- n-tuple value network for gfx950 (libg2048_ntuple.so): evaluation, greedy
// afterstate policy and the TD(0) update.
//
// The network is defined in include/g2048_ntuple.h; every value is an integer and the result is
// checked bit for bit against tests/ntuple_ref.py.  No float anywhere.
//
// Lane layout.  The unit of work is a GROUP OF 8 LANES: lane g of a group applies symmetry g to
// the group's board in registers (transpose = 8 v_perm, row flip = 4 selects, column flip = 4
// v_perm), clamps the exponents to 15, packs them into 16 nibbles (one u64), and loops over the T
// tuples with the spec's own cell lists -- which stay wave-uniform, so a tuple's shifts are
// scalar operands.  Transforming the board by g and reading the spec's cells is the same as
// reading the board through the expanded cell list of (g, t) (g2048_ntuple_expand).  T is a
// template parameter: a lane's T gathers are all issued before the first is used, then summed as
// int64 and reduced over the group by three xor-shuffles.
//   k_values  8 boards per wave (one group each)
//   k_policy  2 boards per wave: lane 32s + 8a + g evaluates after(board s, a) under g; illegal
//             moves load nothing.  For the TD step the groups a == 0 also gather V(prev) in the
//             same burst (T more loads in flight on 16 lanes), so err and delta cost no second
//             pass over the board.
//   k_update  8 boards per wave, 128 per block: lane g adds delta into its T entries of
//             idx(prev, g, .) -- summed per block in LDS first, then no-return 32-bit integer
//             atomics -- and lane 0 of the group commits prev / has_prev.
// The two launches of g2048_ntuple_td_step are the only ordering: the first never writes the
// table, the second never reads it.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/g2048_ntuple.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

namespace {

using namespace g2048;
// Params, sym / pack_row / nibbles / entry, load_board and the spec checks are shared with
// g2048_ntsearch.hip
using namespace g2048::nt;

// sum over the 8 lanes of a group
__device__ __forceinline__ int64_t group_sum(int64_t v) {
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

constexpr int BLOCK = 256;

template <int T>
__global__ __launch_bounds__(BLOCK) void k_values(const int32_t* __restrict__ lut,
                                                  const uint4* __restrict__ boards, int64_t n,
                                                  int64_t* __restrict__ values, Params p) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    const bool live = i < n;  // dead groups keep their lanes for the shuffles
    const uint64_t nib = nibbles(sym(load_board(boards, live ? i : n - 1), g));
    int32_t v[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = lut[entry(p, nib, t)];
    int64_t s = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) s += v[t];
    s = group_sum(s);
    if (live && g == 0u) values[i] = s;
}

template <int T, bool TD>
__global__ __launch_bounds__(BLOCK) void k_policy(
    const int32_t* __restrict__ lut, const uint4* __restrict__ boards, int64_t n,
    int64_t* __restrict__ q_out, uint8_t* __restrict__ action_out, uint4* __restrict__ after_out,
    const uint4* __restrict__ prev, const uint8_t* __restrict__ has_prev, int32_t lr_num,
    int32_t lr_shift, int32_t* __restrict__ delta_out, int64_t* __restrict__ err_out, Params p) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t wave = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t i = wave * 2 + (lane >> 5);
    const uint32_t a = (lane >> 3) & 3u, g = lane & 7u;
    const bool live = i < n;
    const int64_t bi = live ? i : n - 1;
    const Board b = load_board(boards, bi);
    const uint32_t legal = legal_mask(b);
    const bool ok = ((legal >> a) & 1u) != 0u;
    Board s = b;
    const uint32_t gain = apply_move(s, a);
    const uint64_t nib = nibbles(sym(s, g));
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = ok ? lut[entry(p, nib, t)] : 0;
    bool hp = false;
    if constexpr (TD) {
        hp = has_prev[bi] != 0;
        const uint64_t pnib = nibbles(sym(load_board(prev, bi), g));
#pragma unroll
        for (int t = 0; t < T; ++t) pv[t] = (hp && a == 0u) ? lut[entry(p, pnib, t)] : 0;
    }
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const int64_t q = ok ? ((int64_t)gain << F) + sum : INT64_MIN;
    const uint32_t base = lane & 32u;
    const int64_t q0 = __shfl(q, base), q1 = __shfl(q, base + 8u);
    const int64_t q2 = __shfl(q, base + 16u), q3 = __shfl(q, base + 24u);
    // smallest a with the largest q; an illegal move holds INT64_MIN and a legal move's q is far
    // above it, so with no legal move the action stays 0
    uint32_t act = 0;
    int64_t best = q0;
    if (q1 > best) { act = 1; best = q1; }
    if (q2 > best) { act = 2; best = q2; }
    if (q3 > best) { act = 3; best = q3; }
    if constexpr (TD) {
#pragma unroll
        for (int t = 0; t < T; ++t) psum += pv[t];
        psum = group_sum(psum);  // V(prev) in the group a == 0
    }
    if (!live) return;
    if (q_out != nullptr && (lane & 31u) < 4u) {
        const uint32_t k = lane & 3u;
        q_out[i * 4 + k] = k == 0u ? q0 : k == 1u ? q1 : k == 2u ? q2 : q3;
    }
    if (action_out != nullptr && (lane & 31u) == 0u) action_out[i] = (uint8_t)act;
    // the lane (a == action, g == 0) holds after(b, action); with no legal move after = b
    if (after_out != nullptr && a == act && g == 0u) {
        const Board o = legal != 0u ? s : b;
        after_out[i] = make_uint4(o.r0, o.r1, o.r2, o.r3);
    }
    if constexpr (TD) {
        if ((lane & 31u) == 0u) {
            const int64_t target = legal != 0u ? best : 0;
            const int64_t err = hp ? target - psum : 0;
            delta_out[i] = (int32_t)((err * (int64_t)lr_num) >> lr_shift);
            if (err_out != nullptr) err_out[i] = err;
        }
    }
}

// The update's block: 128 boards.  The boards of a batch share their early-game entries (the
// index of four or six empty cells, of a lone 2 in a corner, ...), and adds into one address
// serialise at the memory side, so a block first sums what it adds into an entry in an LDS hash
// table (the entry index is the key; after four slots taken by other keys the add goes straight
// to memory) and then flushes every used slot with one atomic.  Integer adds commute and associate
// modulo 2^32, so the table ends up the same whichever way the sum is grouped.
constexpr int UBLOCK = 1024, SLOT_BITS = 13;
constexpr uint32_t SLOTS = 1u << SLOT_BITS, PROBES = 4;  // 64 KiB of LDS, linear probing
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;  // entry indices are < 2^27

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_update(int32_t* __restrict__ lut,
                                                   const uint4* __restrict__ boards, int64_t n,
                                                   uint4* __restrict__ prev,
                                                   uint8_t* __restrict__ has_prev,
                                                   const uint8_t* __restrict__ action,
                                                   const int32_t* __restrict__ delta, Params p) {
    __shared__ uint32_t keys[SLOTS];
    __shared__ uint32_t sums[SLOTS];
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        keys[s] = NO_KEY;
        sums[s] = 0u;
    }
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * UBLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    const bool live = i < n;
    uint32_t* table = reinterpret_cast<uint32_t*>(lut);  // additions modulo 2^32
    const uint32_t d = live && has_prev[i] != 0 ? (uint32_t)delta[i] : 0u;
    if (d != 0u) {
        const uint64_t nib = nibbles(sym(load_board(prev, i), g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = entry(p, nib, t);
            const uint32_t home = (e * 0x9E3779B1u) >> (32 - SLOT_BITS);
            bool placed = false;
#pragma unroll
            for (uint32_t probe = 0; probe < PROBES; ++probe) {
                if (placed) continue;
                const uint32_t slot = (home + probe) & (SLOTS - 1u);
                const uint32_t old = atomicCAS(&keys[slot], NO_KEY, e);
                placed = old == NO_KEY || old == e;
                if (placed) atomicAdd(&sums[slot], d);
            }
            if (!placed) atomicAdd(&table[e], d);
        }
    }
    // every read of prev[i] and has_prev[i] lies before this barrier, lane 0's stores after it
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s], v = sums[s];
        if (k != NO_KEY && v != 0u) atomicAdd(&table[k], v);
    }
    if (!live || g != 0u) return;
    const Board b = load_board(boards, i);
    const bool any = legal_mask(b) != 0u;
    if (any) {
        Board s = b;
        apply_move(s, (uint32_t)action[i] & 3u);
        prev[i] = make_uint4(s.r0, s.r1, s.r2, s.r3);
    }
    has_prev[i] = any ? 1 : 0;
}

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define G_HIP(expr)                                                                        \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(G2048_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                         \
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

int check_spec(const char* who, const g2048_ntuple_spec* spec) {
    return nt::check_spec(g_err, who, spec);
}

int check_common(const char* who, const g2048_ntuple_spec* spec, const int32_t* lut,
                 const uint8_t* boards, int64_t n) {
    return nt::check_common(g_err, who, spec, lut, boards, n);
}

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

// blocks of BLOCK threads for n boards at `per` boards per block
dim3 grid_for(int64_t n, int per) { return dim3((uint32_t)((n + per - 1) / per)); }

}  // namespace

extern "C" {

const char* g2048_ntuple_last_error(void) { return g_err.c_str(); }

int64_t g2048_ntuple_lut_entries(const g2048_ntuple_spec* spec) {
    const int rc = check_spec("ntuple_lut_entries", spec);
    if (rc != G2048_OK) return rc;
    return (int64_t)spec->n_tuples << (4 * spec->n_cells);
}

int g2048_ntuple_expand(const g2048_ntuple_spec* spec, uint8_t out[8][MAXT][MAXM]) {
    const int rc = check_spec("ntuple_expand", spec);
    if (rc != G2048_OK) return rc;
    if (out == nullptr) return fail(G2048_EINVAL, "ntuple_expand: out is NULL");
    for (int g = 0; g < 8; ++g) {
        const bool tr = (g >> 2) & 1, fc = (g >> 1) & 1, fr = g & 1;
        for (int t = 0; t < MAXT; ++t)
            for (int k = 0; k < MAXM; ++k) {
                if (t >= spec->n_tuples || k >= spec->n_cells) {
                    out[g][t][k] = 0;
                    continue;
                }
                const int cell = spec->cells[t][k], r = cell >> 2, c = cell & 3;
                const int rr = fr ? 3 - r : r, cc = fc ? 3 - c : c;
                out[g][t][k] = (uint8_t)(tr ? 4 * cc + rr : 4 * rr + cc);
            }
    }
    return G2048_OK;
}

int g2048_ntuple_values(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                        const uint8_t* boards_dev, int64_t n, int64_t* values_out_dev,
                        int device_id, void* stream) {
    const int rc = check_common("ntuple_values", spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (values_out_dev == nullptr)
        return fail(G2048_EINVAL, "ntuple_values: values_out_dev is NULL");
    if (((uintptr_t)values_out_dev & 7u) != 0)
        return fail(G2048_EINVAL, "ntuple_values: values_out_dev must be 8-byte aligned");
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    DISPATCH_T(spec->n_tuples, (k_values<TT><<<grid_for(n, BLOCK / 8), dim3(BLOCK), 0, st>>>(
                                   lut_dev, boards, n, values_out_dev, p)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_ntuple_act(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                     const uint8_t* boards_dev, int64_t n, int64_t* q_out_dev,
                     uint8_t* action_out_dev, uint8_t* after_out_dev, int device_id,
                     void* stream) {
    const int rc = check_common("ntuple_act", spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (q_out_dev == nullptr && action_out_dev == nullptr && after_out_dev == nullptr)
        return fail(G2048_EINVAL, "ntuple_act: all three outputs are NULL");
    if (((uintptr_t)q_out_dev & 7u) != 0)
        return fail(G2048_EINVAL, "ntuple_act: q_out_dev must be 8-byte aligned");
    if (((uintptr_t)after_out_dev & 15u) != 0)
        return fail(G2048_EINVAL, "ntuple_act: after_out_dev must be 16-byte aligned");
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* after = reinterpret_cast<uint4*>(after_out_dev);
    DISPATCH_T(spec->n_tuples,
               (k_policy<TT, false><<<grid_for(n, BLOCK / 32), dim3(BLOCK), 0, st>>>(
                   lut_dev, boards, n, q_out_dev, action_out_dev, after, nullptr, nullptr, 0, 0,
                   nullptr, nullptr, p)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_ntuple_td_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, const uint8_t* boards_dev,
                         int64_t n, uint8_t* prev_dev, uint8_t* has_prev_dev, int32_t lr_num,
                         int32_t lr_shift, uint8_t* action_out_dev, int32_t* delta_out_dev,
                         int64_t* err_out_dev, int device_id, void* stream) {
    const int rc = check_common("ntuple_td_step", spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (prev_dev == nullptr || has_prev_dev == nullptr)
        return fail(G2048_EINVAL, "ntuple_td_step: prev_dev / has_prev_dev is NULL");
    if (((uintptr_t)prev_dev & 15u) != 0)
        return fail(G2048_EINVAL, "ntuple_td_step: prev_dev must be 16-byte aligned");
    if (lr_num < 0 || lr_num > G2048_NTUPLE_MAX_LR_NUM)
        return fail(G2048_EINVAL, "ntuple_td_step: lr_num = %d outside [0, %d]", lr_num,
                    G2048_NTUPLE_MAX_LR_NUM);
    if (lr_shift < 0 || lr_shift > G2048_NTUPLE_MAX_LR_SHIFT)
        return fail(G2048_EINVAL, "ntuple_td_step: lr_shift = %d outside [0, %d]", lr_shift,
                    G2048_NTUPLE_MAX_LR_SHIFT);
    if (action_out_dev == nullptr || delta_out_dev == nullptr)
        return fail(G2048_EINVAL, "ntuple_td_step: action_out_dev / delta_out_dev is NULL");
    if (((uintptr_t)delta_out_dev & 3u) != 0)
        return fail(G2048_EINVAL, "ntuple_td_step: delta_out_dev must be 4-byte aligned");
    if (((uintptr_t)err_out_dev & 7u) != 0)
        return fail(G2048_EINVAL, "ntuple_td_step: err_out_dev must be 8-byte aligned");
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* prev = reinterpret_cast<uint4*>(prev_dev);
    DISPATCH_T(spec->n_tuples,
               (k_policy<TT, true><<<grid_for(n, BLOCK / 32), dim3(BLOCK), 0, st>>>(
                   lut_dev, boards, n, nullptr, action_out_dev, nullptr, prev, has_prev_dev,
                   lr_num, lr_shift, delta_out_dev, err_out_dev, p)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples, (k_update<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                                   lut_dev, boards, n, prev, has_prev_dev, action_out_dev,
                                   delta_out_dev, p)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
