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
//
// g2048_ntuple_dev.hpp holds what this file shares with the other libraries of the family: the
// index helpers, the policy's lane decode, group sum, argmax and err / delta, k_policy itself
// (the batch-mean steps launch it too), the merge table's keys and the prev commit of the update,
// and the host plumbing and argument checks.  Here are k_values, k_update with the merge table's
// sums, and the entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_ntuple.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

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

// The update's block: 128 boards.  The boards of a batch share their early-game entries (the
// index of four or six empty cells, of a lone 2 in a corner, ...), and adds into one address
// serialise at the memory side, so a block first sums what it adds into an entry in an LDS hash
// table (g2048_ntuple_dev.hpp's clear_keys / claim_slot: the entry index is the key; after four
// slots taken by other keys the add goes straight to memory) and then flushes every used slot
// with one atomic.  Integer adds commute and associate modulo 2^32, so the table ends up the same
// whichever way the sum is grouped.
constexpr int UBLOCK = 1024, SLOT_BITS = 13;
constexpr uint32_t SLOTS = 1u << SLOT_BITS;  // 64 KiB of LDS

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_update(int32_t* __restrict__ lut,
                                                   const uint4* __restrict__ boards, int64_t n,
                                                   uint4* __restrict__ prev,
                                                   uint8_t* __restrict__ has_prev,
                                                   const uint8_t* __restrict__ action,
                                                   const int32_t* __restrict__ delta, Params p) {
    __shared__ uint32_t keys[SLOTS];
    __shared__ uint32_t sums[SLOTS];
    clear_keys<SLOT_BITS, UBLOCK>(keys);
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) sums[s] = 0u;
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
            const uint32_t slot = claim_slot<SLOT_BITS>(keys, e);
            if (slot != NO_SLOT) atomicAdd(&sums[slot], d);
            else atomicAdd(&table[e], d);
        }
    }
    // every read of prev[i] and has_prev[i] lies before this barrier, lane 0's stores after it
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s], v = sums[s];
        if (k != NO_KEY && v != 0u) atomicAdd(&table[k], v);
    }
    if (live && g == 0u) commit_prev(boards, i, action, prev, has_prev);
}

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_ntuple_last_error(void) { return g_err.c_str(); }

int64_t g2048_ntuple_lut_entries(const g2048_ntuple_spec* spec) {
    const int rc = check_spec(g_err, "ntuple_lut_entries", spec);
    if (rc != G2048_OK) return rc;
    return (int64_t)spec->n_tuples << (4 * spec->n_cells);
}

int g2048_ntuple_expand(const g2048_ntuple_spec* spec, uint8_t out[8][MAXT][MAXM]) {
    const int rc = check_spec(g_err, "ntuple_expand", spec);
    if (rc != G2048_OK) return rc;
    if (out == nullptr) return refuse(g_err, "ntuple_expand: out is NULL");
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
    const int rc = check_common(g_err, "ntuple_values", spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (values_out_dev == nullptr)
        return refuse(g_err, "ntuple_values: values_out_dev is NULL");
    if (((uintptr_t)values_out_dev & 7u) != 0)
        return refuse(g_err, "ntuple_values: values_out_dev must be 8-byte aligned");
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
    const int rc = check_common(g_err, "ntuple_act", spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (q_out_dev == nullptr && action_out_dev == nullptr && after_out_dev == nullptr)
        return refuse(g_err, "ntuple_act: all three outputs are NULL");
    if (((uintptr_t)q_out_dev & 7u) != 0)
        return refuse(g_err, "ntuple_act: q_out_dev must be 8-byte aligned");
    if (((uintptr_t)after_out_dev & 15u) != 0)
        return refuse(g_err, "ntuple_act: after_out_dev must be 16-byte aligned");
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* after = reinterpret_cast<uint4*>(after_out_dev);
    DISPATCH_T(spec->n_tuples,
               (k_policy<TT, false><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, nullptr, nullptr, 0, 0, nullptr, nullptr, p,
                   q_out_dev, after)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_ntuple_td_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, const uint8_t* boards_dev,
                         int64_t n, uint8_t* prev_dev, uint8_t* has_prev_dev, int32_t lr_num,
                         int32_t lr_shift, uint8_t* action_out_dev, int32_t* delta_out_dev,
                         int64_t* err_out_dev, int device_id, void* stream) {
    const char* who = "ntuple_td_step";
    int rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* prev = reinterpret_cast<uint4*>(prev_dev);
    DISPATCH_T(spec->n_tuples,
               (k_policy<TT, true><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, prev, has_prev_dev, lr_num, lr_shift,
                   delta_out_dev, err_out_dev, p, nullptr, nullptr)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples, (k_update<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                                   lut_dev, boards, n, prev, has_prev_dev, action_out_dev,
                                   delta_out_dev, p)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
