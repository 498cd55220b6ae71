// g2048_ntstage.hip -- multi-stage n-tuple value network with weight promotion for gfx950
// (libg2048_ntstage.so): evaluation, greedy afterstate policy and the TD(0) update.
//
// The network is defined in include/g2048_ntstage.h: S tables of g2048_ntuple.h's shape, the one
// a board reads chosen by its largest tile, and INT32_MIN for "never written", which falls
// through to the stage below.  Every value is an integer and the result is checked bit for bit
// against tests/ntstage_ref.py.  No float anywhere.
//
// The kernels keep the frames of g2048_ntuple.hip (lane layouts, group sum, argmax, err / delta,
// the LDS merge table and the prev commit all come from g2048_ntuple_dev.hpp):
//   k_stage_values  8 boards per wave (one group each)
//   k_stage_policy  2 boards per wave: lane 32s + 8a + g evaluates after(board s, a) under g, at
//                   the AFTERSTATE's stage.  For the TD step the groups a == 0 also gather
//                   V(prev) in the same burst and store the promoted values.
//   k_stage_update  8 boards per wave, 128 per block: lane g adds delta into its T entries of
//                   idx(prev, g, .) at stage(prev) through the block's LDS merge table.
// g2048_ntstage_dev.hpp holds what this file shares with the other libraries that read a staged
// table: M(b) and the stage, the fall-through (resolve), k_stage_policy itself (the staged
// batch-mean steps launch it too) with the argument why its promotion needs no ordering, and the
// validation of a stage spec.  Here are k_stage_values, k_stage_update and the entry points.
//   M(b) and the stage  M(b) is taken on the un-transformed board in registers: the even and the
//       odd bytes of the four words as 16-bit pairs, seven v_pk_max_u16 and one max of the two
//       halves.  The bounds ride in the params struct as eight bytes (255 past S - 1, above any
//       exponent), wave-uniform, so the stage is seven compares against scalar operands.  The
//       entry index becomes s * T * 16^m + entry(...) < 2^30, so NO_KEY stays free.
//   Gathers  The T gathers at the lane's own stage are all issued before the first use.  Lanes
//       that received UNSET then step down one stage and gather again, at most S - 1 rounds and
//       only the lanes that need it; a wave leaves the loop as soon as none of its lanes does.
//       In the TD step the afterstate's and prev's entries share the rounds.
//   Promotion  The groups a == 0 of the policy launch have resolved prev's entries; they store
//       the resolved value into those they found UNSET.  The update launch then only adds, into
//       entries that are no longer UNSET, and never reads the table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_ntstage.h"
#include "../../include/g2048_ntuple.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int BLOCK = 256;

template <int T>
__global__ __launch_bounds__(BLOCK) void k_stage_values(const int32_t* __restrict__ lut,
                                                        const uint4* __restrict__ boards,
                                                        int64_t n, int64_t* __restrict__ values,
                                                        Params p, StageParams sp) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    const bool live = i < n;  // dead groups keep their lanes for the shuffles and the vote
    const Board b = load_board(boards, live ? i : n - 1);
    const uint32_t st = stage_of(b, sp);
    const uint64_t nib = nibbles(sym(b, g));
    uint32_t e[T];
    int32_t v[T];
#pragma unroll
    for (int t = 0; t < T; ++t) e[t] = st * sp.stride + entry(p, nib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = lut[e[t]];
    resolve<T, false>(lut, sp, e, v, st, e, v, st);
    int64_t s = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) s += v[t];
    s = group_sum(s);
    if (live && g == 0u) values[i] = s;
}

// The update's block, as in g2048_ntuple.hip: 128 boards, their adds summed per entry in an LDS
// hash table first (the key is the staged entry index, < 2^30), then one atomic per used slot.
// The entries it adds into were promoted by the policy launch, so none of them is UNSET and the
// table is never read here.
constexpr int UBLOCK = 1024, SLOT_BITS = 13;
constexpr uint32_t SLOTS = 1u << SLOT_BITS;  // 64 KiB of LDS

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_stage_update(
    int32_t* __restrict__ lut, const uint4* __restrict__ boards, int64_t n,
    uint4* __restrict__ prev, uint8_t* __restrict__ has_prev, const uint8_t* __restrict__ action,
    const int32_t* __restrict__ delta, Params p, StageParams sp) {
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
        const Board pb = load_board(prev, i);
        const uint32_t base = stage_of(pb, sp) * sp.stride;
        const uint64_t nib = nibbles(sym(pb, g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = base + entry(p, nib, t);
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

const char* g2048_ntstage_last_error(void) { return g_err.c_str(); }

int64_t g2048_ntstage_lut_entries(const g2048_ntuple_spec* spec,
                                  const g2048_ntstage_spec* stages) {
    const char* who = "ntstage_lut_entries";
    int rc = check_spec(g_err, who, spec);
    if (rc != G2048_OK) return rc;
    rc = check_stages(g_err, who, stages);
    if (rc != G2048_OK) return rc;
    return (int64_t)stages->n_stages * ((int64_t)spec->n_tuples << (4 * spec->n_cells));
}

int g2048_ntstage_values(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                         const int32_t* lut_dev, const uint8_t* boards_dev, int64_t n,
                         int64_t* values_out_dev, int device_id, void* stream) {
    const int rc = check_staged(g_err, "ntstage_values", spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (values_out_dev == nullptr)
        return refuse(g_err, "ntstage_values: values_out_dev is NULL");
    if (((uintptr_t)values_out_dev & 7u) != 0)
        return refuse(g_err, "ntstage_values: values_out_dev must be 8-byte aligned");
    const Params p = make_params(*spec);
    const StageParams sp = make_stage_params(*spec, *stages);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    DISPATCH_T(spec->n_tuples,
               (k_stage_values<TT><<<grid_for(n, BLOCK / 8), dim3(BLOCK), 0, st>>>(
                   lut_dev, boards, n, values_out_dev, p, sp)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_ntstage_act(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                      const int32_t* lut_dev, const uint8_t* boards_dev, int64_t n,
                      int64_t* q_out_dev, uint8_t* action_out_dev, uint8_t* after_out_dev,
                      int device_id, void* stream) {
    const int rc = check_staged(g_err, "ntstage_act", spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (q_out_dev == nullptr && action_out_dev == nullptr && after_out_dev == nullptr)
        return refuse(g_err, "ntstage_act: all three outputs are NULL");
    if (((uintptr_t)q_out_dev & 7u) != 0)
        return refuse(g_err, "ntstage_act: q_out_dev must be 8-byte aligned");
    if (((uintptr_t)after_out_dev & 15u) != 0)
        return refuse(g_err, "ntstage_act: after_out_dev must be 16-byte aligned");
    const Params p = make_params(*spec);
    const StageParams sp = make_stage_params(*spec, *stages);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* after = reinterpret_cast<uint4*>(after_out_dev);
    DISPATCH_T(spec->n_tuples,
               (k_stage_policy<TT, false><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, nullptr, nullptr, 0, 0, nullptr, nullptr, p,
                   sp, q_out_dev, after)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

int g2048_ntstage_td_step(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                          int32_t* lut_dev, const uint8_t* boards_dev, int64_t n,
                          uint8_t* prev_dev, uint8_t* has_prev_dev, int32_t lr_num,
                          int32_t lr_shift, uint8_t* action_out_dev, int32_t* delta_out_dev,
                          int64_t* err_out_dev, int device_id, void* stream) {
    const char* who = "ntstage_td_step";
    int rc = check_staged(g_err, who, spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    const Params p = make_params(*spec);
    const StageParams sp = make_stage_params(*spec, *stages);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* prev = reinterpret_cast<uint4*>(prev_dev);
    DISPATCH_T(spec->n_tuples,
               (k_stage_policy<TT, true><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, prev, has_prev_dev, lr_num, lr_shift,
                   delta_out_dev, err_out_dev, p, sp, nullptr, nullptr)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples,
               (k_stage_update<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                   lut_dev, boards, n, prev, has_prev_dev, action_out_dev, delta_out_dev, p, sp)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
