// g2048_nttc.hip -- temporal-coherence learning for the n-tuple value network on gfx950
// (libg2048_nttc.so).
//
// The rule is defined in include/g2048_nttc.h; every value is an integer and the result is checked
// bit for bit against tests/nttc_ref.py.  No float anywhere.  The library takes the spec and the
// table of g2048_ntuple.h and does not link against libg2048_ntuple.so.  What it has in common
// with g2048_ntuple.hip is g2048_ntuple_dev.hpp's: the index helpers, the policy's lane decode,
// group sum, argmax and err / delta, the rate, the merge table's keys and the prev commit of the
// update, and the host plumbing and argument checks.  Here are the (E, A) gather, the hand-over of
// the steps, the merge table's three sums and the entry points.
//
// A step is two launches, because an entry's step depends on its (E, A) from before the call and
// nothing orders a read in one block against an add in another:
//   k_tc_policy  g2048_ntuple.hip's k_policy layout: 2 boards per wave, lane 32s + 8a + g
//                evaluates after(board s, a) under symmetry g.  The groups a == 0 also form
//                idx(prev, g, .) and, in the same burst as the afterstates' gathers, load lut and
//                the 16 bytes of (E, A) there (one global_load_dwordx4 per entry).  Every lane of
//                such a group then has err and delta (the half-wave's best q by shuffles, V(prev)
//                by the group sum), computes rate and step for its T entries and writes the
//                steps to the workspace: work[(8 i + g) T + t].
//   k_tc_update  8 boards per wave, 128 per block: lane g re-forms its T entries of
//                idx(prev, g, .), reads its steps back and adds step into lut (32 bit), delta
//                into E and |delta| into A (64 bit).  Per block the three sums of an entry are
//                first merged in an LDS hash table and each used slot is flushed with one atomic
//                per sum; lane 0 of the group then commits prev / has_prev.
// The first launch never writes lut or ea, the second never reads them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_nttc.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

// The scatter's form: 1 = merged per block in LDS (kept), 0 = one atomic per add.
#ifndef G2048_NTTC_MERGE
#define G2048_NTTC_MERGE 1
#endif
// G2048_NTTC_SLOT_BITS, if defined, fixes log2 of the LDS table's slots for every T
// (tc_slot_bits)

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int RATE_BITS = G2048_NTTC_RATE_BITS;

// rate(E, A) of the header is g2048_ntuple_dev.hpp's tc_rate<RATE_BITS>
__host__ __device__ __forceinline__ int32_t tc_step_of(int32_t delta, uint32_t rate) {
    return (int32_t)(((int64_t)delta * (int64_t)rate) >> RATE_BITS);
}

constexpr int BLOCK = 256;

template <int T>
__global__ __launch_bounds__(BLOCK) void k_tc_policy(
    const int32_t* __restrict__ lut, const longlong2* __restrict__ ea,
    const uint4* __restrict__ boards, int64_t n, uint8_t* __restrict__ action_out,
    const uint4* __restrict__ prev, const uint8_t* __restrict__ has_prev, int32_t lr_num,
    int32_t lr_shift, int32_t* __restrict__ delta_out, int64_t* __restrict__ err_out,
    int32_t* __restrict__ work, Params p) {
    const PolicyLane l = policy_lane<BLOCK>(boards, n);
    int32_t v[T], pv[T];
    longlong2 pea[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[entry(p, l.nib, t)] : 0;
    const bool hp = has_prev[l.bi] != 0;
    const bool mine = hp && l.a == 0u;  // this lane reads idx(prev, g, .)
    const uint64_t pnib = nibbles(sym(load_board(prev, l.bi), l.g));
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const uint32_t e = entry(p, pnib, t);
        pv[t] = mine ? lut[e] : 0;
        pea[t] = mine ? ea[e] : make_longlong2(0, 0);
    }
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const Best m = best_move<8>(l.ok ? ((int64_t)l.gain << F) + sum : INT64_MIN, l.lane);
#pragma unroll
    for (int t = 0; t < T; ++t) psum += pv[t];
    psum = group_sum(psum);  // V(prev) in the group a == 0
    if (!l.live) return;
    // every lane of the group a == 0 holds best, V(prev) and has_prev: err and delta need no
    // broadcast
    const TdError td = td_error(m.best, psum, hp, l.legal, lr_num, lr_shift);
    if ((l.lane & 31u) == 0u) {
        action_out[l.i] = (uint8_t)m.act;
        delta_out[l.i] = td.delta;
        if (err_out != nullptr) err_out[l.i] = td.err;
    }
    if (mine && td.delta != 0) {
        int32_t* w = work + (l.i * 8 + l.g) * T;
#pragma unroll
        for (int t = 0; t < T; ++t)
            w[t] = tc_step_of(td.delta, tc_rate<RATE_BITS>(pea[t].x, pea[t].y));
    }
}

// The update's block: 128 boards.  The boards of a batch share their early-game entries, and adds
// into one address serialise at the memory side, so a block first sums what it adds into an entry
// in an LDS hash table (g2048_ntuple_dev.hpp's clear_keys / claim_slot: the entry index is the
// key; after four slots taken by other keys the adds go straight to memory) and then flushes every
// used slot.  Integer adds commute and associate modulo 2^32 and 2^64, so lut and ea end up the
// same whichever way the sums are grouped.
constexpr int UBLOCK = 1024;
#if G2048_NTTC_MERGE
// log2 of the table's slots; a slot is 24 bytes (key, step sum, E sum, A sum) and a block makes
// 1024 T entry updates.  Measured: the 4 x 6 set gets faster with every doubling up
// to the 4096 slots (96 KiB, one block per CU) that fit a CU's 160 KiB of LDS; on the 2 x 4 set
// 1024 to 4096 slots differ by less than one run differs from the next, so it keeps 1024.
template <int T>
constexpr int tc_slot_bits() {
#ifdef G2048_NTTC_SLOT_BITS
    return G2048_NTTC_SLOT_BITS;
#else
    return T <= 1 ? 9 : T == 2 ? 10 : 12;
#endif
}
#endif

using u64 = unsigned long long;

// the three adds of one entry, straight to memory
__device__ __forceinline__ void add_sums(uint32_t* table, u64* ea, uint32_t e, uint32_t step,
                                         u64 de, u64 da) {
    if (step != 0u) atomicAdd(&table[e], step);
    if (de != 0ull) atomicAdd(&ea[2u * (size_t)e], de);
    atomicAdd(&ea[2u * (size_t)e + 1u], da);
}

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_tc_update(
    int32_t* __restrict__ lut, int64_t* __restrict__ ea_, const uint4* __restrict__ boards,
    int64_t n, uint4* __restrict__ prev, uint8_t* __restrict__ has_prev,
    const uint8_t* __restrict__ action, const int32_t* __restrict__ delta,
    const int32_t* __restrict__ work, Params p) {
#if G2048_NTTC_MERGE
    constexpr int SLOT_BITS = tc_slot_bits<T>();
    constexpr uint32_t SLOTS = 1u << SLOT_BITS;
    static_assert(SLOTS * 24u <= 160u * 1024u, "the LDS table must fit a CU's 160 KiB");
    __shared__ uint32_t keys[SLOTS];
    __shared__ uint32_t steps[SLOTS];
    __shared__ u64 esum[SLOTS];
    __shared__ u64 asum[SLOTS];
    clear_keys<SLOT_BITS, UBLOCK>(keys);
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        steps[s] = 0u;
        esum[s] = 0ull;
        asum[s] = 0ull;
    }
    __syncthreads();
#endif
    const int64_t tid = (int64_t)blockIdx.x * UBLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    const bool live = i < n;
    uint32_t* table = reinterpret_cast<uint32_t*>(lut);  // additions modulo 2^32
    u64* ea = reinterpret_cast<u64*>(ea_);               // and modulo 2^64
    const int32_t d = live && has_prev[i] != 0 ? delta[i] : 0;
    if (d != 0) {
        const uint64_t nib = nibbles(sym(load_board(prev, i), g));
        const int32_t* w = work + (i * 8 + g) * T;
        const u64 de = (u64)(int64_t)d;
        const u64 da = d < 0 ? 0ull - de : de;  // |INT32_MIN| = 2^31
        int32_t st[T];
#pragma unroll
        for (int t = 0; t < T; ++t) st[t] = w[t];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = entry(p, nib, t);
            const uint32_t step = (uint32_t)st[t];
#if G2048_NTTC_MERGE
            const uint32_t slot = claim_slot<SLOT_BITS>(keys, e);
            if (slot != NO_SLOT) {
                if (step != 0u) atomicAdd(&steps[slot], step);
                atomicAdd(&esum[slot], de);
                atomicAdd(&asum[slot], da);
            } else {
                add_sums(table, ea, e, step, de, da);
            }
#else
            add_sums(table, ea, e, step, de, da);
#endif
        }
    }
    // every read of prev[i] and has_prev[i] lies before this barrier, lane 0's stores after it
    __syncthreads();
#if G2048_NTTC_MERGE
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s];
        if (k != NO_KEY) add_sums(table, ea, k, steps[s], esum[s], asum[s]);
    }
#endif
    if (live && g == 0u) commit_prev(boards, i, action, prev, has_prev);
}

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_nttc_last_error(void) { return g_err.c_str(); }

int32_t g2048_nttc_rate(int64_t E, int64_t A) {
    return nt::checked_rate<RATE_BITS, G2048_NTTC_MAX_A>(g_err, "nttc_rate", E, A);
}

int64_t g2048_nttc_work_bytes(const g2048_ntuple_spec* spec, int64_t n) {
    const int rc = nt::check_spec(g_err, "nttc_work_bytes", spec);
    if (rc != G2048_OK) return rc;
    if (n < 1 || n > G2048_MAX_BOARDS)
        return refuse(g_err, "nttc_work_bytes: n = %lld outside [1, G2048_MAX_BOARDS]",
                      (long long)n);
    return n * 8 * spec->n_tuples * (int64_t)sizeof(int32_t);
}

int g2048_nttc_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, int64_t* ea_dev,
                    const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev, uint8_t* has_prev_dev,
                    int32_t lr_num, int32_t lr_shift, uint8_t* action_out_dev,
                    int32_t* delta_out_dev, int64_t* err_out_dev, void* work_dev, int device_id,
                    void* stream) {
    const char* who = "nttc_step";
    int rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (ea_dev == nullptr) return refuse(g_err, "nttc_step: ea_dev is NULL");
    if (((uintptr_t)ea_dev & 15u) != 0)
        return refuse(g_err, "nttc_step: ea_dev must be 16-byte aligned");
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    if (work_dev == nullptr) return refuse(g_err, "nttc_step: work_dev is NULL");
    if (((uintptr_t)work_dev & 3u) != 0)
        return refuse(g_err, "nttc_step: work_dev must be 4-byte aligned");
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* prev = reinterpret_cast<uint4*>(prev_dev);
    const longlong2* ea = reinterpret_cast<const longlong2*>(ea_dev);
    int32_t* work = static_cast<int32_t*>(work_dev);
    DISPATCH_T(spec->n_tuples,
               (k_tc_policy<TT><<<grid_for(n, BLOCK / 32), dim3(BLOCK), 0, st>>>(
                   lut_dev, ea, boards, n, action_out_dev, prev, has_prev_dev, lr_num, lr_shift,
                   delta_out_dev, err_out_dev, work, p)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples, (k_tc_update<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                                   lut_dev, ea_dev, boards, n, prev, has_prev_dev, action_out_dev,
                                   delta_out_dev, work, p)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
