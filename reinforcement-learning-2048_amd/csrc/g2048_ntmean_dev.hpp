// g2048_ntmean_dev.hpp -- the batch-mean step, shared by the six libraries that run it:
// g2048_ntmean.hip, g2048_stagemean.hip, g2048_ntmeantc.hip, g2048_stagemeantc.hip,
// g2048_stagedelay.hip and g2048_stageback.hip.  One copy, so the owner exchange cannot drift
// between them.
//   device  the (D, C) gather (k_mean_gather) and the apply with its owner exchange
//           (k_mean_apply), each once, over two small by-value objects:
//             Index  how an entry index is formed: FlatIndex, entry(p, nib, t) alone, or
//                    g2048_ntstage_dev.hpp's StagedIndex, which adds stage(prev) * stride
//             Tail   what the owner of an entry does with m = floor(D / C): MeanTail adds m into
//                    the table, TcTail scales m by rate(E, A) and updates (E, A)
//           A library whose hits come from elsewhere (a ring, a trajectory) writes kernels of its
//           own around the same pieces: the gather table's hit and flush (gather_hit,
//           gather_flush), add_entry, apply_entry and the tails.
//   host    the three launches of a step (mean_step); the checks of acc and ea and their size
//           stand in g2048_ntuple_dev.hpp
// Header-only and internal to each library, as g2048_ntuple_dev.hpp: nothing here is exported.
//
// Why three launches.  An entry moves by floor(D / C) over ALL hits of the step, and nothing
// orders an add in one block against a read in another:
//   policy  k_policy<T, true> (or k_stage_policy<T, true>, which also promotes): writes action,
//           err and delta; never writes acc or ea, and lut only by promotion
//   gather  every hit re-forms its entry and adds (delta, 1) into acc; touches acc only
//   apply   one lane of the grid per distinct entry takes (D, C) out and moves the entry; never
//           reads lut.  Lane 0 of a board's group then commits prev / has_prev.
// Why acc moves only by atomics.  Everything in acc moves by device-scope atomics (the gather's
// adds, then the apply's exchanges), so no plain load ever has to see another block's atomic.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

// G2048_NTMEAN_SLOT_BITS, if defined, fixes log2 of the gather's LDS slots for every T (slot_bits)

namespace g2048 {
namespace nt {

using u64 = unsigned long long;

// The gather's and the apply's block: 128 boards, lane g of a board's group of 8.
constexpr int UBLOCK = 1024;

// log2 of the gather table's slots; a slot is 16 bytes (key, D sum, C sum: a block makes at most
// 1024 T hits, so its C fits 32 bits).  Measured.
template <int T>
constexpr int slot_bits() {
#ifdef G2048_NTMEAN_SLOT_BITS
    return G2048_NTMEAN_SLOT_BITS;
#else
    return T <= 1 ? 9 : T == 2 ? 10 : 12;
#endif
}

// the apply's table holds keys only (4 bytes a slot): room for every hit of a block at T <= 4
constexpr int APPLY_SLOT_BITS = 13;

// ------------------------------------------------------------------ the two policy objects
struct FlatIndex {
    __device__ __forceinline__ uint32_t base(const Board&) const { return 0u; }
};

struct MeanTail {
    __device__ __forceinline__ void operator()(uint32_t* table, uint32_t e, int64_t m) const {
        const uint32_t q = (uint32_t)m;  // additions modulo 2^32
        if (q != 0u) atomicAdd(&table[e], q);
    }
};

// ea needs no atomics.  An entry's (E, A) is touched by the lane that owns the entry and by no
// other: the exchange of C hands exactly one lane of the grid a non-zero C per entry per call (the
// gather's adds are complete before the apply starts, the launches being stream-ordered, and the
// first exchange leaves 0 for everyone after it), and the first two launches never take ea as an
// argument -- promotion copies the weight only.  That lane's load therefore sees what the previous
// call's owner stored -- a kernel boundary lies between them -- and nothing in this call can have
// changed it: "every read of ea sees the state before the call" holds by construction, and the
// store races with nothing.  Two stages' entries of one (t, i) are two keys, two owners and two
// (E, A).  One 16-byte load and one 16-byte store; |m| <= 2^31.
template <int RATE_BITS>
struct TcTail {
    longlong2* ea;
    __device__ __forceinline__ void operator()(uint32_t* table, uint32_t e, int64_t m) const {
        if (m == 0) return;
        const longlong2 s = ea[(size_t)e];
        const int64_t step = (m * (int64_t)tc_rate<RATE_BITS>(s.x, s.y)) >> RATE_BITS;
        if (step != 0) atomicAdd(&table[e], (uint32_t)step);
        ea[(size_t)e] = make_longlong2(s.x + m, s.y + (m < 0 ? -m : m));
    }
};

// ------------------------------------------------------------------ device: gather
// (D, C) of one entry into acc, straight to memory.  e < 2^30: 2 e + 1 reaches 2^31.
__device__ __forceinline__ void add_entry(u64* acc, uint32_t e, u64 d, u64 c) {
    if (d != 0ull) atomicAdd(&acc[2u * (size_t)e], d);
    atomicAdd(&acc[2u * (size_t)e + 1u], c);
}

// The gather's table, over the three LDS arrays the kernel declares (2^slot_bits<T>() slots each):
// per block the two sums of an entry are first merged in an LDS hash table and each used slot is
// flushed with two 64-bit atomic adds; a hit without a slot after four probes adds straight to
// memory.  A kernel clears the arrays, has every board-lane add its T hits (gather_hit) and
// flushes (gather_flush), with a barrier of its own on either side of the hits.  Only these two
// are functions: they compile to the text the kernels had with the code written out.  The clear,
// the loop over a lane's T entries and the apply's whole frame do not -- a function that holds
// them is simplified before it is inlined, and the kernel around it comes out in another order
// (profiles/tcfamily/README.md) -- so each kernel keeps those lines.
template <int T>
constexpr uint32_t gather_slots() {
    static_assert((16u << slot_bits<T>()) <= 160u * 1024u, "the LDS table must fit a CU's 160 KiB");
    return 1u << slot_bits<T>();
}

// one hit: (de, 1) into entry e
template <int T>
__device__ __forceinline__ void gather_hit(uint32_t* keys, uint32_t* csum, u64* dsum, u64* acc,
                                           uint32_t e, u64 de) {
    const uint32_t slot = claim_slot<slot_bits<T>()>(keys, e);
    if (slot != NO_SLOT) {
        atomicAdd(&dsum[slot], de);
        atomicAdd(&csum[slot], 1u);
    } else {
        add_entry(acc, e, de, 1ull);
    }
}

template <int T>
__device__ __forceinline__ void gather_flush(const uint32_t* keys, const uint32_t* csum,
                                             const u64* dsum, u64* acc) {
    for (uint32_t s = threadIdx.x; s < gather_slots<T>(); s += UBLOCK) {
        const uint32_t k = keys[s];
        if (k != NO_KEY) add_entry(acc, k, dsum[s], (u64)csum[s]);
    }
}

// 8 boards per wave, 128 per block: lane g re-forms its T entries of idx(prev, g, .).
template <int T, typename Index>
static __global__ __launch_bounds__(UBLOCK) void k_mean_gather(
    int64_t* __restrict__ acc_, int64_t n, const uint4* __restrict__ prev,
    const uint8_t* __restrict__ has_prev, const int32_t* __restrict__ delta, Params p, Index ix) {
    __shared__ uint32_t keys[gather_slots<T>()];
    __shared__ uint32_t csum[gather_slots<T>()];
    __shared__ u64 dsum[gather_slots<T>()];
    clear_keys<slot_bits<T>(), UBLOCK>(keys);
    for (uint32_t s = threadIdx.x; s < gather_slots<T>(); s += UBLOCK) {
        csum[s] = 0u;
        dsum[s] = 0ull;
    }
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * UBLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    u64* acc = reinterpret_cast<u64*>(acc_);  // additions modulo 2^64
    const int32_t d = i < n && has_prev[i] != 0 ? delta[i] : 0;
    if (d != 0) {
        const Board pb = load_board(prev, i);
        const uint32_t base = ix.base(pb);
        const uint64_t nib = nibbles(sym(pb, g));
        const u64 de = (u64)(int64_t)d;
#pragma unroll
        for (int t = 0; t < T; ++t)
            gather_hit<T>(keys, csum, dsum, acc, base + entry(p, nib, t), de);
    }
    __syncthreads();
    gather_flush<T>(keys, csum, dsum, acc);
}

// ------------------------------------------------------------------ device: apply
// floor(D / C), 1 <= C <= 8 n < 2^35: the truncating quotient, one lower where the remainder is
// negative
__device__ __forceinline__ int64_t floor_div(int64_t D, int64_t c) {
    int64_t q = D / c;
    if (D - q * c < 0) --q;
    return q;
}

// Several lanes of the grid ask for one entry (one per block that hit it, and every hit that
// found no slot).  The lane that takes the non-zero C out owns the entry: it takes D out too and
// hands m = floor(D / C) to the tail.
template <typename Tail>
__device__ __forceinline__ void apply_entry(uint32_t* table, u64* acc, uint32_t e, Tail tail) {
    const u64 c = atomicExch(&acc[2u * (size_t)e + 1u], 0ull);
    if (c == 0ull) return;
    const int64_t D = (int64_t)atomicExch(&acc[2u * (size_t)e], 0ull);
    tail(table, e, c == 1ull ? D : floor_div(D, (int64_t)c));
}

// The gather's frame: every hit re-forms its entry, and the LDS key table reduces a block's hits
// to one lane per distinct entry, which asks for it.  What the tail is made of (nothing, or ea)
// comes as kernel arguments of its own right behind acc, and the tail is built here: a kernel's
// leading pointer arguments arrive preloaded in SGPRs, a tail passed by value never would.
template <int T, typename Index, typename Tail, typename... TailArgs>
static __global__ __launch_bounds__(UBLOCK) void k_mean_apply(
    int32_t* __restrict__ lut, int64_t* __restrict__ acc_, TailArgs... tail_args,
    const uint4* __restrict__ boards, int64_t n, uint4* __restrict__ prev,
    uint8_t* __restrict__ has_prev, const uint8_t* __restrict__ action,
    const int32_t* __restrict__ delta, Params p, Index ix) {
    const Tail tail{tail_args...};
    constexpr uint32_t SLOTS = 1u << APPLY_SLOT_BITS;
    __shared__ uint32_t keys[SLOTS];
    clear_keys<APPLY_SLOT_BITS, UBLOCK>(keys);
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * UBLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    const bool live = i < n;
    uint32_t* table = reinterpret_cast<uint32_t*>(lut);  // additions modulo 2^32
    u64* acc = reinterpret_cast<u64*>(acc_);
    const int32_t d = live && has_prev[i] != 0 ? delta[i] : 0;
    if (d != 0) {
        const Board pb = load_board(prev, i);
        const uint32_t base = ix.base(pb);
        const uint64_t nib = nibbles(sym(pb, g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = base + entry(p, nib, t);
            // a hit that finds no slot asks for the entry itself
            if (claim_slot<APPLY_SLOT_BITS>(keys, e) == NO_SLOT) apply_entry(table, acc, e, tail);
        }
    }
    // every read of prev[i] and has_prev[i], stage_of(prev) included, lies before this barrier,
    // lane 0's stores after it
    __syncthreads();
    // One slot after the other.  Tried: a lane's eight exchanges of C in flight together, then
    // its exchanges of D -- equal at 65 536 boards, slower at 4 096.
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s];
        if (k != NO_KEY) apply_entry(table, acc, k, tail);
    }
    if (live && g == 0u) commit_prev(boards, i, action, prev, has_prev);
}

// ------------------------------------------------------------------ host
// the TD policy launch that goes with an index; g2048_ntstage_dev.hpp has StagedIndex's
template <int T>
inline void launch_td_policy(const FlatIndex&, hipStream_t st, int32_t* lut, const uint4* boards,
                             int64_t n, const uint4* prev, const uint8_t* has_prev, int32_t lr_num,
                             int32_t lr_shift, uint8_t* action, int32_t* delta, int64_t* err,
                             const Params& p) {
    k_policy<T, true><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
        lut, boards, n, action, prev, has_prev, lr_num, lr_shift, delta, err, p, nullptr, nullptr);
}

// The three launches of a step on the caller's device, after every argument has been checked.
// `g_err` is the library's message, which G_HIP writes.  launch_td_policy is an overload set over
// the index type: FlatIndex's is above, StagedIndex's stands next to StagedIndex in
// g2048_ntstage_dev.hpp and is found through its argument when mean_step is instantiated, so a
// source that passes a StagedIndex must include that header (it has to, to name the type).
// The tail's arguments (none, or ea) come last.
template <typename Tail, typename Index, typename... TailArgs>
inline int mean_step(std::string& g_err, const g2048_ntuple_spec& spec, Index ix,
                     int32_t* lut, int64_t* acc, const uint8_t* boards_dev, int64_t n,
                     uint8_t* prev_dev, uint8_t* has_prev, int32_t lr_num, int32_t lr_shift,
                     uint8_t* action, int32_t* delta, int64_t* err, int device_id, void* stream,
                     TailArgs... tail_args) {
    const Params p = make_params(spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* prev = reinterpret_cast<uint4*>(prev_dev);
    const dim3 grid = grid_for(n, UBLOCK / 8);
    DISPATCH_T(spec.n_tuples, (launch_td_policy<TT>(ix, st, lut, boards, n, prev, has_prev, lr_num,
                                                    lr_shift, action, delta, err, p)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec.n_tuples, (k_mean_gather<TT><<<grid, dim3(UBLOCK), 0, st>>>(
                                  acc, n, prev, has_prev, delta, p, ix)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec.n_tuples,
               (k_mean_apply<TT, Index, Tail, TailArgs...><<<grid, dim3(UBLOCK), 0, st>>>(
                   lut, acc, tail_args..., boards, n, prev, has_prev, action, delta, p, ix)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // namespace nt
}  // namespace g2048
