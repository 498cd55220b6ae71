// g2048_stagemeantc.hip -- temporal-coherence learning on the batch-mean rule for the multi-stage
// n-tuple value network on gfx950 (libg2048_stagemeantc.so).
//
// The rule is defined in include/g2048_stagemeantc.h; every value is an integer and the result is
// checked bit for bit against tests/stagemeantc_ref.py.  No float anywhere.  The library takes the
// spec, the stage spec and the table of g2048_ntstage.h and does not link against another library
// of the project.  It composes three existing steps: the staged TD step's policy launch with its
// fall-through and promotion (g2048_ntstage.hip), the batch-mean step's (D, C) gather and exchange
// (g2048_ntmean.hip), and the temporal-coherence rate (g2048_nttc.hip).  The index helpers, the
// policy's lane decode, group sum, argmax, err / delta, the merge table's keys, the prev commit
// and the host plumbing come from g2048_ntuple_dev.hpp, the stage rule from
// g2048_ntstage_dev.hpp.  The fall-through loop, the gather / apply bodies, the floor division
// and the rate live inside those three .hip files, so they are restated here, each under a
// comment that names its original.
//
// A step is three launches, because an entry moves by floor(D / C) over ALL hits of the step and
// nothing orders an add in one block against a read in another:
//   k_smtc_policy  k_sm_policy's job unchanged (g2048_stagemean.hip): 2 boards per wave, lane
//                  32s + 8a + g evaluates after(board s, a) under symmetry g at the AFTERSTATE's
//                  stage; the groups a == 0 also gather V(prev) at stage(prev) in the same
//                  fall-through rounds and store the promoted values.  Writes action, err and
//                  delta.  The only table words it writes are UNSET entries, each with the value
//                  it resolves to in the pre-call table, so any lane that reads one, before or
//                  after the store, resolves to the same number, and two lanes that promote one
//                  entry store the same number: nothing has to be ordered inside the launch.
//   k_smtc_gather  k_sm_gather's job unchanged: 8 boards per wave, 128 per block: lane g re-forms
//                  its T staged entries stage(prev) * stride + entry(prev, g, .) (< 2^30, so
//                  NO_KEY stays free) and adds (delta, 1) into acc.  Per block the two sums of an
//                  entry are first merged in an LDS hash table and each used slot is flushed with
//                  two 64-bit atomic adds; a hit without a slot after four probes adds straight
//                  to memory.
//   k_smtc_apply   k_sm_apply's frame with k_mtc_apply's owner tail (g2048_ntmeantc.hip): the LDS
//                  key table reduces a block's hits to one lane per distinct staged entry, and
//                  that lane exchanges C with 0.  The one lane of the grid that gets a non-zero C
//                  back owns the entry: it exchanges D with 0, forms m = floor(D / C) and, if
//                  m != 0, loads (E, A) of the STAGED entry, computes rate and step, adds step
//                  into lut and stores (E + m, A + |m|).  The first launch promoted every entry a
//                  hit can address, so the add never lands on UNSET and this launch never reads
//                  lut.  Lane 0 of a board's group then commits prev / has_prev.
// The second launch touches acc only, the third never reads lut.  Everything in acc moves by
// device-scope atomics (adds, then exchanges), so no plain load ever has to see another block's
// atomic.
//
// ea needs no atomics.  A staged entry's (E, A) is touched by the lane that owns the entry and by
// no other: the exchange of C hands exactly one lane of the grid a non-zero C per staged entry
// per call (the gather's adds are complete before the apply starts, the launches being
// stream-ordered, and the first exchange leaves 0 for everyone after it), and the first two
// launches never take ea as an argument -- promotion copies the weight only, so the policy launch
// has no business with it.  That lane's load therefore sees what the previous call's owner stored
// -- a kernel boundary lies between them -- and nothing in this call can have changed it: "every
// read of ea sees the state before the call" holds by construction, and the store races with
// nothing.  Two stages' entries of one (t, i) are two keys, two owners and two (E, A).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stagemeantc.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

using u64 = unsigned long long;

constexpr int RATE_BITS = G2048_STAGEMEANTC_RATE_BITS;

// tc_rate of g2048_nttc.hip, restated: rate(E, A) of the header.  In the domain (|E| <= A < 2^62)
// both shifted operands are below 2^16 and the divisor is at least 1: a 32-bit unsigned division.
__host__ __device__ __forceinline__ uint32_t tc_rate(int64_t E, int64_t A) {
    if (A == 0) return 1u << RATE_BITS;
    const uint64_t a = (uint64_t)A, e = E < 0 ? 0ull - (uint64_t)E : (uint64_t)E;
    const int bits = 64 - __builtin_clzll(a);
    const int s = bits > RATE_BITS ? bits - RATE_BITS : 0;
    const uint32_t num = (uint32_t)(e >> s) << RATE_BITS, den = (uint32_t)(a >> s);
    return num / den;
}

constexpr int BLOCK = 256;

// The fall-through of g2048_ntstage.hip (`resolve` with TWO = true), restated: v[t] holds
// lut[e[t]] of a lane at stage s, pv[t] holds lut[pe[t]] at stage ps (0 in a lane that gathers
// nothing).  Round r reads the entry r stages down for every value still UNSET in a lane whose
// stage is >= r; what is UNSET at stage 0 is 0.  The two sets share the rounds.  Called by whole
// waves: the loop's exit is a wave vote.
template <int T>
__device__ __forceinline__ void resolve2(const int32_t* lut, const StageParams& sp,
                                         const uint32_t (&e)[T], int32_t (&v)[T], uint32_t s,
                                         const uint32_t (&pe)[T], int32_t (&pv)[T], uint32_t ps) {
    for (uint32_t r = 1; r < sp.n_stages; ++r) {
        bool need = false;
#pragma unroll
        for (int t = 0; t < T; ++t)
            need |= (v[t] == UNSET && s >= r) || (pv[t] == UNSET && ps >= r);
        if (!__any(need)) break;
        const uint32_t down = r * sp.stride;
        int32_t w[T], pw[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            w[t] = (v[t] == UNSET && s >= r) ? lut[e[t] - down] : v[t];
            pw[t] = (pv[t] == UNSET && ps >= r) ? lut[pe[t] - down] : pv[t];
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            v[t] = w[t];
            pv[t] = pw[t];
        }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        v[t] = v[t] == UNSET ? 0 : v[t];
        pv[t] = pv[t] == UNSET ? 0 : pv[t];
    }
}

// k_stage_policy<T, true> of g2048_ntstage.hip with the TD outputs only, restated.  The table is
// read and the promoted entries are written in one launch: no const, no __restrict__.  ea is not
// an argument: promotion copies the weight only.
template <int T>
__global__ __launch_bounds__(BLOCK) void k_smtc_policy(
    int32_t* lut, const uint4* __restrict__ boards, int64_t n, uint8_t* __restrict__ action_out,
    const uint4* __restrict__ prev, const uint8_t* __restrict__ has_prev, int32_t lr_num,
    int32_t lr_shift, int32_t* __restrict__ delta_out, int64_t* __restrict__ err_out, Params p,
    StageParams sp) {
    const PolicyLane l = policy_lane<BLOCK>(boards, n);
    const uint32_t st = stage_of(l.s, sp);  // the afterstate's stage: a merge can raise it
    uint32_t e[T], pe[T];
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) e[t] = st * sp.stride + entry(p, l.nib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[e[t]] : 0;
    const bool hp = has_prev[l.bi] != 0;
    const bool mine = hp && l.a == 0u;  // this lane gathers (and promotes) prev's entries
    const Board pb = load_board(prev, l.bi);
    const uint32_t pst = stage_of(pb, sp);
    const uint64_t pnib = nibbles(sym(pb, l.g));
    uint32_t unset = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) pe[t] = pst * sp.stride + entry(p, pnib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) pv[t] = mine ? lut[pe[t]] : 0;
#pragma unroll
    for (int t = 0; t < T; ++t) unset |= pv[t] == UNSET ? 1u << t : 0u;
    resolve2<T>(lut, sp, e, v, st, pe, pv, pst);
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const Best m = best_move<8>(l.ok ? ((int64_t)l.gain << F) + sum : INT64_MIN, l.lane);
#pragma unroll
    for (int t = 0; t < T; ++t) psum += pv[t];
    psum = group_sum(psum);  // V(prev) in the group a == 0
    if (!l.live) return;
    // promotion: the value the entry resolves to, into the entries this lane found UNSET.
    // `unset` is 0 outside the groups a == 0 of boards with has_prev.
#pragma unroll
    for (int t = 0; t < T; ++t)
        if ((unset >> t) & 1u) lut[pe[t]] = pv[t];
    if ((l.lane & 31u) == 0u) {
        const TdError td = td_error(m.best, psum, hp, l.legal, lr_num, lr_shift);
        action_out[l.i] = (uint8_t)m.act;
        delta_out[l.i] = td.delta;
        if (err_out != nullptr) err_out[l.i] = td.err;
    }
}

// The gather's and the apply's block: 128 boards, lane g of a board's group of 8.
constexpr int UBLOCK = 1024;

// log2 of the gather table's slots; a slot is 16 bytes (key, D sum, C sum: a block makes at most
// 1024 T hits, so its C fits 32 bits).  g2048_ntmean.hip's measured counts.
template <int T>
constexpr int slot_bits() {
    return T <= 1 ? 9 : T == 2 ? 10 : 12;
}

// the apply's table holds keys only (4 bytes a slot): room for every hit of a block at T <= 4
constexpr int APPLY_SLOT_BITS = 13;

// (D, C) of one staged entry into acc, straight to memory (g2048_ntmean.hip's add_entry).
// e < 2^30: 2 e + 1 reaches 2^31.
__device__ __forceinline__ void add_entry(u64* acc, uint32_t e, u64 d, u64 c) {
    if (d != 0ull) atomicAdd(&acc[2u * (size_t)e], d);
    atomicAdd(&acc[2u * (size_t)e + 1u], c);
}

// k_mean_gather of g2048_ntmean.hip, restated with the staged entry index.
template <int T>
__global__ __launch_bounds__(UBLOCK) void k_smtc_gather(
    int64_t* __restrict__ acc_, int64_t n, const uint4* __restrict__ prev,
    const uint8_t* __restrict__ has_prev, const int32_t* __restrict__ delta, Params p,
    StageParams sp) {
    constexpr int SLOT_BITS = slot_bits<T>();
    constexpr uint32_t SLOTS = 1u << SLOT_BITS;
    static_assert(SLOTS * 16u <= 160u * 1024u, "the LDS table must fit a CU's 160 KiB");
    __shared__ uint32_t keys[SLOTS];
    __shared__ uint32_t csum[SLOTS];
    __shared__ u64 dsum[SLOTS];
    clear_keys<SLOT_BITS, UBLOCK>(keys);
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
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
        const uint32_t base = stage_of(pb, sp) * sp.stride;
        const uint64_t nib = nibbles(sym(pb, g));
        const u64 de = (u64)(int64_t)d;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = base + entry(p, nib, t);
            const uint32_t slot = claim_slot<SLOT_BITS>(keys, e);
            if (slot != NO_SLOT) {
                atomicAdd(&dsum[slot], de);
                atomicAdd(&csum[slot], 1u);
            } else {
                add_entry(acc, e, de, 1ull);
            }
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s];
        if (k != NO_KEY) add_entry(acc, k, dsum[s], (u64)csum[s]);
    }
}

// floor(D / C), 1 <= C <= 8 n < 2^35: the truncating quotient, one lower where the remainder is
// negative (g2048_ntmean.hip's floor_div, kept in 64 bits: |m| <= 2^31)
__device__ __forceinline__ int64_t floor_div(int64_t D, int64_t c) {
    int64_t q = D / c;
    if (D - q * c < 0) --q;
    return q;
}

// Several lanes of the grid ask for one staged entry (one per block that hit it, and every hit
// that found no slot).  The lane that takes the non-zero C out owns the entry (g2048_ntmean.hip's
// apply_entry up to the quotient); the tail is g2048_ntmeantc.hip's: the owner alone reads and
// writes the staged entry's (E, A), with one 16-byte load and one 16-byte store (see the head of
// this file).  e < 2^30 and ea[e] is 16 bytes: the pointer arithmetic on longlong2* is in size_t,
// as is acc's, where 2 e + 1 reaches 2^31.
__device__ __forceinline__ void apply_entry(uint32_t* table, u64* acc, longlong2* ea,
                                            uint32_t e) {
    const u64 c = atomicExch(&acc[2u * (size_t)e + 1u], 0ull);
    if (c == 0ull) return;
    const int64_t D = (int64_t)atomicExch(&acc[2u * (size_t)e], 0ull);
    const int64_t m = c == 1ull ? D : floor_div(D, (int64_t)c);
    if (m == 0) return;
    const longlong2 s = ea[(size_t)e];
    const int64_t step = (m * (int64_t)tc_rate(s.x, s.y)) >> RATE_BITS;
    if (step != 0) atomicAdd(&table[e], (uint32_t)step);
    ea[(size_t)e] = make_longlong2(s.x + m, s.y + (m < 0 ? -m : m));
}

// k_mean_apply of g2048_ntmean.hip, restated with the staged entry index and the owner's longer
// tail.
template <int T>
__global__ __launch_bounds__(UBLOCK) void k_smtc_apply(
    int32_t* __restrict__ lut, int64_t* __restrict__ acc_, longlong2* __restrict__ ea,
    const uint4* __restrict__ boards, int64_t n, uint4* __restrict__ prev,
    uint8_t* __restrict__ has_prev, const uint8_t* __restrict__ action,
    const int32_t* __restrict__ delta, Params p, StageParams sp) {
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
        const uint32_t base = stage_of(pb, sp) * sp.stride;
        const uint64_t nib = nibbles(sym(pb, g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = base + entry(p, nib, t);
            // a hit that finds no slot asks for the entry itself
            if (claim_slot<APPLY_SLOT_BITS>(keys, e) == NO_SLOT) apply_entry(table, acc, ea, e);
        }
    }
    // every read of prev[i] and has_prev[i], stage_of(prev) included, lies before this barrier,
    // lane 0's stores after it
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s];
        if (k != NO_KEY) apply_entry(table, acc, ea, k);
    }
    if (live && g == 0u) commit_prev(boards, i, action, prev, has_prev);
}

thread_local std::string g_err;

// the spec, the stage spec and the rest of check_common (g2048_ntstage.hip's check_staged)
int check_staged(const char* who, const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                 const int32_t* lut, const uint8_t* boards, int64_t n) {
    int rc = check_spec(g_err, who, spec);
    if (rc != G2048_OK) return rc;
    rc = check_stages(g_err, who, stages);
    if (rc != G2048_OK) return rc;
    return check_common(g_err, who, spec, lut, boards, n);
}

// bytes of acc, and of ea: 16 per staged entry
int64_t table_bytes(const g2048_ntuple_spec& spec, const g2048_ntstage_spec& stages) {
    return (int64_t)stages.n_stages * ((int64_t)spec.n_tuples << (4 * spec.n_cells)) * 2 *
           (int64_t)sizeof(int64_t);
}

}  // namespace

extern "C" {

const char* g2048_stagemeantc_last_error(void) { return g_err.c_str(); }

int32_t g2048_stagemeantc_rate(int64_t E, int64_t A) {
    if (A < 0 || A > G2048_STAGEMEANTC_MAX_A)
        return refuse(g_err, "stagemeantc_rate: A = %lld outside [0, 2^62)", (long long)A);
    if (E > A || E < -A)
        return refuse(g_err, "stagemeantc_rate: |E| = |%lld| exceeds A = %lld", (long long)E,
                      (long long)A);
    return (int32_t)tc_rate(E, A);
}

int64_t g2048_stagemeantc_acc_bytes(const g2048_ntuple_spec* spec,
                                    const g2048_ntstage_spec* stages) {
    const char* who = "stagemeantc_acc_bytes";
    int rc = check_spec(g_err, who, spec);
    if (rc != G2048_OK) return rc;
    rc = check_stages(g_err, who, stages);
    if (rc != G2048_OK) return rc;
    return table_bytes(*spec, *stages);
}

int g2048_stagemeantc_step(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                           int32_t* lut_dev, int64_t* acc_dev, int64_t* ea_dev,
                           const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                           uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                           uint8_t* action_out_dev, int32_t* delta_out_dev, int64_t* err_out_dev,
                           int device_id, void* stream) {
    const char* who = "stagemeantc_step";
    int rc = check_staged(who, spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (acc_dev == nullptr) return refuse(g_err, "stagemeantc_step: acc_dev is NULL");
    if (((uintptr_t)acc_dev & 15u) != 0)
        return refuse(g_err, "stagemeantc_step: acc_dev must be 16-byte aligned");
    if (ea_dev == nullptr) return refuse(g_err, "stagemeantc_step: ea_dev is NULL");
    if (((uintptr_t)ea_dev & 15u) != 0)
        return refuse(g_err, "stagemeantc_step: ea_dev must be 16-byte aligned");
    {
        // acc and ea are two tables of table_bytes each: the same one, or two that share a part,
        // would hand the exchanges of (D, C) a staged entry's (E, A)
        const uintptr_t a = (uintptr_t)acc_dev, b = (uintptr_t)ea_dev;
        const uintptr_t gap = a < b ? b - a : a - b;
        if (gap < (uintptr_t)table_bytes(*spec, *stages))
            return refuse(g_err, "stagemeantc_step: ea_dev overlaps acc_dev");
    }
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    const Params p = make_params(*spec);
    const StageParams sp = make_stage_params(*spec, *stages);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* prev = reinterpret_cast<uint4*>(prev_dev);
    longlong2* ea = reinterpret_cast<longlong2*>(ea_dev);
    DISPATCH_T(spec->n_tuples,
               (k_smtc_policy<TT><<<grid_for(n, BLOCK / 32), dim3(BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, prev, has_prev_dev, lr_num, lr_shift,
                   delta_out_dev, err_out_dev, p, sp)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples,
               (k_smtc_gather<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                   acc_dev, n, prev, has_prev_dev, delta_out_dev, p, sp)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples,
               (k_smtc_apply<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                   lut_dev, acc_dev, ea, boards, n, prev, has_prev_dev, action_out_dev,
                   delta_out_dev, p, sp)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
