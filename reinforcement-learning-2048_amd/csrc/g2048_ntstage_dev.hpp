// g2048_ntstage_dev.hpp -- the stage rule of include/g2048_ntstage.h, shared by the libraries
// that read a staged table: g2048_ntstage.hip, g2048_stagesearch.hip, g2048_stagemean.hip,
// g2048_stagemeantc.hip, g2048_stagedelay.hip and g2048_stageback.hip.  One copy, so they cannot
// drift.
//   device  M(b) on the board in registers (max_tile), stage(b) against the bounds bytes of the
//           params struct (stage_of); the staged entry index of the batch-mean kernels
//           (StagedIndex); the learners' fall-through, a wave vote over one or two sets of T
//           entries (resolve); the promotion store of every staged TD policy (promote); the
//           staged policy kernel (k_stage_policy: act, and the first launch of the staged TD
//           steps that keep prev / has_prev)
//   host    the validation of a stage spec (check_stages, check_staged), the params struct
//           (StageParams, make_stage_params), and what the staged batch-mean libraries' entry
//           points open with (staged_acc_bytes, check_staged_tc)
// Below the root the search keeps a fall-through of its own, a per-lane loop over a burst
// (g2048_stageleaf_dev.hpp's StagedLeaf); at depth 1, where whole waves reach the leaf, it calls
// resolve.  It instantiates no kernel template of this header.
// Header-only and internal to each library, as g2048_ntuple_dev.hpp: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/g2048_ntstage.h"
#include "../../include/g2048_ntuple.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

namespace g2048 {
namespace nt {

constexpr int MAXS = G2048_NTSTAGE_MAX_STAGES;
constexpr int32_t UNSET = G2048_NTSTAGE_UNSET;

struct StageParams {
    uint32_t stride;    // T * 16^m, the entries of one stage
    uint32_t n_stages;  // S
    uint64_t bounds;    // byte k = bounds[k] for k < S - 1, 255 (above any exponent) past that
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 pairs(uint32_t w) { return __builtin_bit_cast(u16x2, w); }

// M(b): the largest exponent byte.  Even and odd bytes as 16-bit pairs, a packed max over the
// eight words, then the larger half.
__device__ __forceinline__ uint32_t max_tile(const Board& b) {
    constexpr uint32_t EVEN = 0x00FF00FFu;
    u16x2 m = __builtin_elementwise_max(pairs(b.r0 & EVEN), pairs((b.r0 >> 8) & EVEN));
    m = __builtin_elementwise_max(m, pairs(b.r1 & EVEN));
    m = __builtin_elementwise_max(m, pairs((b.r1 >> 8) & EVEN));
    m = __builtin_elementwise_max(m, pairs(b.r2 & EVEN));
    m = __builtin_elementwise_max(m, pairs((b.r2 >> 8) & EVEN));
    m = __builtin_elementwise_max(m, pairs(b.r3 & EVEN));
    m = __builtin_elementwise_max(m, pairs((b.r3 >> 8) & EVEN));
    const uint32_t w = __builtin_bit_cast(uint32_t, m);
    return max(w & 0xFFFFu, w >> 16);
}

// stage(b): the number of bounds that M(b) reaches
__device__ __forceinline__ uint32_t stage_of(const Board& b, const StageParams& sp) {
    const uint32_t m = max_tile(b);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < MAXS - 1; ++k) s += m >= ((uint32_t)(sp.bounds >> (8 * k)) & 0xFFu) ? 1u : 0u;
    return s;
}

// The batch-mean kernels' entry index on a staged table: stage(prev) * stride is added to
// entry(p, nib, t).  The sum is < 2^30, so NO_KEY stays free.
struct StagedIndex {
    StageParams sp;
    __device__ __forceinline__ uint32_t base(const Board& prev) const {
        return stage_of(prev, sp) * sp.stride;
    }
};

// The fall-through: v[t] holds lut[e[t]] of a lane at stage s (0 in a lane that gathers
// nothing).  Round r reads the entry r stages down for every value still UNSET in a lane with
// s >= r; what is UNSET at stage 0 is 0.  With TWO a second set (pe, pv, ps) shares the rounds.
// Called by whole waves: the loop's exit is a wave vote.
template <int T, bool TWO, typename LUT>
__device__ __forceinline__ void resolve(LUT lut, const StageParams& sp, const uint32_t (&e)[T],
                                        int32_t (&v)[T], uint32_t s, const uint32_t (&pe)[T],
                                        int32_t (&pv)[T], uint32_t ps) {
    for (uint32_t r = 1; r < sp.n_stages; ++r) {
        bool need = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if constexpr (TWO) need |= (v[t] == UNSET && s >= r) || (pv[t] == UNSET && ps >= r);
            else need |= v[t] == UNSET && s >= r;
        }
        if (!__any(need)) break;
        const uint32_t down = r * sp.stride;
        int32_t w[T], pw[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            w[t] = (v[t] == UNSET && s >= r) ? lut[e[t] - down] : v[t];
            if constexpr (TWO) pw[t] = (pv[t] == UNSET && ps >= r) ? lut[pe[t] - down] : pv[t];
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            v[t] = w[t];
            if constexpr (TWO) pv[t] = pw[t];
        }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        v[t] = v[t] == UNSET ? 0 : v[t];
        if constexpr (TWO) pv[t] = pv[t] == UNSET ? 0 : pv[t];
    }
}

// ------------------------------------------------------------------ device: promotion
// The promotion store, shared by the staged TD policies (k_stage_policy<T, true> here,
// k_delay_policy, k_back_policy).  Each kernel forms and loads its two sets of T entries, takes
// the mask of the UNSET ones and sums the values itself: a function that holds those loops is
// simplified before it is inlined (the loads of Params move to the kernel's entry, the sums
// associate another way) and the kernel comes out in another order, act's instantiation
// included (profiles/tcfamily/README.md).
// Promotion: the value the entry resolves to, into the entries that `unset` names (0 in a lane
// that promotes nothing).
// Promotion needs no ordering.  The only table words the launch writes are UNSET entries, each
// with the value it resolves to in the pre-call table, so any lane that reads one, before or after
// the store, resolves to the same number, and two lanes that promote one entry store the same
// number.  Every entry a later launch of the step adds into was promoted here, so those launches
// never land on UNSET and never read the table.
template <int T>
__device__ __forceinline__ void promote(int32_t* lut, const uint32_t (&e)[T],
                                        const int32_t (&v)[T], uint32_t unset) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        if ((unset >> t) & 1u) lut[e[t]] = v[t];
}

// The table pointer of the policy kernel: read-only for act; the TD step's launch writes the
// promoted entries, so there the const and the __restrict__ go.
template <bool TD>
using PolicyLut = std::conditional_t<TD, int32_t*, const int32_t* __restrict__>;

// k_policy (g2048_ntuple_dev.hpp) at the AFTERSTATE's stage.  With TD the groups a == 0 also
// gather V(prev) at stage(prev) in the same fall-through rounds and store the promoted values,
// and the launch writes action, delta and err only: q_out and after_out are not looked at,
// action_out is not null.
template <int T, bool TD>
static __global__ __launch_bounds__(POLICY_BLOCK) void k_stage_policy(
    PolicyLut<TD> lut, const uint4* __restrict__ boards, int64_t n,
    uint8_t* __restrict__ action_out, const uint4* __restrict__ prev,
    const uint8_t* __restrict__ has_prev, int32_t lr_num, int32_t lr_shift,
    int32_t* __restrict__ delta_out, int64_t* __restrict__ err_out, Params p, StageParams sp,
    int64_t* __restrict__ q_out, uint4* __restrict__ after_out) {
    const PolicyLane l = policy_lane<POLICY_BLOCK>(boards, n);
    const uint32_t st = stage_of(l.s, sp);  // the afterstate's stage: a merge can raise it
    uint32_t e[T], pe[T];
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) e[t] = st * sp.stride + entry(p, l.nib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[e[t]] : 0;
    bool hp = false, mine = false;  // mine: this lane gathers (and promotes) prev's entries
    uint32_t pst = 0, unset = 0;
    if constexpr (TD) {
        hp = has_prev[l.bi] != 0;
        mine = hp && l.a == 0u;
        const Board pb = load_board(prev, l.bi);
        pst = stage_of(pb, sp);
        const uint64_t pnib = nibbles(sym(pb, l.g));
#pragma unroll
        for (int t = 0; t < T; ++t) pe[t] = pst * sp.stride + entry(p, pnib, t);
#pragma unroll
        for (int t = 0; t < T; ++t) pv[t] = mine ? lut[pe[t]] : 0;
#pragma unroll
        for (int t = 0; t < T; ++t) unset |= pv[t] == UNSET ? 1u << t : 0u;
        resolve<T, true>(lut, sp, e, v, st, pe, pv, pst);
    } else {
        resolve<T, false>(lut, sp, e, v, st, e, v, st);
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
        // `unset` is 0 outside the groups a == 0 of boards with has_prev
        promote(lut, pe, pv, unset);
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

// the TD policy launch that goes with StagedIndex (g2048_ntmean_dev.hpp's mean_step calls it)
template <int T>
inline void launch_td_policy(const StagedIndex& ix, hipStream_t st, int32_t* lut,
                             const uint4* boards, int64_t n, const uint4* prev,
                             const uint8_t* has_prev, int32_t lr_num, int32_t lr_shift,
                             uint8_t* action, int32_t* delta, int64_t* err, const Params& p) {
    k_stage_policy<T, true><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
        lut, boards, n, action, prev, has_prev, lr_num, lr_shift, delta, err, p, ix.sp, nullptr,
        nullptr);
}

inline int check_stages(std::string& err, const char* who, const g2048_ntstage_spec* stages) {
    if (stages == nullptr) return refuse(err, "%s: stages is NULL", who);
    const int S = stages->n_stages;
    if (S < 1 || S > MAXS) return refuse(err, "%s: n_stages = %d outside [1, %d]", who, S, MAXS);
    for (int k = 0; k < MAXS - 1; ++k) {
        const int b = stages->bounds[k];
        if (k >= S - 1) {
            if (b != 0)
                return refuse(err, "%s: unused bound %d = %d must be 0 (n_stages = %d)", who, k,
                              b, S);
            continue;
        }
        if (b < 1 || b > G2048_NTSTAGE_MAX_BOUND)
            return refuse(err, "%s: bound %d = %d outside [1, %d]", who, k, b,
                          G2048_NTSTAGE_MAX_BOUND);
        if (k > 0 && b <= stages->bounds[k - 1])
            return refuse(err, "%s: bounds must be strictly increasing (bound %d = %d after %d)",
                          who, k, b, stages->bounds[k - 1]);
    }
    return G2048_OK;
}

// the spec, the stage spec and the rest of check_common
inline int check_staged(std::string& err, const char* who, const g2048_ntuple_spec* spec,
                        const g2048_ntstage_spec* stages, const int32_t* lut,
                        const uint8_t* boards, int64_t n) {
    int rc = check_spec(err, who, spec);
    if (rc != G2048_OK) return rc;
    rc = check_stages(err, who, stages);
    if (rc != G2048_OK) return rc;
    return check_common(err, who, spec, lut, boards, n);
}

// what every exported *_acc_bytes of a staged library returns
inline int64_t staged_acc_bytes(std::string& err, const char* who, const g2048_ntuple_spec* spec,
                                const g2048_ntstage_spec* stages) {
    int rc = check_spec(err, who, spec);
    if (rc != G2048_OK) return rc;
    rc = check_stages(err, who, stages);
    if (rc != G2048_OK) return rc;
    return table_bytes(*spec, stages->n_stages);
}

// check_staged, then acc and ea beside the staged table: how every staged mean-TC step opens
inline int check_staged_tc(std::string& err, const char* who, const g2048_ntuple_spec* spec,
                           const g2048_ntstage_spec* stages, const int32_t* lut,
                           const uint8_t* boards, int64_t n, const int64_t* acc,
                           const int64_t* ea) {
    int rc = check_staged(err, who, spec, stages, lut, boards, n);
    if (rc != G2048_OK) return rc;
    rc = check_acc(err, who, acc);
    if (rc != G2048_OK) return rc;
    return check_ea(err, who, ea, acc, table_bytes(*spec, stages->n_stages));
}

inline StageParams make_stage_params(const g2048_ntuple_spec& spec,
                                     const g2048_ntstage_spec& stages) {
    StageParams sp = {};
    sp.stride = (uint32_t)spec.n_tuples << (4 * spec.n_cells);
    sp.n_stages = (uint32_t)stages.n_stages;
    for (int k = 0; k < MAXS; ++k)
        sp.bounds |= (uint64_t)(k < stages.n_stages - 1 ? stages.bounds[k] : 255u) << (8 * k);
    return sp;
}

}  // namespace nt
}  // namespace g2048
