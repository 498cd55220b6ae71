// g2048_ntstage_dev.hpp -- the stage rule of include/g2048_ntstage.h, shared by the two libraries
// that read a staged table: g2048_ntstage.hip (libg2048_ntstage.so) and g2048_stagesearch.hip
// (libg2048_stagesearch.so).  One copy, so the two cannot drift.
//   device  M(b) on the board in registers (max_tile), stage(b) against the bounds bytes of the
//           params struct (stage_of)
//   host    the validation of a stage spec (check_stages) and the params struct (StageParams,
//           make_stage_params)
// The gathers and their fall-through stay in the kernels: the learner's rounds are a wave vote
// over one or two sets of T entries, the search's a per-lane loop over a burst.
// Header-only and internal to each library, as g2048_ntuple_dev.hpp: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

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
