// g2048_stageleaf_dev.hpp -- the leaf of the expectimax tree walk (g2048_ntsearch_dev.hpp) over a
// staged table, shared by the two libraries that search one: g2048_stagesearch.hip (a wave per
// board) and g2048_deepsearch.hip (a tree spread over many waves).  One copy, so the stage of a
// leaf and its fall-through cannot drift.
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
//       rounds ended by a vote: g2048_ntstage_dev.hpp's resolve, as in k_stage_policy.
// Header-only and internal to each library, as g2048_ntuple_dev.hpp: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntsearch_dev.hpp"

namespace g2048 {
namespace nt {

struct StagedLeaf {
    StageParams sp;

    struct At {
        uint32_t st, top;  // the leaf's stage and the first entry of that stage, st * stride
    };
    // stage(s), kept below S for any bytes: a board outside the domain (an exponent byte that
    // reaches the 255 of an unused bound) must not index past the table
    __device__ __forceinline__ At at(const Board& s) const {
        const uint32_t st = min(stage_of(s, sp), sp.n_stages - 1u);
        return At{st, st * sp.stride};
    }

    // the smallest of a burst's values: UNSET is INT32_MIN, so the burst holds an UNSET iff this
    // is UNSET (8 NT / 2 v_min3_i32 instead of a compare per value)
    template <int NT>
    static __device__ __forceinline__ int32_t smallest(const int32_t (&v)[NT][8]) {
        int32_t lo = v[0][0];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int g = 0; g < 8; ++g) lo = min(lo, v[j][g]);
        }
        return lo;
    }

    // 8 NT gathers at the leaf's stage, then -- only in a lane whose burst holds an UNSET -- the
    // fall-through rounds of that lane (t0 is wave-uniform, the stage and the rounds are not)
    template <int NT>
    __device__ __forceinline__ int64_t burst(const int32_t* __restrict__ lut, const Params& p,
                                             const uint64_t (&x)[8], int t0, At at) const {
        int32_t v[NT][8];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int g = 0; g < 8; ++g) v[j][g] = lut[at.top + entry(p, x[g], t0 + j)];
        }
        if (smallest<NT>(v) == UNSET) {
#pragma unroll 1
            for (uint32_t r = 1; r <= at.st; ++r) {
                const uint32_t base = at.top - r * sp.stride;  // r <= st: never below stage 0
                int32_t w[NT][8];
#pragma unroll
                for (int j = 0; j < NT; ++j) {
#pragma unroll
                    for (int g = 0; g < 8; ++g)
                        w[j][g] = v[j][g] == UNSET ? lut[base + entry(p, x[g], t0 + j)] : v[j][g];
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

    // k_stage_policy's lane: T loads in flight at the afterstate's stage.  A lane that gathers
    // nothing holds 0, never UNSET: it asks for no round.  The index sits behind the
    // wave-uniform t < T with its load (T indices, not MAXT).
    __device__ __forceinline__ int64_t first_ply(const int32_t* __restrict__ lut, const Params& p,
                                                 const Board& s, uint64_t nib, bool ok) const {
        const int T = (int)p.n_tuples;
        const At a = at(s);
        uint32_t e[MAXT];
        int32_t q[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            e[t] = 0u, q[t] = 0;
            if (t < T) {
                e[t] = a.top + entry(p, nib, t);
                q[t] = ok ? lut[e[t]] : 0;
            }
        }
        resolve<MAXT, false>(lut, sp, e, q, a.st, e, q, a.st);
        int64_t sum = 0;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) sum += q[t];
        return sum;
    }
};

}  // namespace nt
}  // namespace g2048
