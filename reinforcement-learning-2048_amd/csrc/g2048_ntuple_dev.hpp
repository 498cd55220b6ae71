// g2048_ntuple_dev.hpp -- what the two libraries that read an n-tuple table share
// (g2048_ntuple.hip -> libg2048_ntuple.so, g2048_ntsearch.hip -> libg2048_ntsearch.so): the
// device helpers that turn a board into table indices (include/g2048_ntuple.h: symmetries, the
// clamp to 15, idx) and the host-side validation of a spec and of the arguments every device
// entry point has.  Header-only and internal to each library: nothing here is exported, and the
// libraries do not link against each other.
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

// ------------------------------------------------------------------ host: validation
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

}  // namespace nt
}  // namespace g2048
