// g2048_search.hip -- batched expectimax search player for gfx950 (libg2048_search.so).
//
// The search is defined in include/g2048_search.h; every value is an int64 and the result is
// checked bit for bit against tests/expectimax_ref.py.
//
// One wavefront per board (grid-stride over boards).  The first ply has 4 moves x 16 spawn cells
// = 64 children: lane 16a + c owns move a and spawn cell c, slides the root board by a, and -- if
// a is legal and cell c of the slid board is empty -- evaluates its two spawned boards (a 2 and a
// 4 at c) to depth - 1 by a per-lane recursion whose depth is a template parameter, so it lives
// in registers (no stack, no LDS).  The 16 lanes of a move sum their weighted values within their
// row, one floor division finishes the chance node, and the four root values are read from lanes
// 0 / 16 / 32 / 48.
//
// Board arithmetic is g2048_board.hpp's (line-parallel slide, SWAR legal mask).  The heuristic's
// byte sums are v_sad_u8 on the row words and on the transposed board:
//   Sm  = the 3 row-to-row SADs + the 3 column-to-column SADs
//   Mo  = (Sm - SAD(row 0, row 3) - SAD(col 0, col 3)) / 2
// because along one line inc + dec = sum |e_{k+1} - e_k| and inc - dec = e_3 - e_0 (telescoping),
// so min(inc, dec) = (sum |d_k| - |e_3 - e_0|) / 2.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/g2048_search.h"
#include "g2048_board.hpp"

namespace {

using namespace g2048;

struct Params {
    int32_t gain, empty, smooth, mono, corner, lost;
    int32_t c2, c4, W;  // chance weights of a 2 (W - w4) and of a 4 (w4); W
};

// byte-wise max of two words whose bytes are < 128: (x | 0x80) - y keeps bit 7 iff x >= y and
// never borrows across bytes
__device__ __forceinline__ uint32_t bmax(uint32_t x, uint32_t y) {
    return bsel(expand80(((x | K80) - y) & K80), x, y);
}

__device__ __forceinline__ uint32_t sad(uint32_t a, uint32_t b, uint32_t acc) {
    return __builtin_amdgcn_sad_u8(a, b, acc);
}

// bit 4r + c set iff cell (r, c) is empty
__device__ __forceinline__ uint32_t empty_mask(const Board& b) {
    // 0x80 flags of rows 0..3 moved to bits 7-k of each byte, then the four bytes' nibbles
    const uint32_t z = (z80(b.r0) >> 7) | (z80(b.r1) >> 6) | (z80(b.r2) >> 5) | (z80(b.r3) >> 4);
    // byte c of z holds bit r for cell (r, c); gather bit r of byte c into bit 4r + c
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t w = z >> r;  // bit 8c = cell (r, c)
        m |= ((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (4u * r);
    }
    return m;
}

__device__ __forceinline__ int64_t heuristic(const Board& b, const Params& p) {
    const Board t = transpose(b);
    const uint32_t zf = z80(b.r0) | (z80(b.r1) >> 1) | (z80(b.r2) >> 2) | (z80(b.r3) >> 3);
    const int32_t E = __popc(zf);
    uint32_t sm = sad(b.r0, b.r1, 0u);
    sm = sad(b.r1, b.r2, sm);
    sm = sad(b.r2, b.r3, sm);
    sm = sad(t.r0, t.r1, sm);
    sm = sad(t.r1, t.r2, sm);
    sm = sad(t.r2, t.r3, sm);
    const uint32_t ends = sad(b.r0, b.r3, sad(t.r0, t.r3, 0u));
    const int32_t Sm = (int32_t)sm, Mo = (int32_t)((sm - ends) >> 1);
    const uint32_t m = bmax(bmax(b.r0, b.r1), bmax(b.r2, b.r3));
    const uint32_t mx = max(max(m & 0xFFu, (m >> 8) & 0xFFu), max((m >> 16) & 0xFFu, m >> 24));
    const uint32_t cm = max(max(b.r0 & 0xFFu, b.r0 >> 24), max(b.r3 & 0xFFu, b.r3 >> 24));
    const int32_t C = cm == mx ? (int32_t)mx : 0;
    return (int64_t)p.empty * E - (int64_t)p.smooth * Sm - (int64_t)p.mono * Mo +
           (int64_t)p.corner * C;
}

// sum over the 16 cells of (e - 1) * 2^e (0 for an empty cell): the merge score it takes to build
// the board from 2s.  A merge of two e tiles raises it by 2^(e+1), the merge's gain, so a move's
// gain is the difference across it -- in int64, where apply_move's u32 sum would wrap.
__device__ __forceinline__ int64_t build_score(const Board& b) {
    const uint32_t rows[4] = {b.r0, b.r1, b.r2, b.r3};
    int64_t s = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t e = (rows[r] >> (8 * c)) & 0xFFu;
            s += e ? (e - 1) << e : 0;
        }
    }
    return s;
}

// after(b, a) in place; returns gain(b, a).  apply_move's gain is a u32 sum of 2^e with e taken
// mod 32: exact while every tile before the move is <= 2^27 (eight merged tiles <= 2^28 sum to
// <= 2^31).  Boards with a larger tile take the int64 difference instead.
__device__ __forceinline__ int64_t move_gain(Board& b, uint32_t a) {
    constexpr uint32_t K100 = 0x64646464u;  // e + 100 >= 128 iff e >= 28
    const bool big = (((b.r0 + K100) | (b.r1 + K100) | (b.r2 + K100) | (b.r3 + K100)) & K80) != 0u;
    const Board before = b;
    const uint32_t g = apply_move(b, a);
    if (big) return build_score(b) - build_score(before);
    return (int64_t)g;
}

__device__ __forceinline__ int64_t floor_quot(int64_t num, int32_t den) {  // den > 0
    const int64_t q = num / den;
    return q - (int64_t)(num % den < 0);
}

template <int D>
__device__ __forceinline__ int64_t vmax(const Board& b, const Params& p);

// Chance node over the slid board s; the children are searched D more player moves deep.
template <int D>
__device__ __forceinline__ int64_t vchance(const Board& s, const Params& p) {
    const uint32_t em = empty_mask(s);
    const int32_t n = __popc(em);
    int64_t sum = 0;
    // one loop over (cell, tile) pairs: bits 0-15 spawn a 2, bits 16-31 a 4
#pragma unroll 1
    for (uint32_t it = em | (em << 16); it != 0u; it &= it - 1u) {
        const uint32_t bit = __ffs(it) - 1u;
        const bool four = bit >= 16u;
        Board c = s;
        set_cell(c, bit & 15u, four ? 2u : 1u);
        sum += (int64_t)(four ? p.c4 : p.c2) * vmax<D>(c, p);
    }
    return floor_quot(sum, p.W * max(n, 1));
}

template <int D>
__device__ __forceinline__ int64_t vmax(const Board& b, const Params& p) {
    if constexpr (D == 0) {
        // a board that just received a tile is never empty, so is_done == (legal == 0)
        return is_done(b) ? -(int64_t)p.lost : heuristic(b, p);
    } else {
        const uint32_t legal = legal_mask(b);
        if (legal == 0u) return -(int64_t)p.lost;
        int64_t best = INT64_MIN;
#pragma unroll 1
        for (uint32_t a = 0; a < 4u; ++a) {
            if (!((legal >> a) & 1u)) continue;
            Board s = b;
            const int64_t g = move_gain(s, a);
            const int64_t v = (int64_t)p.gain * g + vchance<D - 1>(s, p);
            best = v > best ? v : best;
        }
        return best;
    }
}

constexpr int BLOCK = 256, WAVES = BLOCK / 64;

template <int DEPTH>
__global__ __launch_bounds__(BLOCK) void k_expectimax(const uint4* __restrict__ boards, int64_t n,
                                                      Params p, int64_t* __restrict__ values,
                                                      uint8_t* __restrict__ action) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = lane >> 4, c = lane & 15u;
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    for (int64_t i = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); i < n; i += stride) {
        const uint4 w = boards[i];  // wave-uniform address
        const Board b{w.x, w.y, w.z, w.w};
        const bool ok = (legal_mask(b) >> a) & 1u;
        Board s = b;
        const int64_t g = move_gain(s, a);
        int64_t sum = 0;
        if (ok && cell_empty(s, c)) {
            // the 2 and the 4 through one copy of the recursion's code
#pragma unroll 1
            for (uint32_t e = 1; e <= 2u; ++e) {
                Board child = s;
                set_cell(child, c, e);
                sum += (int64_t)(e == 1u ? p.c2 : p.c4) * vmax<DEPTH - 1>(child, p);
            }
        }
        // the chance node of move a: its 16 lanes are one row of the wave
        sum += __shfl_xor(sum, 8);
        sum += __shfl_xor(sum, 4);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 1);
        const int32_t ne = __popc(empty_mask(s));
        const int64_t v = ok ? (int64_t)p.gain * g + floor_quot(sum, p.W * max(ne, 1)) : INT64_MIN;
        const int64_t v0 = __shfl(v, 0), v1 = __shfl(v, 16), v2 = __shfl(v, 32), v3 = __shfl(v, 48);
        // smallest a with the largest value; an illegal move holds INT64_MIN and a legal move's
        // value is far above it, so with no legal move the action stays 0
        uint32_t act = 0;
        int64_t best = v0;
        if (v1 > best) { act = 1; best = v1; }
        if (v2 > best) { act = 2; best = v2; }
        if (v3 > best) { act = 3; }
        if (values != nullptr && lane < 4u)
            values[i * 4 + lane] = lane == 0u ? v0 : lane == 1u ? v1 : lane == 2u ? v2 : v3;
        if (action != nullptr && lane == 0u) action[i] = (uint8_t)act;
    }
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

constexpr g2048_search_weights DEFAULTS = {256, 2048, 256, 1024, 512, 1000000};

}  // namespace

extern "C" {

void g2048_search_default_weights(g2048_search_weights* w) {
    if (w != nullptr) *w = DEFAULTS;
}

const char* g2048_search_last_error(void) { return g_err.c_str(); }

int g2048_search_expectimax(const uint8_t* boards_dev, int64_t n, int depth, uint32_t flags,
                            const g2048_search_weights* w, int64_t* values_out_dev,
                            uint8_t* action_out_dev, int device_id, void* stream) {
    if (boards_dev == nullptr) return fail(G2048_EINVAL, "search_expectimax: boards_dev is NULL");
    if (((uintptr_t)boards_dev & 15u) != 0)
        return fail(G2048_EINVAL, "search_expectimax: boards_dev must be 16-byte aligned");
    if (n < 1 || n > G2048_MAX_BOARDS)
        return fail(G2048_EINVAL, "search_expectimax: n = %lld outside [1, G2048_MAX_BOARDS]",
                    (long long)n);
    if (depth < 1 || depth > G2048_SEARCH_MAX_DEPTH)
        return fail(G2048_EINVAL, "search_expectimax: depth = %d outside [1, %d]", depth,
                    G2048_SEARCH_MAX_DEPTH);
    if ((flags & ~(uint32_t)G2048_P4_10) != 0u)
        return fail(G2048_EINVAL, "search_expectimax: flags = 0x%x (only G2048_P4_10 is accepted)",
                    flags);
    if (values_out_dev == nullptr && action_out_dev == nullptr)
        return fail(G2048_EINVAL, "search_expectimax: both outputs are NULL");
    if (((uintptr_t)values_out_dev & 7u) != 0)
        return fail(G2048_EINVAL, "search_expectimax: values_out_dev must be 8-byte aligned");
    const g2048_search_weights ww = w != nullptr ? *w : DEFAULTS;
    const int32_t ws[6] = {ww.gain, ww.empty, ww.smooth, ww.mono, ww.corner, ww.lost};
    static const char* const names[6] = {"gain", "empty", "smooth", "mono", "corner", "lost"};
    for (int k = 0; k < 6; ++k) {
        const int32_t hi = k == 5 ? G2048_SEARCH_MAX_LOST : G2048_SEARCH_MAX_WEIGHT;
        if (ws[k] < 0 || ws[k] > hi)
            return fail(G2048_EINVAL, "search_expectimax: weight %s = %d outside [0, %d]", names[k],
                        ws[k], hi);
    }
    Params p;
    p.gain = ww.gain, p.empty = ww.empty, p.smooth = ww.smooth;
    p.mono = ww.mono, p.corner = ww.corner, p.lost = ww.lost;
    p.W = (flags & G2048_P4_10) ? 10 : 2;
    p.c4 = 1;
    p.c2 = p.W - p.c4;

    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    // a wave per board up to 8 blocks per CU, the rest by grid stride
    const int64_t blocks = (n + WAVES - 1) / WAVES;
    const dim3 grid((uint32_t)(blocks < 2048 ? blocks : 2048)), block(BLOCK);
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    switch (depth) {
    case 1: k_expectimax<1><<<grid, block, 0, st>>>(boards, n, p, values_out_dev, action_out_dev); break;
    case 2: k_expectimax<2><<<grid, block, 0, st>>>(boards, n, p, values_out_dev, action_out_dev); break;
    case 3: k_expectimax<3><<<grid, block, 0, st>>>(boards, n, p, values_out_dev, action_out_dev); break;
    default: k_expectimax<4><<<grid, block, 0, st>>>(boards, n, p, values_out_dev, action_out_dev); break;
    }
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
