// g2048_ntrestart.hip -- the per-board restart pool of n-tuple self-play for gfx950
// (libg2048_ntrestart.so): one kernel that runs after the env's step, records a snapshot when a
// board first reaches a largest-tile level and replaces a freshly re-dealt board with one of its
// own snapshots, by a fixed rotation of levels.
//
// The rule is defined in include/g2048_ntrestart.h.  Every value is an integer, board i touches
// row i of every buffer and nothing else, and the result is checked bit for bit against
// tests/ntrestart_ref.py.  No float, no atomics, no LDS, no traffic between lanes.
//
//   k_restart  one lane per board.  Every lane loads its board (one 16-byte load), done and top;
//              M(b) is the packed-max reduction of g2048_ntstage_dev.hpp, restated here so that
//              this library shares no internal header with the other eight (its stamp follows
//              its own source).  The common lane (the board moved on and did not climb) then
//              stores its restored_out byte, or nothing.  The two rare paths are divergent:
//                capture  two more loads (score, start) and the group clock, then the slot as two
//                         16-byte stores (the board; {score, moves, 0, 0}), valid and top;
//                done     turn, valid; a restore loads the slot (two 16-byte loads) and start,
//                         and stores the board (16 bytes), score, start and top.
//              A slot is 32 bytes and a board's 16 slots are 512 bytes, so every slot access is
//              a naturally aligned 16-byte access.  The rotation rides in the params struct as
//              eight bytes, wave-uniform.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/g2048_ntrestart.h"

namespace {

constexpr int BLOCK = 256;
constexpr uint32_t LEVELS = G2048_NTRESTART_LEVELS;

static_assert(sizeof(g2048_ntrestart_slot) == G2048_NTRESTART_SLOT_BYTES, "slot layout");

struct Rotation {
    uint64_t levels;  // byte k = levels[k] for k < L
    uint32_t n;       // L
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 pairs(uint32_t w) { return __builtin_bit_cast(u16x2, w); }

// M(b): the largest exponent byte.  Even and odd bytes as 16-bit pairs, a packed max over the
// eight words, then the larger half.
__device__ __forceinline__ uint32_t max_tile(const uint4& b) {
    constexpr uint32_t EVEN = 0x00FF00FFu;
    u16x2 m = __builtin_elementwise_max(pairs(b.x & EVEN), pairs((b.x >> 8) & EVEN));
    m = __builtin_elementwise_max(m, pairs(b.y & EVEN));
    m = __builtin_elementwise_max(m, pairs((b.y >> 8) & EVEN));
    m = __builtin_elementwise_max(m, pairs(b.z & EVEN));
    m = __builtin_elementwise_max(m, pairs((b.z >> 8) & EVEN));
    m = __builtin_elementwise_max(m, pairs(b.w & EVEN));
    m = __builtin_elementwise_max(m, pairs((b.w >> 8) & EVEN));
    const uint32_t w = __builtin_bit_cast(uint32_t, m);
    return max(w & 0xFFFFu, w >> 16);
}

__global__ __launch_bounds__(BLOCK) void k_restart(
    uint4* __restrict__ board, uint32_t* __restrict__ meta, const uint64_t* __restrict__ clock,
    const uint8_t* __restrict__ done, uint4* __restrict__ snap, uint16_t* __restrict__ valid,
    uint8_t* __restrict__ top, uint32_t* __restrict__ turn, uint8_t* __restrict__ restored,
    int64_t n, Rotation rot) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4 b = board[i];
    const uint32_t m = max_tile(b);
    uint32_t* __restrict__ score = meta;
    uint32_t* __restrict__ start = meta + n;
    uint4* __restrict__ slots = snap + i * (2 * LEVELS);  // 2 x 16 bytes per slot
    uint32_t back = 0;
    if (done[i] == 0) {
        // the board moved on: a snapshot the first time the episode stands at level m
        if (m > (uint32_t)top[i] && m < LEVELS) {
            const uint32_t now = (uint32_t)clock[i >> 6];
            slots[2 * m] = b;
            slots[2 * m + 1] = make_uint4(score[i], now - start[i], 0u, 0u);
            valid[i] = (uint16_t)(valid[i] | (1u << m));
            top[i] = (uint8_t)m;
        }
    } else {
        // the env has logged the episode and re-dealt the board: this episode's turn of the
        // rotation
        const uint32_t t = turn[i];
        const uint32_t e = (uint32_t)(rot.levels >> (8u * (t % rot.n))) & 0xFFu;
        turn[i] = t + 1u;
        if (e != 0u && (((uint32_t)valid[i] >> e) & 1u) != 0u) {
            const uint4 sb = slots[2 * e];
            const uint4 sm = slots[2 * e + 1];
            board[i] = sb;
            score[i] = sm.x;
            start[i] -= sm.y;  // moves = clock - start continues from the snapshot's
            top[i] = (uint8_t)e;
            back = e;
        } else {
            top[i] = (uint8_t)m;
        }
    }
    if (restored != nullptr) restored[i] = (uint8_t)back;
}

thread_local std::string g_err;

int refuse(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int refuse(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return G2048_EINVAL;
}

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

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) == 0; }

}  // namespace

extern "C" {

const char* g2048_ntrestart_last_error(void) { return g_err.c_str(); }

int64_t g2048_ntrestart_state_bytes(int64_t n) {
    if (n < 1 || n > G2048_MAX_BOARDS)
        return refuse("ntrestart_state_bytes: n = %lld outside [1, G2048_MAX_BOARDS]",
                      (long long)n);
    return n * (int64_t)(LEVELS * sizeof(g2048_ntrestart_slot) + sizeof(uint16_t) +
                         sizeof(uint8_t) + sizeof(uint32_t));
}

int g2048_ntrestart_apply(const uint8_t* levels, int32_t n_levels, uint8_t* board_dev,
                          uint32_t* meta_dev, const uint64_t* clock_dev, const uint8_t* done_dev,
                          g2048_ntrestart_slot* snap_dev, uint16_t* valid_dev, uint8_t* top_dev,
                          uint32_t* turn_dev, uint8_t* restored_out_dev, int64_t n, int device_id,
                          void* stream) {
    const char* who = "ntrestart_apply";
    if (levels == nullptr) return refuse("%s: levels is NULL", who);
    if (n_levels < 1 || n_levels > G2048_NTRESTART_MAX_ROTATION)
        return refuse("%s: n_levels = %d outside [1, %d]", who, n_levels,
                      G2048_NTRESTART_MAX_ROTATION);
    Rotation rot = {0, (uint32_t)n_levels};
    for (int k = 0; k < n_levels; ++k) {
        if (levels[k] >= LEVELS)
            return refuse("%s: level %d = %u outside [0, %u]", who, k, (unsigned)levels[k],
                          LEVELS - 1u);
        rot.levels |= (uint64_t)levels[k] << (8 * k);
    }
    if (n < 1 || n > G2048_MAX_BOARDS)
        return refuse("%s: n = %lld outside [1, G2048_MAX_BOARDS]", who, (long long)n);
    if (board_dev == nullptr || meta_dev == nullptr || clock_dev == nullptr || done_dev == nullptr)
        return refuse("%s: board_dev / meta_dev / clock_dev / done_dev is NULL", who);
    if (snap_dev == nullptr || valid_dev == nullptr || top_dev == nullptr || turn_dev == nullptr)
        return refuse("%s: snap_dev / valid_dev / top_dev / turn_dev is NULL", who);
    if (!aligned(board_dev, 16)) return refuse("%s: board_dev must be 16-byte aligned", who);
    if (!aligned(snap_dev, 16)) return refuse("%s: snap_dev must be 16-byte aligned", who);
    if (!aligned(clock_dev, 8)) return refuse("%s: clock_dev must be 8-byte aligned", who);
    if (!aligned(meta_dev, 4)) return refuse("%s: meta_dev must be 4-byte aligned", who);
    if (!aligned(turn_dev, 4)) return refuse("%s: turn_dev must be 4-byte aligned", who);
    if (!aligned(valid_dev, 2)) return refuse("%s: valid_dev must be 2-byte aligned", who);
    DeviceGuard guard(device_id);
    const dim3 grid((uint32_t)((n + BLOCK - 1) / BLOCK));
    k_restart<<<grid, dim3(BLOCK), 0, (hipStream_t)stream>>>(
        reinterpret_cast<uint4*>(board_dev), meta_dev, clock_dev, done_dev,
        reinterpret_cast<uint4*>(snap_dev), valid_dev, top_dev, turn_dev, restored_out_dev, n,
        rot);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        refuse("%s: launch: %s", who, hipGetErrorString(e));
        return G2048_EHIP;
    }
    return G2048_OK;
}

}  // extern "C"
