// g2048_ntlambda.hip -- truncated TD(lambda) learning for the n-tuple value network on gfx950
// (libg2048_ntlambda.so).
//
// The rule is defined in include/g2048_ntlambda.h; every value is an integer and the result is
// checked bit for bit against tests/ntlambda_ref.py.  No float anywhere.  The library takes the
// spec and the table of g2048_ntuple.h and does not link against libg2048_ntuple.so.  What it has
// in common with g2048_ntuple.hip is g2048_ntuple_dev.hpp's: the index helpers, the policy's lane
// decode, group sum, argmax and err / delta, the merge table's keys, the clamped ring position
// (which g2048_stagedelay.hip reads too), and the host plumbing and argument checks.  Here are
// the walk over the ring of afterstates with the shifted deltas, its commit and the entry points.
//
// A step is two launches, ordered as in TD(0): the first never writes lut, the second never reads
// it.
//   k_lam_policy  g2048_ntuple.hip's k_policy<T, true>: 2 boards per wave, lane 32s + 8a + g
//                 evaluates after(board s, a) under symmetry g; the groups a == 0 also gather
//                 V(prev) in the same burst, prev being the board's row of its head plane
//                 (one byte load each for head and depth, where TD(0) loads has_prev).
//   k_lam_update  8 boards per wave, 128 per block: lane g walks the board's depth afterstates
//                 back from the head plane; for the afterstate k steps back it packs the nibbles
//                 under symmetry g, forms delta_k = sgn(delta) (|delta| >> k s) and adds it into
//                 its T entries -- summed per block in an LDS hash table first, then one 32-bit
//                 atomic per used slot.  The walk ends at the first delta_k == 0 (the later ones
//                 are 0 too).  After the barrier that ends all reads of the ring, lane 0 of the
//                 group commits head / plane / depth; with depth == H the plane it overwrites is
//                 the one read as k = H - 1 before the barrier.
// H and s are run-time values (the update has no gathers to batch); T is a template parameter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_ntlambda.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"

// G2048_NTLAMBDA_SLOT_BITS, if defined, fixes log2 of the LDS merge table's slots for every T
// (lam_slot_bits)

// -DG2048_NTLAMBDA_COUNT_BYPASS: a measuring build (tools/ntlambda_bench.py --lib) that counts the
// update's adds and those of them that found no slot, and exports g2048_ntlambda_debug_counts.
// Not part of the ABI and not built by default.

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int MAXH = G2048_NTLAMBDA_MAX_HORIZON;
constexpr int BLOCK = 256;

template <int T>
__global__ __launch_bounds__(BLOCK) void k_lam_policy(
    const int32_t* __restrict__ lut, const uint4* __restrict__ boards, int64_t n,
    uint8_t* __restrict__ action_out, const uint4* __restrict__ hist,
    const uint8_t* __restrict__ head, const uint8_t* __restrict__ depth, uint32_t H,
    int32_t lr_num, int32_t lr_shift, int32_t* __restrict__ delta_out,
    int64_t* __restrict__ err_out, Params p) {
    const PolicyLane l = policy_lane<BLOCK>(boards, n);
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[entry(p, l.nib, t)] : 0;
    const Ring r = load_ring(head, depth, l.bi, H);
    const bool hp = r.depth != 0u;
    // the afterstate 0 steps back: row bi of the head plane
    const uint64_t pnib = nibbles(sym(load_board(hist, (int64_t)r.head * n + l.bi), l.g));
#pragma unroll
    for (int t = 0; t < T; ++t) pv[t] = (hp && l.a == 0u) ? lut[entry(p, pnib, t)] : 0;
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const Best m = best_move<8>(l.ok ? ((int64_t)l.gain << F) + sum : INT64_MIN, l.lane);
#pragma unroll
    for (int t = 0; t < T; ++t) psum += pv[t];
    psum = group_sum(psum);  // V(prev) in the group a == 0
    if (!l.live) return;
    if ((l.lane & 31u) == 0u) {
        const TdError td = td_error(m.best, psum, hp, l.legal, lr_num, lr_shift);
        action_out[l.i] = (uint8_t)m.act;
        delta_out[l.i] = td.delta;
        if (err_out != nullptr) err_out[l.i] = td.err;
    }
}

// The update's block: 128 boards, as g2048_ntuple.hip's k_update, with up to H times its keys.
// A block first sums what it adds into an entry in an LDS hash table (g2048_ntuple_dev.hpp's
// clear_keys / claim_slot: the entry index is the key; after four slots taken by other keys the
// add goes straight to memory) and then flushes every used slot with one atomic.  Integer adds
// commute and associate modulo 2^32, so the table ends up the same whichever way the sum is
// grouped.
constexpr int UBLOCK = 1024;
// log2 of the table's slots; a slot is 8 bytes (key, sum) and a block makes up to 1024 T H adds.
// Measured: on the 4 x 6 set 16384 slots (128 KiB, one block per CU) are 1-5 %
// faster than TD(0)'s 8192 (64 KiB, two blocks per CU) at every horizon; on the 2 x 4 set, whose
// 6144 keys at H = 3 fit either, the two take the same time with adds and the larger one 5 us
// more without, so T <= 2 keeps TD(0)'s size.
template <int T>
constexpr int lam_slot_bits() {
#ifdef G2048_NTLAMBDA_SLOT_BITS
    return G2048_NTLAMBDA_SLOT_BITS;
#else
    return T <= 2 ? 13 : 14;
#endif
}

#ifdef G2048_NTLAMBDA_COUNT_BYPASS
__device__ unsigned long long g_counts[2];  // adds; adds that went straight to memory
#endif

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_lam_update(
    int32_t* __restrict__ lut, const uint4* __restrict__ boards, int64_t n,
    uint4* __restrict__ hist, uint8_t* __restrict__ head, uint8_t* __restrict__ depth, uint32_t H,
    uint32_t lam_shift, const uint8_t* __restrict__ action, const int32_t* __restrict__ delta,
    Params p) {
    constexpr int SLOT_BITS = lam_slot_bits<T>();
    constexpr uint32_t SLOTS = 1u << SLOT_BITS;
    static_assert(SLOTS * 8u <= 160u * 1024u, "the LDS table must fit a CU's 160 KiB");
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
    const Ring r = live ? load_ring(head, depth, i, H) : Ring{0u, 0u};
    const int32_t d = r.depth != 0u ? delta[i] : 0;
    // |delta| <= 2^31 fits 32 unsigned bits, and k s <= (H - 1) s <= 31
    const uint32_t mag = d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
    uint32_t plane = r.head;
#ifdef G2048_NTLAMBDA_COUNT_BYPASS
    uint32_t n_adds = 0, n_direct = 0;
#endif
    for (uint32_t k = 0; k < r.depth; ++k) {
        const uint32_t mk = mag >> (k * lam_shift);
        if (mk == 0u) break;  // and so are the later ones
        const uint32_t dk = d < 0 ? 0u - mk : mk;
        const uint64_t nib = nibbles(sym(load_board(hist, (int64_t)plane * n + i), g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = entry(p, nib, t);
            const uint32_t slot = claim_slot<SLOT_BITS>(keys, e);
            if (slot != NO_SLOT) atomicAdd(&sums[slot], dk);
            else atomicAdd(&table[e], dk);
#ifdef G2048_NTLAMBDA_COUNT_BYPASS
            n_adds += 1u;
            n_direct += slot == NO_SLOT ? 1u : 0u;
#endif
        }
        plane = plane == 0u ? H - 1u : plane - 1u;
    }
#ifdef G2048_NTLAMBDA_COUNT_BYPASS
    if (n_adds != 0u) atomicAdd(&g_counts[0], (unsigned long long)n_adds);
    if (n_direct != 0u) atomicAdd(&g_counts[1], (unsigned long long)n_direct);
#endif
    // every read of the board's ring, head and depth lies before this barrier, lane 0's stores
    // after it
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s], v = sums[s];
        if (k != NO_KEY && v != 0u) atomicAdd(&table[k], v);
    }
    if (live && g == 0u) {
        const Board b = load_board(boards, i);
        if (legal_mask(b) != 0u) {
            Board s = b;
            apply_move(s, (uint32_t)action[i] & 3u);
            const uint32_t nh = r.head + 1u == H ? 0u : r.head + 1u;
            hist[(int64_t)nh * n + i] = make_uint4(s.r0, s.r1, s.r2, s.r3);
            head[i] = (uint8_t)nh;
            depth[i] = (uint8_t)min(r.depth + 1u, H);
        } else {
            depth[i] = 0;
        }
    }
}

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_ntlambda_last_error(void) { return g_err.c_str(); }

#ifdef G2048_NTLAMBDA_COUNT_BYPASS
// out[0] = adds, out[1] = adds straight to memory since the last reset (synchronises the device)
G2048_API int g2048_ntlambda_debug_counts(uint64_t out[2], int reset) {
    unsigned long long host[2] = {0ull, 0ull};
    G_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_counts), sizeof(host)));
    out[0] = host[0], out[1] = host[1];
    if (reset != 0) {
        const unsigned long long zero[2] = {0ull, 0ull};
        G_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_counts), zero, sizeof(zero)));
    }
    return G2048_OK;
}
#endif

int g2048_ntlambda_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, const uint8_t* boards_dev,
                        int64_t n, uint8_t* hist_dev, uint8_t* head_dev, uint8_t* depth_dev,
                        int32_t horizon, int32_t lam_shift, int32_t lr_num, int32_t lr_shift,
                        uint8_t* action_out_dev, int32_t* delta_out_dev, int64_t* err_out_dev,
                        int device_id, void* stream) {
    const char* who = "ntlambda_step";
    int rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    if (hist_dev == nullptr || head_dev == nullptr || depth_dev == nullptr)
        return refuse(g_err, "%s: hist_dev / head_dev / depth_dev is NULL", who);
    if (((uintptr_t)hist_dev & 15u) != 0)
        return refuse(g_err, "%s: hist_dev must be 16-byte aligned", who);
    if (horizon < 1 || horizon > MAXH)
        return refuse(g_err, "%s: horizon = %d outside [1, %d]", who, horizon, MAXH);
    if (lam_shift < 1 || lam_shift > G2048_NTLAMBDA_MAX_LAM_SHIFT)
        return refuse(g_err, "%s: lam_shift = %d outside [1, %d]", who, lam_shift,
                      G2048_NTLAMBDA_MAX_LAM_SHIFT);
    if ((horizon - 1) * lam_shift > 31)
        return refuse(g_err, "%s: (horizon - 1) * lam_shift = %d exceeds 31", who,
                      (horizon - 1) * lam_shift);
    if (lr_num < 0 || lr_num > G2048_NTUPLE_MAX_LR_NUM)
        return refuse(g_err, "%s: lr_num = %d outside [0, %d]", who, lr_num,
                      G2048_NTUPLE_MAX_LR_NUM);
    if (lr_shift < 0 || lr_shift > G2048_NTUPLE_MAX_LR_SHIFT)
        return refuse(g_err, "%s: lr_shift = %d outside [0, %d]", who, lr_shift,
                      G2048_NTUPLE_MAX_LR_SHIFT);
    if (action_out_dev == nullptr || delta_out_dev == nullptr)
        return refuse(g_err, "%s: action_out_dev / delta_out_dev is NULL", who);
    if (((uintptr_t)delta_out_dev & 3u) != 0)
        return refuse(g_err, "%s: delta_out_dev must be 4-byte aligned", who);
    if (((uintptr_t)err_out_dev & 7u) != 0)
        return refuse(g_err, "%s: err_out_dev must be 8-byte aligned", who);
    const Params p = make_params(*spec);
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* hist = reinterpret_cast<uint4*>(hist_dev);
    const uint32_t H = (uint32_t)horizon;
    DISPATCH_T(spec->n_tuples,
               (k_lam_policy<TT><<<grid_for(n, BLOCK / 32), dim3(BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, hist, head_dev, depth_dev, H, lr_num,
                   lr_shift, delta_out_dev, err_out_dev, p)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples, (k_lam_update<TT><<<grid_for(n, UBLOCK / 8), dim3(UBLOCK), 0, st>>>(
                                   lut_dev, boards, n, hist, head_dev, depth_dev, H,
                                   (uint32_t)lam_shift, action_out_dev, delta_out_dev, p)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
