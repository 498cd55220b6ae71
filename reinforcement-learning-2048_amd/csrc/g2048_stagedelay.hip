// g2048_stagedelay.hip -- delayed TD(lambda) on the staged batch-mean temporal-coherence rule for
// the multi-stage n-tuple value network on gfx950 (libg2048_stagedelay.so).
//
// The rule is defined in include/g2048_stagedelay.h; every value is an integer and the result is
// checked bit for bit against tests/stagedelay_ref.py.  No float anywhere.  The library takes the
// spec, the stage spec and the table of g2048_ntstage.h and does not link against another library
// of the project.
//
// What it shares with the family is the headers': the policy's lane decode, group sum, argmax,
// err and the clamped ring position (g2048_ntuple_dev.hpp), the stage of a board, the
// fall-through, the promotion store and the staged index (g2048_ntstage_dev.hpp), the gather
// table's hit and flush, the (D, C) add, the owner exchange and the temporal-coherence tail
// (g2048_ntmean_dev.hpp).  Here are the ring of afterstates with its error sums and the three
// kernels that walk it:
//   k_delay_policy  g2048_ntstage_dev.hpp's k_stage_policy<T, true> with prev read through the
//                   head plane (as g2048_ntlambda.hip's k_lam_policy does for the flat table).
//                   Lane k < H of a board's group a == 0 then owns slot k: it forms G_k, writes
//                   delta_out[k][i] (0 unless slot k is applied) and, on a non-terminal board,
//                   stores G_k of a kept slot -- or the 0 of slot H - 1, the plane the commit
//                   writes next -- into g.  One lane per word of g reads and writes it.
//   k_delay_gather  8 boards per wave, 128 per block: lane g < depth of a board's group loads
//                   delta_out[g][i], the group passes them round, and for every slot k with
//                   delta_k != 0 lane g re-forms its T staged entries of the afterstate k steps
//                   back and adds (delta_k, 1) -- merged per block in the LDS table of
//                   k_mean_gather, a hit without a slot after four probes straight to memory.
//   k_delay_apply   the same walk over k_mean_apply's key table and owner exchange; after the
//                   barrier that ends all reads of the ring, lane 0 commits hist / head / depth.
// A non-terminal board has at most one applied slot, so the tables see what k_mean_gather's see;
// a block of terminal boards makes up to H times the keys, and what finds no slot goes the
// direct way, which is correct at any load.  H and s are run-time values; T is a template
// parameter.
// The three kernels keep the lines they have in common with k_stage_policy<T, true>,
// k_mean_gather and k_mean_apply written out.  Only what compiles to the same text either way is
// a function of the headers; the rest, put into one, reschedules the kernel around it
// (profiles/tcfamily/README.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stagedelay.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntmean_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int RATE_BITS = G2048_STAGEDELAY_RATE_BITS;
constexpr int MAXH = G2048_STAGEDELAY_MAX_HORIZON;
static_assert(MAXH <= 8, "a board's group of 8 lanes holds one slot of the ring per lane");

template <int T>
__global__ __launch_bounds__(POLICY_BLOCK) void k_delay_policy(
    int32_t* lut, const uint4* __restrict__ boards, int64_t n, uint8_t* __restrict__ action_out,
    const uint4* __restrict__ hist, const uint8_t* __restrict__ head,
    const uint8_t* __restrict__ depth, int64_t* __restrict__ gsum, uint32_t H, uint32_t lam_shift,
    int32_t lr_num, int32_t lr_shift, int32_t* __restrict__ delta_out,
    int64_t* __restrict__ err_out, Params p, StageParams sp) {
    const PolicyLane l = policy_lane<POLICY_BLOCK>(boards, n);
    const uint32_t st = stage_of(l.s, sp);  // the afterstate's stage: a merge can raise it
    uint32_t e[T], pe[T];
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) e[t] = st * sp.stride + entry(p, l.nib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[e[t]] : 0;
    const Ring r = load_ring(head, depth, l.bi, H);
    const bool hp = r.depth != 0u;
    const bool mine = hp && l.a == 0u;  // this lane gathers (and promotes) prev's entries
    // the afterstate 0 steps back: row bi of the head plane
    const Board pb = load_board(hist, (int64_t)r.head * n + l.bi);
    const uint32_t pst = stage_of(pb, sp);
    const uint64_t pnib = nibbles(sym(pb, l.g));
    uint32_t unset = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) pe[t] = pst * sp.stride + entry(p, pnib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) pv[t] = mine ? lut[pe[t]] : 0;
#pragma unroll
    for (int t = 0; t < T; ++t) unset |= pv[t] == UNSET ? 1u << t : 0u;
    resolve<T, true>(lut, sp, e, v, st, pe, pv, pst);
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const Best m = best_move<8>(l.ok ? ((int64_t)l.gain << F) + sum : INT64_MIN, l.lane);
#pragma unroll
    for (int t = 0; t < T; ++t) psum += pv[t];
    psum = group_sum(psum);  // V(prev) in the group a == 0
    if (!l.live) return;
    // `unset` is 0 outside the groups a == 0 of boards with has_prev
    promote(lut, pe, pv, unset);
    // the group a == 0 holds V(prev) in every lane: lane k of it owns slot k of the ring
    const uint32_t k = l.lane & 31u;
    if (k >= H) return;
    const int64_t err = td_error(m.best, psum, hp, l.legal, lr_num, lr_shift).err;
    if (k == 0u) {
        action_out[l.i] = (uint8_t)m.act;
        if (err_out != nullptr) err_out[l.i] = err;
    }
    const bool terminal = l.legal == 0u;
    const int64_t at = (int64_t)plane_back(r.head, k, H) * n + l.i;
    int32_t dk = 0;
    if (k < r.depth) {
        // |err| in 64 bits, k s <= (H - 1) s <= 31: the shift rounds toward zero
        const uint64_t mag = (err < 0 ? 0ull - (uint64_t)err : (uint64_t)err) >> (k * lam_shift);
        const int64_t G = gsum[at] + (err < 0 ? -(int64_t)mag : (int64_t)mag);
        // k < depth and k == H - 1 say depth == H: the oldest afterstate leaves the window
        if (terminal || k == H - 1u) dk = (int32_t)((G * (int64_t)lr_num) >> lr_shift);
        else gsum[at] = G;
    }
    // (head - (H - 1)) mod H = (head + 1) mod H: the plane the commit gives the new afterstate
    if (!terminal && k == H - 1u) gsum[at] = 0;
    delta_out[(int64_t)k * n + l.i] = dk;
}

// delta_k of the board, in every lane of its group: lane k of the group holds it (0 for
// k >= depth).  Called by whole waves.
__device__ __forceinline__ int32_t slot_delta(int32_t mine, uint32_t k) {
    return __shfl(mine, (int)(((threadIdx.x & 63u) & ~7u) + k));
}

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_delay_gather(
    int64_t* __restrict__ acc_, int64_t n, const uint4* __restrict__ hist,
    const uint8_t* __restrict__ head, const uint8_t* __restrict__ depth, uint32_t H,
    const int32_t* __restrict__ delta, Params p, StagedIndex ix) {
    __shared__ uint32_t keys[gather_slots<T>()];
    __shared__ uint32_t csum[gather_slots<T>()];  // a block makes at most 1024 T H <= 2^16 hits
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
    const bool live = i < n;
    u64* acc = reinterpret_cast<u64*>(acc_);  // additions modulo 2^64
    const Ring r = live ? load_ring(head, depth, i, H) : Ring{0u, 0u};
    const int32_t mine = g < r.depth ? delta[(int64_t)g * n + i] : 0;
    for (uint32_t k = 0; k < H; ++k) {
        const int32_t d = slot_delta(mine, k);
        if (d == 0) continue;  // d != 0 says k < depth
        const Board hb = load_board(hist, (int64_t)plane_back(r.head, k, H) * n + i);
        const uint32_t base = ix.base(hb);
        const uint64_t nib = nibbles(sym(hb, g));
        const u64 de = (u64)(int64_t)d;
#pragma unroll
        for (int t = 0; t < T; ++t)
            gather_hit<T>(keys, csum, dsum, acc, base + entry(p, nib, t), de);
    }
    __syncthreads();
    gather_flush<T>(keys, csum, dsum, acc);
}

template <int T>
__global__ __launch_bounds__(UBLOCK) void k_delay_apply(
    int32_t* __restrict__ lut, int64_t* __restrict__ acc_, longlong2* __restrict__ ea,
    const uint4* __restrict__ boards, int64_t n, uint4* __restrict__ hist,
    uint8_t* __restrict__ head, uint8_t* __restrict__ depth, uint32_t H,
    const uint8_t* __restrict__ action, const int32_t* __restrict__ delta, Params p,
    StagedIndex ix) {
    const TcTail<RATE_BITS> tail{ea};
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
    const Ring r = live ? load_ring(head, depth, i, H) : Ring{0u, 0u};
    const int32_t mine = g < r.depth ? delta[(int64_t)g * n + i] : 0;
    for (uint32_t k = 0; k < H; ++k) {
        const int32_t d = slot_delta(mine, k);
        if (d == 0) continue;
        const Board hb = load_board(hist, (int64_t)plane_back(r.head, k, H) * n + i);
        const uint32_t base = ix.base(hb);
        const uint64_t nib = nibbles(sym(hb, g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = base + entry(p, nib, t);
            // a hit that finds no slot asks for the entry itself
            if (claim_slot<APPLY_SLOT_BITS>(keys, e) == NO_SLOT) apply_entry(table, acc, e, tail);
        }
    }
    // every read of the board's ring, head and depth lies before this barrier, lane 0's stores
    // after it
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t key = keys[s];
        if (key != NO_KEY) apply_entry(table, acc, key, tail);
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

const char* g2048_stagedelay_last_error(void) { return g_err.c_str(); }

int32_t g2048_stagedelay_rate(int64_t E, int64_t A) {
    return checked_rate<RATE_BITS, G2048_STAGEDELAY_MAX_A>(g_err, "stagedelay_rate", E, A);
}

int64_t g2048_stagedelay_acc_bytes(const g2048_ntuple_spec* spec,
                                   const g2048_ntstage_spec* stages) {
    return staged_acc_bytes(g_err, "stagedelay_acc_bytes", spec, stages);
}

int g2048_stagedelay_step(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                          int32_t* lut_dev, int64_t* acc_dev, int64_t* ea_dev,
                          const uint8_t* boards_dev, int64_t n, uint8_t* hist_dev,
                          uint8_t* head_dev, uint8_t* depth_dev, int64_t* g_dev, int32_t horizon,
                          int32_t lam_shift, int32_t lr_num, int32_t lr_shift,
                          uint8_t* action_out_dev, int32_t* delta_out_dev, int64_t* err_out_dev,
                          int device_id, void* stream) {
    const char* who = "stagedelay_step";
    int rc = check_staged_tc(g_err, who, spec, stages, lut_dev, boards_dev, n, acc_dev, ea_dev);
    if (rc != G2048_OK) return rc;
    rc = check_ptr(g_err, who, "g_dev", g_dev, 8);
    if (rc != G2048_OK) return rc;
    if (horizon < 1 || horizon > MAXH)
        return refuse(g_err, "%s: horizon = %d outside [1, %d]", who, horizon, MAXH);
    if (lam_shift < 1 || lam_shift > G2048_STAGEDELAY_MAX_LAM_SHIFT)
        return refuse(g_err, "%s: lam_shift = %d outside [1, %d]", who, lam_shift,
                      G2048_STAGEDELAY_MAX_LAM_SHIFT);
    if ((horizon - 1) * lam_shift > G2048_STAGEDELAY_MAX_LAM_SHIFT)
        return refuse(g_err, "%s: (horizon - 1) * lam_shift = %d exceeds %d", who,
                      (horizon - 1) * lam_shift, G2048_STAGEDELAY_MAX_LAM_SHIFT);
    // the ring stands where prev / has_prev stand: hist for prev, head (and depth) for has_prev
    if (head_dev == nullptr || depth_dev == nullptr)
        return refuse(g_err, "%s: head_dev / depth_dev is NULL", who);
    rc = check_ptr(g_err, who, "hist_dev", hist_dev, 16);
    if (rc != G2048_OK) return rc;
    rc = check_td_args(g_err, who, hist_dev, head_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    const Params p = make_params(*spec);
    const StagedIndex ix{make_stage_params(*spec, *stages)};
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* hist = reinterpret_cast<uint4*>(hist_dev);
    const uint32_t H = (uint32_t)horizon;
    const dim3 grid = grid_for(n, UBLOCK / 8);
    DISPATCH_T(spec->n_tuples, (k_delay_policy<TT><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
                                   lut_dev, boards, n, action_out_dev, hist, head_dev, depth_dev,
                                   g_dev, H, (uint32_t)lam_shift, lr_num, lr_shift, delta_out_dev,
                                   err_out_dev, p, ix.sp)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples, (k_delay_gather<TT><<<grid, dim3(UBLOCK), 0, st>>>(
                                   acc_dev, n, hist, head_dev, depth_dev, H, delta_out_dev, p, ix)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples,
               (k_delay_apply<TT><<<grid, dim3(UBLOCK), 0, st>>>(
                   lut_dev, acc_dev, reinterpret_cast<longlong2*>(ea_dev), boards, n, hist,
                   head_dev, depth_dev, H, action_out_dev, delta_out_dev, p, ix)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
