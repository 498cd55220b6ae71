// g2048_stageback.hip -- backward episode learning on the staged batch-mean temporal-coherence
// rule for the multi-stage n-tuple value network on gfx950 (libg2048_stageback.so).
//
// The rule is defined in include/g2048_stageback.h; every value is an integer and the result is
// checked bit for bit against tests/stageback_ref.py.  No float anywhere.  The library takes the
// spec, the stage spec and the table of g2048_ntstage.h and does not link against another library
// of the project.
//
// What it shares with the family is the headers': the policy's lane decode, group sum, argmax and
// err (g2048_ntuple_dev.hpp), the stage of a board, the fall-through, the promotion store and
// the staged index (g2048_ntstage_dev.hpp), the (D, C) gather, the owner exchange and the temporal-coherence tail
// (g2048_ntmean_dev.hpp).  Here are the two trajectory buffers of a board with their counters and
// the two kernels that the headers do not have:
//   k_back_policy  k_stage_policy's frame, 32 lanes per board.  Lane 0 of a board reads its four
//                  counters and the group passes them round.  Of a replaying board the group
//                  a == 0 gathers (and promotes) x's entries, the group a == 1 gathers y's, both
//                  in the fall-through rounds of the policy's own lookups: resolve<T, true>'s
//                  second set takes a stage per lane.  Lane 0 writes action, delta, err, x_out
//                  and replay_out and commits the counters; the lane (a == action, g == 0),
//                  which holds after(b, action) and its gain, records them.
//   (gather)       k_mean_gather<T, StagedIndex> itself, with prev := x_out and has_prev :=
//                  replay_out.
//   k_back_apply   k_mean_apply's frame with TcTail and without the commit of prev.
// Only the first launch sees the trajectory and the counters.  A board's words of them are read
// and written by that board's 32 lanes alone, all in one wave, every load before the first store,
// and the buffer read ((cur & 1) ^ 1) is never the buffer written (cur & 1).  L is a run-time
// value; T is a template parameter.
// The two kernels keep the lines they have in common with k_stage_policy<T, true>
// and k_mean_apply written out.  Only what compiles to the same text either way is
// a function of the headers; the rest, put into one, reschedules the kernel around it
// (profiles/tcfamily/README.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stageback.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntmean_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int RATE_BITS = G2048_STAGEBACK_RATE_BITS;

// Row (i, buf, slot) of traj and of gain: 64-bit, n L reaches 2^31 and there are two buffers.
// buf <= 1 and slot < L, so the row lies inside board i's own planes whatever the counters hold.
__device__ __forceinline__ int64_t slot_row(int64_t i, uint32_t buf, uint32_t slot, uint32_t L) {
    return (i * 2 + (int64_t)buf) * (int64_t)L + (int64_t)slot;
}

template <int T>
__global__ __launch_bounds__(POLICY_BLOCK) void k_back_policy(
    int32_t* lut, const uint4* __restrict__ boards, int64_t n, uint8_t* __restrict__ action_out,
    uint4* traj, int32_t* gain, uint8_t* cur, uint32_t* rec, uint32_t* rep_n, uint32_t* rep_k,
    uint32_t L, int32_t lr_num, int32_t lr_shift, int32_t* __restrict__ delta_out,
    uint4* __restrict__ x_out, uint8_t* __restrict__ replay_out, int64_t* __restrict__ err_out,
    Params p, StageParams sp) {
    const PolicyLane l = policy_lane<POLICY_BLOCK>(boards, n);
    const uint32_t st = stage_of(l.s, sp);  // the afterstate's stage: a merge can raise it
    uint32_t e[T], pe[T];
    int32_t v[T], pv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) e[t] = st * sp.stride + entry(p, l.nib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = l.ok ? lut[e[t]] : 0;
    // the board's counters: its lane 0 loads them, its 32 lanes get them
    const bool lead = (l.lane & 31u) == 0u;
    const int first = (int)(l.lane & 32u);
    uint32_t raw_cur = 0, c_rec = 0, c_n = 0, c_k = 0;
    if (lead) {
        raw_cur = cur[l.bi];
        c_rec = rec[l.bi];
        c_n = rep_n[l.bi];
        c_k = rep_k[l.bi];
    }
    const uint32_t c_cur = (uint32_t)__shfl((int)raw_cur, first) & 1u;  // only bit 0 counts
    c_rec = (uint32_t)__shfl((int)c_rec, first);
    c_n = (uint32_t)__shfl((int)c_n, first);
    c_k = (uint32_t)__shfl((int)c_k, first);
    const bool replays = c_k < min(c_n, L);
    const bool has_y = replays && c_k != 0u;  // x has a successor: it is not the episode's last
    // j = rep_n - 1 - rep_k; where the board idles the slots are not used, and are < L anyway
    const uint32_t sx = (c_n - 1u - c_k) % L;
    const uint32_t sy = sx + 1u == L ? 0u : sx + 1u;
    const bool gx = replays && l.a == 0u;  // this lane gathers (and promotes) x's entries
    const bool gy = has_y && l.a == 1u;    // this lane gathers y's
    const bool mine = gx || gy;
    Board pb = Board{0u, 0u, 0u, 0u};
    if (mine) pb = load_board(traj, slot_row(l.bi, c_cur ^ 1u, gx ? sx : sy, L));
    // a gain reaches 2^31 (eight merges of 27s): the plane holds its 32-bit pattern
    const uint32_t ygain = lead && has_y ? (uint32_t)gain[slot_row(l.bi, c_cur ^ 1u, sy, L)] : 0u;
    const uint32_t pst = stage_of(pb, sp);
    const uint64_t pnib = nibbles(sym(pb, l.g));
    uint32_t unset = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) pe[t] = pst * sp.stride + entry(p, pnib, t);
#pragma unroll
    for (int t = 0; t < T; ++t) pv[t] = mine ? lut[pe[t]] : 0;
#pragma unroll
    for (int t = 0; t < T; ++t) unset |= (gx && pv[t] == UNSET) ? 1u << t : 0u;
    resolve<T, true>(lut, sp, e, v, st, pe, pv, pst);
    int64_t sum = 0, psum = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) sum += v[t];
    sum = group_sum(sum);
    const Best m = best_move<8>(l.ok ? ((int64_t)l.gain << F) + sum : INT64_MIN, l.lane);
#pragma unroll
    for (int t = 0; t < T; ++t) psum += pv[t];
    psum = group_sum(psum);                      // V(x) in the group a == 0, V(y) in a == 1
    const int64_t vy = __shfl(psum, first + 8);  // V(y), or 0 without a successor
    if (!l.live) return;
    // x's entries that this lane found UNSET: `unset` is 0 outside the groups a == 0 of
    // replaying boards
    promote(lut, pe, pv, unset);
    // record: this lane holds after(b, action) and gain(b, action)
    if (l.legal != 0u && l.a == m.act && l.g == 0u) {
        const int64_t at = slot_row(l.i, c_cur, c_rec % L, L);
        traj[at] = make_uint4(l.s.r0, l.s.r1, l.s.r2, l.s.r3);
        gain[at] = (int32_t)l.gain;
    }
    if (!lead) return;
    // the target stands where the best q stands in the forward rule, on a board that goes on
    const int64_t target = has_y ? ((int64_t)ygain << F) + vy : 0;
    const TdError td = td_error(target, psum, replays, 1u, lr_num, lr_shift);
    action_out[l.i] = (uint8_t)m.act;
    delta_out[l.i] = td.delta;
    if (err_out != nullptr) err_out[l.i] = td.err;
    replay_out[l.i] = replays ? 1 : 0;
    if (replays) x_out[l.i] = make_uint4(pb.r0, pb.r1, pb.r2, pb.r3);
    // commit: the transition of an older replay is made above even where the episode closes here
    if (l.legal != 0u) {
        rec[l.i] = c_rec + 1u;
        if (replays) rep_k[l.i] = c_k + 1u;
    } else if (c_rec != 0u) {
        cur[l.i] = (uint8_t)(raw_cur ^ 1u);
        rep_n[l.i] = c_rec;
        rep_k[l.i] = 0u;
        rec[l.i] = 0u;
    } else if (replays) {
        rep_k[l.i] = c_k + 1u;
    }
}

// k_mean_apply's frame without its last line: the step keeps no prev, so nothing is committed
// here and the launch needs neither the boards nor the actions.
template <int T>
__global__ __launch_bounds__(UBLOCK) void k_back_apply(
    int32_t* __restrict__ lut, int64_t* __restrict__ acc_, longlong2* __restrict__ ea, int64_t n,
    const uint4* __restrict__ x, const uint8_t* __restrict__ replays,
    const int32_t* __restrict__ delta, Params p, StagedIndex ix) {
    const TcTail<RATE_BITS> tail{ea};
    constexpr uint32_t SLOTS = 1u << APPLY_SLOT_BITS;
    __shared__ uint32_t keys[SLOTS];
    clear_keys<APPLY_SLOT_BITS, UBLOCK>(keys);
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * UBLOCK + threadIdx.x;
    const int64_t i = tid >> 3;
    const uint32_t g = threadIdx.x & 7u;
    uint32_t* table = reinterpret_cast<uint32_t*>(lut);  // additions modulo 2^32
    u64* acc = reinterpret_cast<u64*>(acc_);
    const int32_t d = i < n && replays[i] != 0 ? delta[i] : 0;
    if (d != 0) {
        const Board xb = load_board(x, i);
        const uint32_t base = ix.base(xb);
        const uint64_t nib = nibbles(sym(xb, g));
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t e = base + entry(p, nib, t);
            // a hit that finds no slot asks for the entry itself
            if (claim_slot<APPLY_SLOT_BITS>(keys, e) == NO_SLOT) apply_entry(table, acc, e, tail);
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < SLOTS; s += UBLOCK) {
        const uint32_t k = keys[s];
        if (k != NO_KEY) apply_entry(table, acc, k, tail);
    }
}

thread_local std::string g_err;

int check_horizon(const char* who, int64_t n, int32_t horizon) {
    if (horizon < 1 || horizon > G2048_STAGEBACK_MAX_HORIZON)
        return refuse(g_err, "%s: horizon = %d outside [1, %d]", who, horizon,
                      G2048_STAGEBACK_MAX_HORIZON);
    if (n * (int64_t)horizon > G2048_STAGEBACK_MAX_SLOTS)
        return refuse(g_err, "%s: n * horizon = %lld exceeds 2^31", who,
                      (long long)(n * (int64_t)horizon));
    return G2048_OK;
}

}  // namespace

extern "C" {

const char* g2048_stageback_last_error(void) { return g_err.c_str(); }

int32_t g2048_stageback_rate(int64_t E, int64_t A) {
    return checked_rate<RATE_BITS, G2048_STAGEBACK_MAX_A>(g_err, "stageback_rate", E, A);
}

int64_t g2048_stageback_acc_bytes(const g2048_ntuple_spec* spec,
                                  const g2048_ntstage_spec* stages) {
    return staged_acc_bytes(g_err, "stageback_acc_bytes", spec, stages);
}

int64_t g2048_stageback_traj_bytes(int64_t n, int32_t horizon) {
    const char* who = "stageback_traj_bytes";
    if (n < 1 || n > G2048_MAX_BOARDS)
        return refuse(g_err, "%s: n = %lld outside [1, G2048_MAX_BOARDS]", who, (long long)n);
    const int rc = check_horizon(who, n, horizon);
    if (rc != G2048_OK) return rc;
    return 32 * n * (int64_t)horizon;
}

int g2048_stageback_step(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                         int32_t* lut_dev, int64_t* acc_dev, int64_t* ea_dev,
                         const uint8_t* boards_dev, int64_t n, uint8_t* traj_dev,
                         int32_t* gain_dev, uint8_t* cur_dev, uint32_t* rec_dev,
                         uint32_t* rep_n_dev, uint32_t* rep_k_dev, int32_t horizon, int32_t lr_num,
                         int32_t lr_shift, uint8_t* action_out_dev, int32_t* delta_out_dev,
                         uint8_t* x_out_dev, uint8_t* replay_out_dev, int64_t* err_out_dev,
                         int device_id, void* stream) {
    const char* who = "stageback_step";
    int rc = check_staged_tc(g_err, who, spec, stages, lut_dev, boards_dev, n, acc_dev, ea_dev);
    if (rc != G2048_OK) return rc;
    rc = check_horizon(who, n, horizon);
    if (rc != G2048_OK) return rc;
    const struct {
        const char* name;
        const void* ptr;
        unsigned align;
    } ptrs[] = {{"traj_dev", traj_dev, 16},   {"gain_dev", gain_dev, 4},
                {"cur_dev", cur_dev, 1},      {"rec_dev", rec_dev, 4},
                {"rep_n_dev", rep_n_dev, 4},  {"rep_k_dev", rep_k_dev, 4},
                {"x_out_dev", x_out_dev, 16}, {"replay_out_dev", replay_out_dev, 1}};
    for (const auto& q : ptrs) {
        rc = check_ptr(g_err, who, q.name, q.ptr, q.align);
        if (rc != G2048_OK) return rc;
    }
    // x_out and replay_out stand where prev and has_prev stand: checked above, so what is left of
    // this are the rate and the three outputs of every learning step
    rc = check_td_args(g_err, who, x_out_dev, replay_out_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    const Params p = make_params(*spec);
    const StagedIndex ix{make_stage_params(*spec, *stages)};
    DeviceGuard guard(device_id);
    hipStream_t st = (hipStream_t)stream;
    const uint4* boards = reinterpret_cast<const uint4*>(boards_dev);
    uint4* x_out = reinterpret_cast<uint4*>(x_out_dev);
    const dim3 grid = grid_for(n, UBLOCK / 8);
    DISPATCH_T(spec->n_tuples,
               (k_back_policy<TT><<<policy_grid(n), dim3(POLICY_BLOCK), 0, st>>>(
                   lut_dev, boards, n, action_out_dev, reinterpret_cast<uint4*>(traj_dev), gain_dev,
                   cur_dev, rec_dev, rep_n_dev, rep_k_dev, (uint32_t)horizon, lr_num, lr_shift,
                   delta_out_dev, x_out, replay_out_dev, err_out_dev, p, ix.sp)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples,
               (k_mean_gather<TT, StagedIndex><<<grid, dim3(UBLOCK), 0, st>>>(
                   acc_dev, n, x_out, replay_out_dev, delta_out_dev, p, ix)));
    G_HIP(hipGetLastError());
    DISPATCH_T(spec->n_tuples, (k_back_apply<TT><<<grid, dim3(UBLOCK), 0, st>>>(
                                   lut_dev, acc_dev, reinterpret_cast<longlong2*>(ea_dev), n, x_out,
                                   replay_out_dev, delta_out_dev, p, ix)));
    G_HIP(hipGetLastError());
    return G2048_OK;
}

}  // extern "C"
