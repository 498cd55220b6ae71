// g2048_stagemeantc.hip -- temporal-coherence learning on the batch-mean rule for the multi-stage
// n-tuple value network on gfx950 (libg2048_stagemeantc.so).
//
// The rule is defined in include/g2048_stagemeantc.h; every value is an integer and the result is
// checked bit for bit against tests/stagemeantc_ref.py.  No float anywhere.  The library takes the
// spec, the stage spec and the table of g2048_ntstage.h and does not link against another library
// of the project.
//
// It composes g2048_ntstage_dev.hpp's staged policy launch with its fall-through and promotion
// (k_stage_policy<T, true>) and g2048_ntuple_dev.hpp's rate (tc_rate) with g2048_ntmean_dev.hpp's
// gather and apply over StagedIndex and TcTail: the owner of a STAGED entry forms
// m = floor(D / C) and, if m != 0, loads that entry's (E, A), adds (m * rate) >> RATE_BITS into
// lut and stores (E + m, A + |m|).  ea is no argument of the policy launch: promotion copies the
// weight only.  The step's three launches, why promotion needs no ordering and why ea needs no
// atomics are argued in the headers; g2048_stagedelay.hip and g2048_stageback.hip put the same
// rule, the same checked rate and the same opening checks on their own schedules.  Here are the
// entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stagemeantc.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntmean_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int RATE_BITS = G2048_STAGEMEANTC_RATE_BITS;

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_stagemeantc_last_error(void) { return g_err.c_str(); }

int32_t g2048_stagemeantc_rate(int64_t E, int64_t A) {
    return checked_rate<RATE_BITS, G2048_STAGEMEANTC_MAX_A>(g_err, "stagemeantc_rate", E, A);
}

int64_t g2048_stagemeantc_acc_bytes(const g2048_ntuple_spec* spec,
                                    const g2048_ntstage_spec* stages) {
    return staged_acc_bytes(g_err, "stagemeantc_acc_bytes", spec, stages);
}

int g2048_stagemeantc_step(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                           int32_t* lut_dev, int64_t* acc_dev, int64_t* ea_dev,
                           const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                           uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                           uint8_t* action_out_dev, int32_t* delta_out_dev, int64_t* err_out_dev,
                           int device_id, void* stream) {
    const char* who = "stagemeantc_step";
    int rc = check_staged_tc(g_err, who, spec, stages, lut_dev, boards_dev, n, acc_dev, ea_dev);
    if (rc != G2048_OK) return rc;
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    return mean_step<TcTail<RATE_BITS>>(
        g_err, *spec, StagedIndex{make_stage_params(*spec, *stages)}, lut_dev, acc_dev, boards_dev,
        n, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev, delta_out_dev, err_out_dev,
        device_id, stream, reinterpret_cast<longlong2*>(ea_dev));
}

}  // extern "C"
