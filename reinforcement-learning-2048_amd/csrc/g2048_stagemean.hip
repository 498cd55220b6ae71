// g2048_stagemean.hip -- batch-mean TD learning for the multi-stage n-tuple value network on
// gfx950 (libg2048_stagemean.so).
//
// The rule is defined in include/g2048_stagemean.h; every value is an integer and the result is
// checked bit for bit against tests/stagemean_ref.py.  No float anywhere.  The library takes the
// spec, the stage spec and the table of g2048_ntstage.h and does not link against another library
// of the project.
//
// It composes g2048_ntstage_dev.hpp's staged policy launch with its fall-through and promotion
// (k_stage_policy<T, true>) with g2048_ntmean_dev.hpp's gather and apply over StagedIndex and
// MeanTail: the key of a hit is stage(prev) * stride + entry(prev, g, .), and the owner of a
// staged entry adds floor(D / C) into lut.  The policy launch promoted every entry a hit can
// address, so that add never lands on UNSET.  The step's three launches and why they need no
// further ordering are argued in the two headers.  Here are the entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stagemean.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntmean_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_stagemean_last_error(void) { return g_err.c_str(); }

int64_t g2048_stagemean_acc_bytes(const g2048_ntuple_spec* spec,
                                  const g2048_ntstage_spec* stages) {
    return staged_acc_bytes(g_err, "stagemean_acc_bytes", spec, stages);
}

int g2048_stagemean_step(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                         int32_t* lut_dev, int64_t* acc_dev, const uint8_t* boards_dev, int64_t n,
                         uint8_t* prev_dev, uint8_t* has_prev_dev, int32_t lr_num,
                         int32_t lr_shift, uint8_t* action_out_dev, int32_t* delta_out_dev,
                         int64_t* err_out_dev, int device_id, void* stream) {
    const char* who = "stagemean_step";
    int rc = check_staged(g_err, who, spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    rc = check_acc(g_err, who, acc_dev);
    if (rc != G2048_OK) return rc;
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    return mean_step<MeanTail>(g_err, *spec, StagedIndex{make_stage_params(*spec, *stages)},
                               lut_dev, acc_dev, boards_dev, n, prev_dev, has_prev_dev, lr_num,
                               lr_shift, action_out_dev, delta_out_dev, err_out_dev, device_id,
                               stream);
}

}  // extern "C"
