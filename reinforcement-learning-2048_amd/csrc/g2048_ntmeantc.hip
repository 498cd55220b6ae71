// g2048_ntmeantc.hip -- temporal-coherence learning on the batch-mean rule for the n-tuple value
// network on gfx950 (libg2048_ntmeantc.so).
//
// The rule is defined in include/g2048_ntmeantc.h; every value is an integer and the result is
// checked bit for bit against tests/ntmeantc_ref.py.  No float anywhere.  The library takes the
// spec and the table of g2048_ntuple.h and does not link against another library of the project.
//
// It composes g2048_ntuple_dev.hpp's flat policy launch (k_policy<T, true>) and rate (tc_rate)
// with g2048_ntmean_dev.hpp's gather and apply over FlatIndex and TcTail: the owner of an entry
// forms m = floor(D / C) and, if m != 0, loads (E, A), adds (m * rate) >> RATE_BITS into lut and
// stores (E + m, A + |m|).  The step's three launches, and why ea needs no atomics, are argued in
// g2048_ntmean_dev.hpp.  Here are the entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_ntmeantc.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntmean_dev.hpp"

namespace {

using namespace g2048;
using namespace g2048::nt;

constexpr int RATE_BITS = G2048_NTMEANTC_RATE_BITS;

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_ntmeantc_last_error(void) { return g_err.c_str(); }

int32_t g2048_ntmeantc_rate(int64_t E, int64_t A) {
    return checked_rate<RATE_BITS, G2048_NTMEANTC_MAX_A>(g_err, "ntmeantc_rate", E, A);
}

int64_t g2048_ntmeantc_acc_bytes(const g2048_ntuple_spec* spec) {
    const int rc = nt::check_spec(g_err, "ntmeantc_acc_bytes", spec);
    if (rc != G2048_OK) return rc;
    return table_bytes(*spec);
}

int g2048_ntmeantc_step(const g2048_ntuple_spec* spec, int32_t* lut_dev, int64_t* acc_dev,
                        int64_t* ea_dev, const uint8_t* boards_dev, int64_t n, uint8_t* prev_dev,
                        uint8_t* has_prev_dev, int32_t lr_num, int32_t lr_shift,
                        uint8_t* action_out_dev, int32_t* delta_out_dev, int64_t* err_out_dev,
                        int device_id, void* stream) {
    const char* who = "ntmeantc_step";
    int rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    rc = check_acc(g_err, who, acc_dev);
    if (rc != G2048_OK) return rc;
    rc = check_ea(g_err, who, ea_dev, acc_dev, table_bytes(*spec));
    if (rc != G2048_OK) return rc;
    rc = check_td_args(g_err, who, prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                       delta_out_dev, err_out_dev);
    if (rc != G2048_OK) return rc;
    return mean_step<TcTail<RATE_BITS>>(g_err, *spec, FlatIndex{}, lut_dev, acc_dev, boards_dev, n,
                                        prev_dev, has_prev_dev, lr_num, lr_shift, action_out_dev,
                                        delta_out_dev, err_out_dev, device_id, stream,
                                        reinterpret_cast<longlong2*>(ea_dev));
}

}  // extern "C"
