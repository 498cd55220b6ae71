// g2048_ntsearch.hip -- expectimax search over the n-tuple value network for gfx950
// (libg2048_ntsearch.so).
//
// The search is defined in include/g2048_ntsearch.h and checked bit for bit against
// tests/ntsearch_ref.py.  The tree walk, the kernel and the launch are g2048_ntsearch_dev.hpp's;
// the leaf is its FlatLeaf: 8 T gathers from the one table, nothing to settle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_ntsearch.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntsearch_dev.hpp"

#ifndef G2048_NTSEARCH_LEAF_TUPLES
#define G2048_NTSEARCH_LEAF_TUPLES 2  // tuples per burst of 8 gathers each
#endif

namespace {

using namespace g2048::nt;

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_ntsearch_last_error(void) { return g_err.c_str(); }

int g2048_ntsearch_expectimax(const g2048_ntuple_spec* spec, const int32_t* lut_dev,
                              const uint8_t* boards_dev, int64_t n, int depth, uint32_t flags,
                              int64_t* values_out_dev, uint8_t* action_out_dev, int device_id,
                              void* stream) {
    const char* who = "ntsearch_expectimax";
    const int rc = check_common(g_err, who, spec, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    return search_launch<G2048_NTSEARCH_LEAF_TUPLES>(
        g_err, who, G2048_NTSEARCH_MAX_DEPTH, make_params(*spec), FlatLeaf{}, lut_dev, boards_dev,
        n, depth, flags, values_out_dev, action_out_dev, device_id, stream);
}

}  // extern "C"
