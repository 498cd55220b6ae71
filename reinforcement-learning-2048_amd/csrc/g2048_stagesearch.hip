// g2048_stagesearch.hip -- expectimax search over the multi-stage n-tuple network for gfx950
// (libg2048_stagesearch.so).
//
// The search is defined in include/g2048_stagesearch.h: g2048_ntsearch.h's tree with
// g2048_ntstage.h's V at the leaves.  Every value is an int64 and the result is checked bit for
// bit against tests/stagesearch_ref.py.  No float anywhere.  The table is only read.
//
// The tree walk, the kernel and the launch are g2048_ntsearch_dev.hpp's, the same code as the
// single-table search runs.  The leaf (StagedLeaf: the stage of a leaf from its own bytes, the
// fall-through over UNSET entries) is g2048_stageleaf_dev.hpp's, shared with the deep search.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/g2048_stagesearch.h"
#include "g2048_board.hpp"
#include "g2048_ntuple_dev.hpp"
#include "g2048_ntstage_dev.hpp"
#include "g2048_ntsearch_dev.hpp"
#include "g2048_stageleaf_dev.hpp"

#ifndef G2048_STAGESEARCH_LEAF_TUPLES
#define G2048_STAGESEARCH_LEAF_TUPLES 2  // tuples per burst of 8 gathers each
#endif

namespace {

using namespace g2048;
using namespace g2048::nt;

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* g2048_stagesearch_last_error(void) { return g_err.c_str(); }

int g2048_stagesearch_expectimax(const g2048_ntuple_spec* spec, const g2048_ntstage_spec* stages,
                                 const int32_t* lut_dev, const uint8_t* boards_dev, int64_t n,
                                 int depth, uint32_t flags, int64_t* values_out_dev,
                                 uint8_t* action_out_dev, int device_id, void* stream) {
    const char* who = "stagesearch_expectimax";
    const int rc = check_staged(g_err, who, spec, stages, lut_dev, boards_dev, n);
    if (rc != G2048_OK) return rc;
    return search_launch<G2048_STAGESEARCH_LEAF_TUPLES>(
        g_err, who, G2048_STAGESEARCH_MAX_DEPTH, make_params(*spec),
        StagedLeaf{make_stage_params(*spec, *stages)}, lut_dev, boards_dev, n, depth, flags,
        values_out_dev, action_out_dev, device_id, stream);
}

}  // extern "C"
