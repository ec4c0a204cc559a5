// rcdc_repair_trees_level and rcdc_repair_spread: what the host half
// (rcdc_rptree.cpp) and the kernels (rcdc_rptree.hip) share.  Included by
// those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"

namespace rcdc {

constexpr uint32_t kRpBlock = 256;
// rounds of the spread launched between two reads of their "set something"
// words
constexpr uint32_t kRpRoundsPerLaunch = RCDC_REPAIR_SPREAD_ROUNDS;

struct RpLevelArgs {
    const rcdc_trnode *nodes;
    uint32_t n_nodes, n_data, n_tree, n_blobs;
    const rcdc_dindex_hit *data_hits, *tree_hits;
    const uint8_t *tree_is_dir;
    const uint32_t *blob_slot;
    uint8_t *damaged;
    uint64_t n_slots;
    rcdc_repair_edge *edges;
    uint8_t *node_bad;  // scratch, n_nodes bytes, zeroed: a file node with a missing id
    // scratch: missing ids, damaged nodes, files without content, the lowest of them
    unsigned long long *ctr;
};

struct RpSpreadArgs {
    const rcdc_repair_edge *edges;
    uint64_t n_edges;
    uint8_t *changed;
    uint64_t n_slots;
};

hipError_t launch_rp_level(const RpLevelArgs &a, hipStream_t st);
// one round; *set (device) becomes non-zero where the round set a byte
hipError_t launch_rp_spread_round(const RpSpreadArgs &a, uint32_t *set, hipStream_t st);

}  // namespace rcdc
