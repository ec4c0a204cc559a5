// rcdc_check_trees_level and rcdc_tree_names: what the host half
// (rcdc_cktree.cpp) and the kernels (rcdc_cktree.hip) share.  Included by
// those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"

namespace rcdc {

constexpr uint32_t kCtBlock = 256;
constexpr uint32_t kCtScan = 1024;  // counts per workgroup of the scan

struct CtLevelArgs {
    const rcdc_trnode *nodes;
    uint32_t n_nodes, n_data, n_tree;
    const uint8_t *data_ids, *tree_ids, *tree_is_dir;
    const rcdc_dindex_hit *data_hits, *tree_hits;
    uint8_t *data_marks, *tree_marks;
    uint64_t n_data_packs, n_tree_packs;
    // scratch: findings per id / per node, then (scanned) before it; [n]: all
    uint64_t *id_at, *node_at;
    rcdc_cktree_finding *findings;
    uint64_t cap_findings;
};

struct CtNamesArgs {
    const uint8_t *text;
    uint64_t text_len;
    const rcdc_trnode *nodes;
    uint64_t n_nodes;
    const uint32_t *index;
    uint64_t n;
    uint64_t *offsets;  // n + 1
    uint8_t *names;
};

// In-place exclusive scan of v[0, n), the total to v[n]; sums: scratch of
// n / kCtScan + 2 counts.
hipError_t launch_ct_scan(uint64_t *v, uint64_t n, uint64_t *sums, hipStream_t st);
hipError_t launch_ct_count(const CtLevelArgs &a, hipStream_t st);
hipError_t launch_ct_emit(const CtLevelArgs &a, hipStream_t st);
hipError_t launch_ct_name_lens(const CtNamesArgs &a, hipStream_t st);
hipError_t launch_ct_name_copy(const CtNamesArgs &a, hipStream_t st);

}  // namespace rcdc
