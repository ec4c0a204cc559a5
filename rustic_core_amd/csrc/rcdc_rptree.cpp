// rcdc_repair_trees_level and rcdc_repair_spread (include/rcdc.h): the host
// half -- argument checks, scratch memory and the order of the launches.  The
// kernels are in rcdc_rptree.hip.
//
// The level call stops the stream once, to read its four counts.  The spread
// launches RCDC_REPAIR_SPREAD_ROUNDS rounds, each with a word of its own that
// says whether it set a byte, and reads those words in one copy; it ends at
// the first round that set nothing.  Every round but the last sets at least
// one byte that was 0 and no byte goes back to 0, so there are at most
// n_slots + 1 rounds on any edge list.  Scratch lives for one call.

#include <hip/hip_runtime.h>

#include "rcdc_host.h"
#include "rcdc_rptree.h"

using namespace rcdc;

extern "C" {

uint32_t rcdc_repair_spread_rounds_per_launch(void) { return kRpRoundsPerLaunch; }

rcdc_status rcdc_repair_trees_level(rcdc_ctx *ctx, const rcdc_trnode *d_nodes, uint64_t n_nodes,
                                    const rcdc_dindex_hit *d_data_hits, uint64_t n_data_ids,
                                    const uint8_t *d_tree_is_dir,
                                    const rcdc_dindex_hit *d_tree_hits, uint64_t n_tree_ids,
                                    const uint32_t *d_blob_slot, uint64_t n_blobs,
                                    uint8_t *d_damaged, uint64_t n_slots,
                                    rcdc_repair_edge *d_edges, rcdc_repair_level_result *result,
                                    void *hip_stream) {
    if (!ctx) return invalid("rcdc_repair_trees_level: ctx is NULL");
    if (!result) return invalid("rcdc_repair_trees_level: result is NULL");
    if ((n_nodes && !d_nodes) || (n_data_ids && !d_data_hits) ||
        (n_tree_ids && (!d_tree_is_dir || !d_tree_hits || !d_edges)) ||
        (n_blobs && !d_blob_slot) || (n_slots && !d_damaged))
        return invalid("rcdc_repair_trees_level: null array");
    if ((uintptr_t)d_nodes & 15u)
        return invalid("rcdc_repair_trees_level: records must be 16-byte aligned");
    if ((uintptr_t)d_edges & 7u)
        return invalid("rcdc_repair_trees_level: edges must be 8-byte aligned");
    if (((uintptr_t)d_data_hits | (uintptr_t)d_tree_hits | (uintptr_t)d_blob_slot) & 3u)
        return invalid("rcdc_repair_trees_level: hit records and slots must be 4-byte aligned");
    if (n_nodes >= 0xFFFFFFFFull || n_data_ids >= 0xFFFFFFFFull || n_tree_ids >= 0xFFFFFFFFull ||
        n_blobs >= 0xFFFFFFFFull || n_slots >= 0xFFFFFFFFull)
        return invalid("rcdc_repair_trees_level: 2^32 - 1 nodes, ids, blobs or slots or more");
    *result = rcdc_repair_level_result{0, 0, 0, RCDC_REPAIR_NO_NODE};
    if (n_nodes == 0) return RCDC_OK;  // no node: no id and no subtree of a node either

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch sc;
    RpLevelArgs a = {};
    a.nodes = d_nodes;
    a.n_nodes = (uint32_t)n_nodes;
    a.n_data = (uint32_t)n_data_ids;
    a.n_tree = (uint32_t)n_tree_ids;
    a.n_blobs = (uint32_t)n_blobs;
    a.data_hits = d_data_hits;
    a.tree_hits = d_tree_hits;
    a.tree_is_dir = d_tree_is_dir;
    a.blob_slot = d_blob_slot;
    a.damaged = d_damaged;
    a.n_slots = n_slots;
    a.edges = d_edges;
    HIP_TRY(sc.get(&a.node_bad, n_nodes));
    HIP_TRY(sc.get(&a.ctr, 4));
    HIP_TRY(hipMemsetAsync(a.node_bad, 0, n_nodes, st));
    HIP_TRY(hipMemsetAsync(a.ctr, 0, 3 * sizeof *a.ctr, st));
    HIP_TRY(hipMemsetAsync(a.ctr + 3, 0xFF, sizeof *a.ctr, st));
    HIP_TRY(launch_rp_level(a, st));
    unsigned long long got[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(got, a.ctr, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    result->missing_ids = got[0];
    result->damaged_nodes = got[1];
    result->files_without_content = got[2];
    result->first_without_content = got[2] ? got[3] : RCDC_REPAIR_NO_NODE;
    return RCDC_OK;
}

rcdc_status rcdc_repair_spread(rcdc_ctx *ctx, const rcdc_repair_edge *d_edges, uint64_t n_edges,
                               const uint8_t *d_damaged, uint8_t *d_changed, uint64_t n_slots,
                               uint64_t *rounds, void *hip_stream) {
    if (!ctx) return invalid("rcdc_repair_spread: ctx is NULL");
    if (!rounds) return invalid("rcdc_repair_spread: rounds is NULL");
    if ((n_edges && !d_edges) || (n_slots && (!d_damaged || !d_changed)))
        return invalid("rcdc_repair_spread: null array");
    if ((uintptr_t)d_edges & 7u) return invalid("rcdc_repair_spread: edges must be 8-byte aligned");
    if (n_edges >= 0xFFFFFFFFull || n_slots >= 0xFFFFFFFFull)
        return invalid("rcdc_repair_spread: 2^32 - 1 edges or slots or more");
    *rounds = 0;
    if (n_slots == 0) return RCDC_OK;

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_changed != d_damaged)
        HIP_TRY(hipMemcpyAsync(d_changed, d_damaged, n_slots, hipMemcpyDeviceToDevice, st));
    if (n_edges == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        return RCDC_OK;
    }
    Scratch sc;
    uint32_t *set = nullptr;
    HIP_TRY(sc.get(&set, kRpRoundsPerLaunch));
    RpSpreadArgs a = {d_edges, n_edges, d_changed, n_slots};
    for (;;) {
        uint32_t got[kRpRoundsPerLaunch];
        HIP_TRY(hipMemsetAsync(set, 0, sizeof got, st));
        for (uint32_t r = 0; r < kRpRoundsPerLaunch; r++)
            HIP_TRY(launch_rp_spread_round(a, set + r, st));
        HIP_TRY(hipMemcpyAsync(got, set, sizeof got, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t r = 0; r < kRpRoundsPerLaunch; r++) {
            ++*rounds;
            if (!got[r]) return RCDC_OK;  // the rounds behind it found the same fixed point
        }
        if (*rounds > n_slots + kRpRoundsPerLaunch)  // cannot be: every such round set a byte
            return set_error(RCDC_ERR_INTERNAL, "rcdc_repair_spread: no fixed point");
    }
}

}  // extern "C"
