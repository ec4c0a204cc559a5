// rcdc_check_trees_level and rcdc_tree_names (include/rcdc.h): the host half
// -- argument checks, scratch memory and the order of the launches.  The
// kernels are in rcdc_cktree.hip.
//
// Each call stops the stream once, after the scan, to read the count that
// decides whether anything is written (findings, names); what it then
// launches is drained before it returns.  Scratch lives for one call.

#include <hip/hip_runtime.h>

#include <vector>

#include "rcdc_cktree.h"
#include "rcdc_host.h"

using namespace rcdc;

extern "C" {

rcdc_status rcdc_tree_names(rcdc_ctx *ctx, const void *d_text, uint64_t text_len,
                            const rcdc_trnode *d_nodes, uint64_t n_nodes,
                            const uint32_t *d_index, uint64_t n, uint64_t *d_offsets,
                            void *d_names, uint64_t cap_names, uint64_t *total,
                            void *hip_stream) {
    if (!ctx) return invalid("rcdc_tree_names: ctx is NULL");
    if (!total) return invalid("rcdc_tree_names: total is NULL");
    if (n && (!d_index || !d_offsets)) return invalid("rcdc_tree_names: null array");
    if (n && n_nodes && !d_nodes) return invalid("rcdc_tree_names: d_nodes is NULL");
    if (n && n_nodes && text_len && !d_text) return invalid("rcdc_tree_names: d_text is NULL");
    if (((uintptr_t)d_index & 3u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_nodes & 15u))
        return invalid("rcdc_tree_names: a misaligned array");
    if (n >= 0xFFFFFFFFull) return invalid("rcdc_tree_names: 2^32 - 1 names or more");
    *total = 0;
    if (n == 0) return RCDC_OK;

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch sc;
    uint64_t *sums = nullptr;
    HIP_TRY(sc.get(&sums, n / kCtScan + 2));
    CtNamesArgs a = {};
    a.text = static_cast<const uint8_t *>(d_text);
    a.text_len = d_text ? text_len : 0;
    a.nodes = d_nodes;
    a.n_nodes = d_nodes ? n_nodes : 0;
    a.index = d_index;
    a.n = n;
    a.offsets = d_offsets;
    a.names = static_cast<uint8_t *>(d_names);
    HIP_TRY(launch_ct_name_lens(a, st));
    HIP_TRY(launch_ct_scan(d_offsets, n, sums, st));
    HIP_TRY(hipMemcpyAsync(total, d_offsets + n, sizeof *total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (*total == 0 || !d_names || *total > cap_names) return RCDC_OK;
    HIP_TRY(launch_ct_name_copy(a, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RCDC_OK;
}

rcdc_status rcdc_check_trees_level(rcdc_ctx *ctx, const rcdc_trnode *d_nodes, uint64_t n_nodes,
                                   const void *d_data_ids, const rcdc_dindex_hit *d_data_hits,
                                   uint64_t n_data_ids, const void *d_tree_ids,
                                   const uint8_t *d_tree_is_dir,
                                   const rcdc_dindex_hit *d_tree_hits, uint64_t n_tree_ids,
                                   uint8_t *d_data_marks, uint64_t n_data_packs,
                                   uint8_t *d_tree_marks, uint64_t n_tree_packs,
                                   rcdc_cktree_finding *d_findings, uint64_t cap_findings,
                                   uint64_t *n_findings, void *hip_stream) {
    if (!ctx) return invalid("rcdc_check_trees_level: ctx is NULL");
    if (!n_findings) return invalid("rcdc_check_trees_level: n_findings is NULL");
    if ((n_nodes && !d_nodes) || (n_data_ids && (!d_data_ids || !d_data_hits)) ||
        (n_tree_ids && (!d_tree_ids || !d_tree_is_dir || !d_tree_hits)) ||
        (n_data_packs && !d_data_marks) || (n_tree_packs && !d_tree_marks))
        return invalid("rcdc_check_trees_level: null array");
    if (cap_findings && !d_findings) return invalid("rcdc_check_trees_level: d_findings is NULL");
    if (((uintptr_t)d_nodes | (uintptr_t)d_data_ids | (uintptr_t)d_tree_ids |
         (uintptr_t)d_findings) & 15u)
        return invalid("rcdc_check_trees_level: records and ids must be 16-byte aligned");
    if (((uintptr_t)d_data_hits | (uintptr_t)d_tree_hits) & 3u)
        return invalid("rcdc_check_trees_level: hit records must be 4-byte aligned");
    if (n_nodes >= 0xFFFFFFFFull || n_data_ids >= 0xFFFFFFFFull || n_tree_ids >= 0xFFFFFFFFull)
        return invalid("rcdc_check_trees_level: 2^32 - 1 nodes or ids or more");
    *n_findings = 0;
    if (n_nodes == 0) return RCDC_OK;  // no node: no id of a node either

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch sc;
    CtLevelArgs a = {};
    a.nodes = d_nodes;
    a.n_nodes = (uint32_t)n_nodes;
    a.n_data = (uint32_t)n_data_ids;
    a.n_tree = (uint32_t)n_tree_ids;
    a.data_ids = static_cast<const uint8_t *>(d_data_ids);
    a.tree_ids = static_cast<const uint8_t *>(d_tree_ids);
    a.tree_is_dir = d_tree_is_dir;
    a.data_hits = d_data_hits;
    a.tree_hits = d_tree_hits;
    a.data_marks = d_data_marks;
    a.tree_marks = d_tree_marks;
    a.n_data_packs = n_data_packs;
    a.n_tree_packs = n_tree_packs;
    a.findings = d_findings;
    a.cap_findings = cap_findings;
    uint64_t *sums = nullptr;
    HIP_TRY(sc.get(&a.id_at, n_data_ids + 1));
    HIP_TRY(sc.get(&a.node_at, n_nodes + 1));
    HIP_TRY(sc.get(&sums, (n_data_ids > n_nodes ? n_data_ids : n_nodes) / kCtScan + 2));
    HIP_TRY(launch_ct_count(a, st));
    HIP_TRY(launch_ct_scan(a.id_at, n_data_ids, sums, st));
    HIP_TRY(launch_ct_scan(a.node_at, n_nodes, sums, st));
    uint64_t ids = 0, nodes = 0;
    HIP_TRY(hipMemcpyAsync(&ids, a.id_at + n_data_ids, sizeof ids, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&nodes, a.node_at + n_nodes, sizeof nodes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_findings = ids + nodes;
    if (*n_findings == 0 || *n_findings > cap_findings) return RCDC_OK;
    HIP_TRY(launch_ct_emit(a, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RCDC_OK;
}

}  // extern "C"
