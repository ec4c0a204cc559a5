// rcdc_tree_parse and rcdc_tree_nodes (include/rcdc.h): the host half --
// argument checks, the tile table, scratch memory and the order of the
// launches.  The kernels are in rcdc_trparse.hip.
//
// The call stops the stream twice: once after the structural pass, to size
// the record arrays from its four totals, and once at the end, to hand the
// per-blob records to the caller.  Scratch lives for one call.

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rcdc_host.h"
#include "rcdc_trparse.h"

using namespace rcdc;

extern "C" {

void rcdc_tree_parse_bound(uint64_t len, uint64_t *max_data_ids, uint64_t *max_tree_ids,
                           uint64_t *max_nodes) {
    // n content ids and their commas: 67 n - 1 bytes; n nodes with a subtree:
    // 102 n - 1; n nodes: 25 n - 1 (rcdc.h)
    if (max_data_ids) *max_data_ids = (len + 1) / 67;
    if (max_tree_ids) *max_tree_ids = (len + 1) / 102;
    if (max_nodes) *max_nodes = (len + 1) / 25;
}

uint32_t rcdc_tree_parse_tile(void) { return RCDC_TRPARSE_TILE; }

}  // extern "C"

namespace {

struct Fail {
    const char *fn;
    rcdc_status operator()(const char *what) const {
        return invalid((std::string(fn) + ": " + what).c_str());
    }
};

// rcdc_tree_parse, and rcdc_tree_nodes where `nodes` is set: then the grammar
// is G_N, d_nodes takes the records and node_start (n_blobs) their starts.
rcdc_status tree_parse(const char *fn, bool nodes, rcdc_ctx *ctx, const void *d_text,
                       uint64_t text_len, const rcdc_trparse_ref *refs, uint32_t n_blobs,
                       void *d_data_ids, uint64_t cap_data_ids, void *d_tree_ids,
                       uint8_t *d_tree_is_dir, uint64_t cap_tree_ids, rcdc_trnode *d_nodes,
                       uint64_t cap_nodes, uint64_t *node_start, rcdc_trparse_blob *blobs,
                       rcdc_trparse_result *result, void *hip_stream) {
    const Fail fail = {fn};
    if (!ctx) return fail("ctx is NULL");
    if (!result) return fail("result is NULL");
    if (n_blobs && (!refs || !blobs)) return fail("null array");
    if (nodes && n_blobs && !d_nodes) return fail("d_nodes is NULL");
    uint64_t need_nodes = 0;
    uint64_t need_data = 0, need_tree = 0, n_tiles = 0, bytes = 0;
    std::vector<uint32_t> tile_first;
    switch (tile_table(refs, n_blobs, text_len, d_text, kTrTile, tile_first, n_tiles,
                       [&](uint64_t len) {
        uint64_t d = 0, t = 0, nn = 0;
        rcdc_tree_parse_bound(len, &d, &t, &nn);
        need_data += d;
        need_tree += t;
        need_nodes += nn;
        bytes += len;
        // every count of the structural pass is a count of bytes
        return bytes < 0xFFFFFFFFull;
    })) {
    case TileTable::RefOutside: return fail("a ref lies outside the arena");
    case TileTable::ArenaNull: return fail("d_text is NULL");
    case TileTable::TooMany: return fail("the batch holds 2^32 - 1 bytes or more");
    case TileTable::Ok: break;
    }
    if ((d_data_ids && cap_data_ids < need_data) ||
        ((d_tree_ids || d_tree_is_dir) && cap_tree_ids < need_tree) ||
        (nodes && cap_nodes < need_nodes))
        return fail("capacities below rcdc_tree_parse_bound");
    if (((uintptr_t)d_data_ids & 15u) || ((uintptr_t)d_tree_ids & 15u))
        return fail("the id arrays must be 16-byte aligned");
    if (nodes && ((uintptr_t)d_nodes & 15u)) return fail("d_nodes must be 16-byte aligned");
    *result = rcdc_trparse_result{};
    if (n_blobs == 0) return RCDC_OK;

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch sc;
    TrArgs a = {};
    a.text = static_cast<const uint8_t *>(d_text);
    a.text_len = text_len;
    a.n_blobs = n_blobs;
    a.n_tiles = (uint32_t)n_tiles;
    a.gn = nodes ? 1u : 0u;
    rcdc_trparse_ref *d_refs = nullptr;
    uint32_t *d_tile_first = nullptr;
    HIP_TRY(sc.get(&d_refs, n_blobs));
    HIP_TRY(sc.get(&d_tile_first, n_blobs + 1ull));
    HIP_TRY(sc.get(&a.sums, n_tiles));
    HIP_TRY(sc.get(&a.ins, n_tiles));
    HIP_TRY(sc.get(&a.esc, n_tiles));
    HIP_TRY(sc.get(&a.counts, n_tiles + 1));
    HIP_TRY(sc.get(&a.blob_ok, n_blobs));
    HIP_TRY(sc.get(&a.blob_bad, n_blobs));
    HIP_TRY(hipMemcpyAsync(d_refs, refs, n_blobs * sizeof *refs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tile_first, tile_first.data(), (n_blobs + 1ull) * 4,
                          hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.blob_bad, 0, n_blobs * 4ull, st));
    a.refs = d_refs;
    a.tile_first = d_tile_first;
    HIP_TRY(launch_tr_structure(a, st));
    HIP_TRY(hipMemcpyAsync(&a.total, a.counts + n_tiles, sizeof a.total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    HIP_TRY(sc.get(&a.node_open, a.total.n[kTrNode]));
    HIP_TRY(sc.get(&a.id_open, a.total.n[kTrId]));
    HIP_TRY(sc.get(&a.c4, a.total.n[kTrC4]));
    HIP_TRY(sc.get(&a.c2, a.total.n[kTrC2]));
    HIP_TRY(sc.get(&a.tmp_ids, (uint64_t)a.total.n[kTrId] * 32));
    HIP_TRY(sc.get(&a.tmp_nodes, a.total.n[kTrNode]));
    uint32_t *adds = nullptr;
    HIP_TRY(sc.get(&adds, ((uint64_t)a.total.n[kTrNode] + 1) * 4));
    a.adds = adds;
    uint32_t *add_sums = nullptr;
    HIP_TRY(sc.get(&add_sums, ((uint64_t)a.total.n[kTrNode] / kTrScan + 2) * 4));
    a.add_sums = add_sums;
    HIP_TRY(sc.get(&a.blobs, n_blobs));
    a.data_ids = static_cast<uint8_t *>(d_data_ids);
    a.tree_ids = static_cast<uint8_t *>(d_tree_ids);
    a.tree_is_dir = d_tree_is_dir;
    // counted, not written: no capacity to hold the lanes to
    a.cap_data_ids = d_data_ids ? cap_data_ids : ~0ull;
    a.cap_tree_ids = (d_tree_ids || d_tree_is_dir) ? cap_tree_ids : ~0ull;
    if (nodes) {
        a.nodes = d_nodes;
        a.cap_nodes = cap_nodes;
        HIP_TRY(sc.get(&a.node_start, n_blobs));
    }
    HIP_TRY(launch_tr_parse(a, st));
    uint32_t tot[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, adds + (uint64_t)a.total.n[kTrNode] * 4, sizeof tot,
                          hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(blobs, a.blobs, n_blobs * sizeof *blobs, hipMemcpyDeviceToHost, st));
    if (nodes)
        HIP_TRY(hipMemcpyAsync(node_start, a.node_start, n_blobs * sizeof *node_start,
                              hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[0] > a.cap_data_ids || tot[1] > a.cap_tree_ids || (nodes && tot[2] > cap_nodes))
        return set_error(RCDC_ERR_INTERNAL,
                         (std::string(fn) + ": more output than the bound allows").c_str());
    result->data_ids = tot[0];
    result->tree_ids = tot[1];
    result->nodes = tot[2];
    for (uint32_t b = 0; b < n_blobs; b++)
        result->blobs_not_parsed += blobs[b].status != RCDC_TRPARSE_OK;
    return RCDC_OK;
}

}  // namespace

extern "C" {

rcdc_status rcdc_tree_parse(rcdc_ctx *ctx, const void *d_text, uint64_t text_len,
                            const rcdc_trparse_ref *refs, uint32_t n_blobs, void *d_data_ids,
                            uint64_t cap_data_ids, void *d_tree_ids, uint8_t *d_tree_is_dir,
                            uint64_t cap_tree_ids, rcdc_trparse_blob *blobs,
                            rcdc_trparse_result *result, void *hip_stream) {
    return tree_parse("rcdc_tree_parse", false, ctx, d_text, text_len, refs, n_blobs, d_data_ids,
                      cap_data_ids, d_tree_ids, d_tree_is_dir, cap_tree_ids, nullptr, 0, nullptr,
                      blobs, result, hip_stream);
}

void rcdc_tree_nodes_bound(uint64_t len, uint64_t *max_data_ids, uint64_t *max_tree_ids,
                           uint64_t *max_nodes) {
    rcdc_tree_parse_bound(len, max_data_ids, max_tree_ids, max_nodes);
}

rcdc_status rcdc_tree_nodes(rcdc_ctx *ctx, const void *d_text, uint64_t text_len,
                            const rcdc_trparse_ref *refs, uint32_t n_blobs, void *d_data_ids,
                            uint64_t cap_data_ids, void *d_tree_ids, uint8_t *d_tree_is_dir,
                            uint64_t cap_tree_ids, rcdc_trnode *d_nodes, uint64_t cap_nodes,
                            rcdc_trnodes_blob *blobs, rcdc_trparse_result *result,
                            void *hip_stream) {
    if (n_blobs && !blobs) return invalid("rcdc_tree_nodes: null array");
    std::vector<rcdc_trparse_blob> ids(n_blobs);
    std::vector<uint64_t> starts(n_blobs, 0);
    const rcdc_status st =
        tree_parse("rcdc_tree_nodes", true, ctx, d_text, text_len, refs, n_blobs, d_data_ids,
                   cap_data_ids, d_tree_ids, d_tree_is_dir, cap_tree_ids, d_nodes, cap_nodes,
                   starts.data(), ids.data(), result, hip_stream);
    if (st != RCDC_OK) return st;
    for (uint32_t b = 0; b < n_blobs; b++)
        blobs[b] = rcdc_trnodes_blob{ids[b].status,     ids[b].nodes,      ids[b].data_ids,
                                     ids[b].tree_ids,   ids[b].data_start, ids[b].tree_start,
                                     starts[b]};
    return RCDC_OK;
}

}  // extern "C"
