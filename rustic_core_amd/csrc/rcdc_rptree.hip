// rcdc_repair_trees_level and rcdc_repair_spread (include/rcdc.h): the verdict
// of `repair snapshots` (commands/repair/snapshots.rs, blob/tree/modify.rs)
// over the node records of rcdc_tree_nodes.  gfx950, wave64.
//
// A level: one lane per content id finds its node by a search over the
// records' data_start and, where the index lacks the id, marks the node and
// the slot of the node's blob; one lane per node then handles the node's own
// facts -- a dir without a subtree damages its blob, a file without content is
// counted, a node with a subtree writes the edge of its d_tree_ids entry.  No
// lane loops over a node's ids.  Marks are plain byte stores of 1; the counts
// are one atomic per wave.
//
// The spread: changed[p] |= changed[c] over the edges, a lane per edge, a
// round per launch, until a round sets nothing.

#include "rcdc_rptree.h"
#include "rcdc_wave.h"

namespace {

using namespace rcdc;

typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool hit_missing(const rcdc_dindex_hit *hits, uint64_t i) {
    const rcdc_dindex_hit h = hits[i];
    return h.count == 0u || h.loc.pack == RCDC_DINDEX_NO_PACK;
}

// the whole wave arrives; lane 0 adds the wave's count
__device__ __forceinline__ void wave_count(bool mine, unsigned long long *ctr) {
    const unsigned long long n = __popcll(__ballot(mine));
    if (lane_id() == 0 && n) atomicAdd(ctr, n);
}

// the slot of blob b, RCDC_REPAIR_NO_EDGE where there is none
__device__ __forceinline__ uint32_t slot_of(const RpLevelArgs &a, uint32_t b) {
    if (b >= a.n_blobs) return RCDC_REPAIR_NO_EDGE;
    const uint32_t s = a.blob_slot[b];
    return s < a.n_slots ? s : RCDC_REPAIR_NO_EDGE;
}

}  // namespace

__global__ __launch_bounds__(256) void rcdc_rp_id_kernel(RpLevelArgs a) {
    const uint32_t i = blockIdx.x * kRpBlock + threadIdx.x;
    bool missing = false;
    if (i < a.n_data && a.n_nodes && a.nodes[0].data_start <= i && hit_missing(a.data_hits, i)) {
        // the node of id i: the last record with data_start <= i (records
        // before it with the same start hold no id of d_data_ids)
        uint32_t lo = 0, hi = a.n_nodes;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.nodes[mid].data_start <= i) lo = mid; else hi = mid;
        }
        const rcdc_trnode nd = a.nodes[lo];
        // ids past the node's own belong to records of another call: not judged
        if (nd.type == 0u && i - nd.data_start < nd.n_content) {
            missing = true;
            a.node_bad[lo] = 1u;
            const uint32_t s = slot_of(a, nd.blob);
            if (s != RCDC_REPAIR_NO_EDGE) a.damaged[s] = 1u;
        }
    }
    wave_count(missing, a.ctr + 0);
}

__global__ __launch_bounds__(256) void rcdc_rp_node_kernel(RpLevelArgs a) {
    const uint32_t k = blockIdx.x * kRpBlock + threadIdx.x;
    bool bad = false, no_content = false;
    if (k < a.n_nodes) {
        const rcdc_trnode nd = a.nodes[k];
        const uint32_t s = slot_of(a, nd.blob);
        if (nd.type == 0u) {
            no_content = !(nd.flags & RCDC_TRNODE_CONTENT);
            bad = a.node_bad[k] != 0u;
        } else if (nd.type == 1u && !(nd.flags & RCDC_TRNODE_SUBTREE)) {
            bad = true;
            if (s != RCDC_REPAIR_NO_EDGE) a.damaged[s] = 1u;
        }
        if ((nd.flags & RCDC_TRNODE_SUBTREE) && nd.tree_index < a.n_tree) {
            u32x2v e = {RCDC_REPAIR_NO_EDGE, RCDC_REPAIR_NO_EDGE};
            if (a.tree_is_dir[nd.tree_index] && s != RCDC_REPAIR_NO_EDGE) {
                const rcdc_dindex_hit h = a.tree_hits[nd.tree_index];
                if (h.count != 0u && h.entry < a.n_slots) e = u32x2v{s, h.entry};
            }
            *reinterpret_cast<u32x2v *>(a.edges + nd.tree_index) = e;
        }
        if (no_content) atomicMin(a.ctr + 3, (unsigned long long)k);
    }
    wave_count(bad, a.ctr + 1);
    wave_count(no_content, a.ctr + 2);
}

__global__ __launch_bounds__(256) void rcdc_rp_spread_kernel(RpSpreadArgs a, uint32_t *set) {
    const uint64_t i = (uint64_t)blockIdx.x * kRpBlock + threadIdx.x;
    bool mine = false;
    if (i < a.n_edges) {
        const u32x2v e = *reinterpret_cast<const u32x2v *>(a.edges + i);
        if (e.x < a.n_slots && e.y < a.n_slots && a.changed[e.y] != 0u && a.changed[e.x] == 0u) {
            a.changed[e.x] = 1u;
            mine = true;
        }
    }
    if (__ballot(mine) != 0ull && lane_id() == 0) *set = 1u;
}

namespace rcdc {

hipError_t launch_rp_level(const RpLevelArgs &a, hipStream_t st) {
    if (a.n_data) RCDC_LAUNCH(rcdc_rp_id_kernel, blocks(a.n_data, kRpBlock), kRpBlock, a);
    if (a.n_nodes) RCDC_LAUNCH(rcdc_rp_node_kernel, blocks(a.n_nodes, kRpBlock), kRpBlock, a);
    return hipSuccess;
}

hipError_t launch_rp_spread_round(const RpSpreadArgs &a, uint32_t *set, hipStream_t st) {
    if (a.n_edges) RCDC_LAUNCH(rcdc_rp_spread_kernel, blocks(a.n_edges, kRpBlock), kRpBlock, a, set);
    return hipSuccess;
}

}  // namespace rcdc
