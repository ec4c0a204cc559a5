// rcdc_check_trees_level and rcdc_tree_names (include/rcdc.h): a level of
// check_trees (commands/check.rs:627-700) judged from the node records of
// rcdc_tree_nodes and the hit records of two index lookups, and the raw names
// of chosen nodes gathered out of the text arena.  gfx950, wave64.
//
// The level is count, scan, emit.  One lane per content id counts the id's
// findings (an all-zero id, an id the index lacks) and marks the pack of a
// hit; one lane per node counts the node's own finding (a file without
// content, a dir without a subtree, with an all-zero one or with one the
// index lacks) and marks the pack of a dir's hit.  No lane loops over a
// node's ids.  Both count arrays are scanned; a finding of id i of node k
// stands at id_at[i] + node_at[k], the finding of node k itself at
// node_at[k] + id_at[its data_start]: every finding of the nodes before it
// and, inside a file, of the ids before it.  The same lanes then emit, an id
// lane finding its node by a search over the records' data_start.
//
// The scan is over uint64 counts, a workgroup per kCtScan of them, one
// workgroup over their sums, and the sums added back.

#include "rcdc_cktree.h"
#include "rcdc_wave.h"

namespace {

using namespace rcdc;

typedef unsigned long long u64;

// One workgroup of kCtScan: the sum of the values of the threads before this
// one, and *all: of all of them.
__device__ u64 block_excl(u64 x, u64 *lds /* 16 */, u64 *all) {
    const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
    const u64 inc = wave_incl_add64(x);
    __syncthreads();  // a call before this one has read lds
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    u64 before = 0, sum = 0;
    for (uint32_t w = 0; w < kCtScan / 64; w++) {
        const u64 s = lds[w];
        if (w < wave) before += s;
        sum += s;
    }
    *all = sum;
    return before + inc - x;
}

__device__ __forceinline__ bool id_is_null(const uint8_t *ids, uint64_t i) {
    const u32x4v *p = reinterpret_cast<const u32x4v *>(ids + i * 32u);
    const u32x4v a = p[0], b = p[1];
    return (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0u;
}

// the pack of hit i, RCDC_DINDEX_NO_PACK where the index lacks the id
__device__ __forceinline__ uint32_t hit_pack(const rcdc_dindex_hit *hits, uint64_t i) {
    const rcdc_dindex_hit h = hits[i];
    return h.count == 0u ? RCDC_DINDEX_NO_PACK : h.loc.pack;
}

// The finding of the node itself, or -1; *pack: the pack of a dir's subtree
// that the index holds (RCDC_DINDEX_NO_PACK otherwise).
__device__ int node_finding(const CtLevelArgs &a, const rcdc_trnode &nd, uint32_t *pack) {
    *pack = RCDC_DINDEX_NO_PACK;
    if (nd.type == 0u)
        return (nd.flags & RCDC_TRNODE_CONTENT) ? -1 : (int)RCDC_CKTREE_FILE_HAS_NO_CONTENT;
    if (nd.type != 1u) return -1;
    if (!(nd.flags & RCDC_TRNODE_SUBTREE)) return (int)RCDC_CKTREE_NO_SUBTREE;
    if (nd.tree_index >= a.n_tree) return -1;  // records of another level: nothing to judge
    if (id_is_null(a.tree_ids, nd.tree_index)) return (int)RCDC_CKTREE_NULL_SUBTREE;
    *pack = hit_pack(a.tree_hits, nd.tree_index);
    return *pack == RCDC_DINDEX_NO_PACK ? (int)RCDC_CKTREE_SUBTREE_MISSING_IN_INDEX : -1;
}

__device__ __forceinline__ void put(const CtLevelArgs &a, uint64_t at, uint32_t node,
                                    uint32_t kind, uint32_t blob_num) {
    if (at >= a.cap_findings) return;  // the host checked the count: never
    *reinterpret_cast<u32x4v *>(a.findings + at) = u32x4v{node, kind, blob_num, 0u};
}

}  // namespace

// ---- the scan ---------------------------------------------------------------

__global__ __launch_bounds__(1024) void rcdc_ct_scan_kernel(uint64_t *v, uint64_t n,
                                                            uint64_t *sums) {
    __shared__ u64 lds[16];
    const uint64_t i = (uint64_t)blockIdx.x * kCtScan + threadIdx.x;
    u64 all;
    const u64 before = block_excl(i < n ? v[i] : 0, lds, &all);
    if (i < n) v[i] = before;
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// one workgroup: sums[0, m) scanned in place, the total to sums[m]
__global__ __launch_bounds__(1024) void rcdc_ct_scan_sums_kernel(uint64_t *sums, uint64_t m) {
    __shared__ u64 lds[16];
    u64 carry = 0;
    for (uint64_t base = 0; base < m; base += kCtScan) {
        const uint64_t i = base + threadIdx.x;
        u64 all;
        const u64 before = block_excl(i < m ? sums[i] : 0, lds, &all);
        if (i < m) sums[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) sums[m] = carry;
}

// also v[n]: the total
__global__ __launch_bounds__(1024) void rcdc_ct_scan_apply_kernel(uint64_t *v, uint64_t n,
                                                                  const uint64_t *sums, uint64_t m) {
    const uint64_t i = (uint64_t)blockIdx.x * kCtScan + threadIdx.x;
    if (i < n) v[i] += sums[blockIdx.x];
    if (i == 0) v[n] = sums[m];
}

// ---- the level ----------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ct_id_count_kernel(CtLevelArgs a) {
    const uint32_t i = blockIdx.x * kCtBlock + threadIdx.x;
    if (i >= a.n_data) return;
    const uint32_t pack = hit_pack(a.data_hits, i);
    const bool miss = pack == RCDC_DINDEX_NO_PACK;
    a.id_at[i] = (id_is_null(a.data_ids, i) ? 1u : 0u) + (miss ? 1u : 0u);
    if (!miss && pack < a.n_data_packs) a.data_marks[pack] = 1u;
}

__global__ __launch_bounds__(256) void rcdc_ct_node_count_kernel(CtLevelArgs a) {
    const uint32_t k = blockIdx.x * kCtBlock + threadIdx.x;
    if (k >= a.n_nodes) return;
    const rcdc_trnode nd = a.nodes[k];
    uint32_t pack;
    a.node_at[k] = node_finding(a, nd, &pack) >= 0 ? 1u : 0u;
    if (pack != RCDC_DINDEX_NO_PACK && pack < a.n_tree_packs) a.tree_marks[pack] = 1u;
}

__global__ __launch_bounds__(256) void rcdc_ct_id_emit_kernel(CtLevelArgs a) {
    const uint32_t i = blockIdx.x * kCtBlock + threadIdx.x;
    if (i >= a.n_data) return;
    if (a.id_at[i + 1] == a.id_at[i]) return;
    // the node of id i: the last record with data_start <= i (records before
    // it with the same start hold no id of d_data_ids)
    uint32_t lo = 0, hi = a.n_nodes;
    if (hi == 0 || a.nodes[0].data_start > i) return;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.nodes[mid].data_start <= i) lo = mid; else hi = mid;
    }
    uint64_t at = a.id_at[i] + a.node_at[lo];
    const uint32_t blob_num = i - a.nodes[lo].data_start;
    if (id_is_null(a.data_ids, i)) put(a, at++, lo, RCDC_CKTREE_FILE_BLOB_HAS_NULL_ID, blob_num);
    if (hit_pack(a.data_hits, i) == RCDC_DINDEX_NO_PACK)
        put(a, at, lo, RCDC_CKTREE_FILE_BLOB_NOT_IN_INDEX, blob_num);
}

__global__ __launch_bounds__(256) void rcdc_ct_node_emit_kernel(CtLevelArgs a) {
    const uint32_t k = blockIdx.x * kCtBlock + threadIdx.x;
    if (k >= a.n_nodes) return;
    if (a.node_at[k + 1] == a.node_at[k]) return;
    const rcdc_trnode nd = a.nodes[k];
    uint32_t pack;
    const int kind = node_finding(a, nd, &pack);
    if (kind < 0) return;
    const uint32_t ids_before = nd.data_start < a.n_data ? nd.data_start : a.n_data;
    put(a, a.node_at[k] + a.id_at[ids_before], k, (uint32_t)kind, 0u);
}

// ---- names ----------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ct_name_len_kernel(CtNamesArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * kCtBlock + threadIdx.x;
    if (j >= a.n) return;
    const uint32_t k = a.index[j];
    uint64_t len = 0;
    if (k < a.n_nodes) {
        const rcdc_trnode nd = a.nodes[k];
        if (nd.name_off <= a.text_len && nd.name_len <= a.text_len - nd.name_off) len = nd.name_len;
    }
    a.offsets[j] = len;
}

// One wave per name.  Where source and destination are the same distance from
// a 16-byte boundary the middle goes as 16 bytes per lane and the ragged ends
// byte by byte; elsewhere every byte goes alone.
__global__ __launch_bounds__(256) void rcdc_ct_name_copy_kernel(CtNamesArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * (kCtBlock / 64) + threadIdx.x / 64;
    if (j >= a.n) return;
    const uint64_t len = a.offsets[j + 1] - a.offsets[j];
    if (len == 0) return;  // also an index or a span the length kernel refused
    const uint8_t *src = a.text + a.nodes[a.index[j]].name_off;
    uint8_t *dst = a.names + a.offsets[j];
    const uint32_t lane = lane_id();
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15u) != 0u) {
        for (uint64_t b = lane; b < len; b += 64) dst[b] = src[b];
        return;
    }
    uint64_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    const uint64_t chunks = (len - head) / 16;
    for (uint64_t c = lane; c < chunks; c += 64)
        *reinterpret_cast<u32x4v *>(dst + head + c * 16) =
            *reinterpret_cast<const u32x4v *>(src + head + c * 16);
    const uint64_t done = head + chunks * 16;
    if (lane < len - done) dst[done + lane] = src[done + lane];
}

namespace rcdc {

hipError_t launch_ct_scan(uint64_t *v, uint64_t n, uint64_t *sums, hipStream_t st) {
    const uint64_t m = (n + kCtScan - 1) / kCtScan;
    if (m) RCDC_LAUNCH(rcdc_ct_scan_kernel, (uint32_t)m, kCtScan, v, n, sums);
    RCDC_LAUNCH(rcdc_ct_scan_sums_kernel, 1, kCtScan, sums, m);
    RCDC_LAUNCH(rcdc_ct_scan_apply_kernel, m ? (uint32_t)m : 1u, kCtScan, v, n, sums, m);
    return hipSuccess;
}

hipError_t launch_ct_count(const CtLevelArgs &a, hipStream_t st) {
    if (a.n_data) RCDC_LAUNCH(rcdc_ct_id_count_kernel, blocks(a.n_data, kCtBlock), kCtBlock, a);
    if (a.n_nodes) RCDC_LAUNCH(rcdc_ct_node_count_kernel, blocks(a.n_nodes, kCtBlock), kCtBlock, a);
    return hipSuccess;
}

hipError_t launch_ct_emit(const CtLevelArgs &a, hipStream_t st) {
    if (a.n_data) RCDC_LAUNCH(rcdc_ct_id_emit_kernel, blocks(a.n_data, kCtBlock), kCtBlock, a);
    if (a.n_nodes) RCDC_LAUNCH(rcdc_ct_node_emit_kernel, blocks(a.n_nodes, kCtBlock), kCtBlock, a);
    return hipSuccess;
}

hipError_t launch_ct_name_lens(const CtNamesArgs &a, hipStream_t st) {
    if (a.n) RCDC_LAUNCH(rcdc_ct_name_len_kernel, blocks(a.n, kCtBlock), kCtBlock, a);
    return hipSuccess;
}

hipError_t launch_ct_name_copy(const CtNamesArgs &a, hipStream_t st) {
    if (a.n) RCDC_LAUNCH(rcdc_ct_name_copy_kernel, blocks(a.n, kCtBlock / 64), kCtBlock, a);
    return hipSuccess;
}

}  // namespace rcdc
