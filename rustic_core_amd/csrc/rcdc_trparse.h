// rcdc_tree_parse: what the host half (rcdc_trparse.cpp) and the kernels
// (rcdc_trparse.hip) share.  Included by those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"
#include "rcdc_json_tiles.h"

namespace rcdc {

constexpr uint32_t kTrTile = RCDC_TRPARSE_TILE;  // bytes per tile: one wave
constexpr uint32_t kTrBlock = 256;               // 4 tiles per workgroup
constexpr uint32_t kTrScan = 1024;               // node records per workgroup of the numbering's scan

// The structural pass's records (rcdc_json_tiles.h).  The event kinds, in
// the order of TileCounts::n: node opens ('{' at depth 2), string opens at
// depth 4 (the elements of "content"), ']' at depth 4 (closes "content" or
// "extended_attributes") and ']' at depth 2 (closes "nodes").
enum TrEvent : uint32_t { kTrNode, kTrId, kTrC4, kTrC2 };
struct TrGrammar {
    // ch is a byte that counts, outside a string; -1: no event
    RCDC_JT_FN static int event_of(uint8_t ch, int32_t depth) {
        if (ch == '{') return depth == 2 ? (int)kTrNode : -1;
        if (ch == '"') return depth == 4 ? (int)kTrId : -1;
        if (ch == ']') return depth == 4 ? (int)kTrC4 : depth == 2 ? (int)kTrC2 : -1;
        return -1;
    }
};
using TrTileSum = jt::TileSum;
using TrTileIn = jt::TileIn;
using TrCounts = jt::TileCounts;
using TrIdOpen = jt::TileOpen;          // ref: the blob
using TrNodeOpen = jt::TileOpenRanked;  // rank_a: id opens, rank_b: ']' at depth 4 before it
using TrClose = jt::TileClose;          // rank: id opens (c4) / node opens (c2) before it
constexpr uint32_t kTrNodeOk = 1u, kTrNodeFile = 2u, kTrNodeDir = 4u, kTrNodeSubtree = 8u;
// for the node records of rcdc_tree_nodes: "content" is an array, the raw
// name holds a backslash, and the type as its index in NODE_TYPES
constexpr uint32_t kTrNodeContent = 16u, kTrNodeNameEsc = 32u, kTrNodeTypeShift = 8u;
struct TrNodeTmp {
    uint32_t subtree[8];
    uint32_t flags;     // kTrNode*
    uint32_t blob;
    uint32_t id0, nids; // its content: id opens [id0, id0 + nids)
    uint64_t name_pos;  // the first byte after the name's opening quote
    uint32_t name_len;  // raw bytes up to its closing quote
    uint32_t pad;
};

struct TrArgs {
    const uint8_t *text;
    uint64_t text_len;
    const rcdc_trparse_ref *refs;   // device copy
    const uint32_t *tile_first;     // n_blobs + 1
    uint32_t n_blobs, n_tiles;
    uint32_t gn;                    // the grammar is G_N (rcdc_tree_nodes): a dir may lack its subtree
    // scratch
    TrTileSum *sums;
    TrTileIn *ins;
    uint8_t *esc;                   // per tile: its first byte is escaped
    TrCounts *counts;               // n_tiles + 1: the last one holds the totals
    TrNodeOpen *node_open;
    TrIdOpen *id_open;
    TrClose *c4, *c2;
    TrCounts total;
    uint8_t *tmp_ids;               // 32 B per id open
    TrNodeTmp *tmp_nodes;
    uint32_t *blob_ok;              // the blob lane's verdict, then the blob's
    uint32_t *blob_bad;             // set by any lane that fails
    void *adds;                     // four uint32 per node open, + 1: the numbering's scan
    void *add_sums;                 // four uint32 per kTrScan node opens, + 1
    // outputs (device)
    uint8_t *data_ids, *tree_ids, *tree_is_dir;
    uint64_t cap_data_ids, cap_tree_ids;
    rcdc_trparse_blob *blobs;
    // rcdc_tree_nodes only (null otherwise): the node records, and per blob
    // where its records start
    rcdc_trnode *nodes;
    uint64_t cap_nodes;
    uint64_t *node_start;
};

// the structural pass up to the totals in counts[n_tiles]
hipError_t launch_tr_structure(const TrArgs &a, hipStream_t st);
// the structural pass's emit, the strict lanes, the numbering
hipError_t launch_tr_parse(const TrArgs &a, hipStream_t st);

}  // namespace rcdc
