// rcdc_index_parse: what the host half (rcdc_ixparse.cpp) and the kernels
// (rcdc_ixparse.hip) share.  Included by those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"
#include "rcdc_json_tiles.h"

namespace rcdc {

constexpr uint32_t kIxTile = RCDC_IXPARSE_TILE;  // bytes per tile: one wave
constexpr uint32_t kIxBlock = 256;               // 4 tiles per workgroup

// The structural pass's records (rcdc_json_tiles.h).  The event kinds, in
// the order of TileCounts::n: blob-object opens ('{' at depth 4), pack-object
// opens ('{' at depth 2), ']' at depth 4 (closes a "blobs" array) and ']' at
// depth 2 (closes an array of the root).
enum IxEvent : uint32_t { kIxBlob, kIxPack, kIxC4, kIxC2 };
struct IxGrammar {
    // ch is a byte that counts, outside a string; -1: no event
    RCDC_JT_FN static int event_of(uint8_t ch, int32_t depth) {
        if (ch == '{') return depth == 4 ? (int)kIxBlob : depth == 2 ? (int)kIxPack : -1;
        if (ch == ']') return depth == 4 ? (int)kIxC4 : depth == 2 ? (int)kIxC2 : -1;
        return -1;
    }
};
using IxTileSum = jt::TileSum;
using IxTileIn = jt::TileIn;
using IxCounts = jt::TileCounts;
using IxBlobOpen = jt::TileOpen;        // ref: the file
using IxPackOpen = jt::TileOpenRanked;  // rank_a: blob opens, rank_b: ']' at depth 4 before it
using IxClose = jt::TileClose;          // rank: blob opens (c4) / pack opens (c2) before it
struct IxBlobTmp {
    uint32_t offset, length, ulen, type;
};
struct IxPackTmp {
    uint32_t id[8];
    uint32_t size, has_size, nblobs, blob0, file, type, ok;
    // set by the numbering kernel
    uint32_t collected, number, entry0, out;
    uint32_t pad;
};
struct IxFileTmp {
    uint32_t ok, pack_a, pack_b, ndelete;
};

struct IxArgs {
    const uint8_t *json;
    uint64_t json_len;
    const rcdc_ixparse_ref *refs;   // device copy
    const uint32_t *tile_first;     // n_files + 1
    uint32_t n_files, n_tiles;
    // scratch
    IxTileSum *sums;
    IxTileIn *ins;
    IxCounts *counts;               // n_tiles + 1: the last one holds the totals
    IxBlobOpen *blob_open;
    IxPackOpen *pack_open;
    IxClose *c4, *c2;
    IxCounts total;
    uint8_t *tmp_ids;               // 32 B per blob open
    IxBlobTmp *tmp_blobs;
    IxPackTmp *tmp_packs;
    IxFileTmp *tmp_files;
    uint32_t *file_bad;
    void *adds;                     // four uint32 per pack open, + 1: the numbering's scan
    // outputs (device)
    uint8_t *ids[2];
    rcdc_dindex_loc *locs[2];
    uint64_t cap_entries, cap_packs;
    uint32_t pack_base[2];
    rcdc_ixparse_file *files;
    rcdc_ixparse_pack *packs;
    uint64_t *result;               // packs[2], entries[2]
};

// stage 1 up to the totals in counts[n_tiles]
hipError_t launch_ix_structure(const IxArgs &a, hipStream_t st);
// stage 1's emit, stages 2 to 4
hipError_t launch_ix_parse(const IxArgs &a, hipStream_t st);

}  // namespace rcdc
