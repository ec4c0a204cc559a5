// rcdc_pack_header_parse: what the host half (rcdc_pkhdr.cpp) and the kernels
// (rcdc_pkhdr.hip) share.  Included by those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"

namespace rcdc {

constexpr uint32_t kPhTile = RCDC_PKHDR_TILE;  // bytes per tile: one wave
constexpr uint32_t kPhPhases = 41;             // distances to the next entry start: 0..40
constexpr uint32_t kPhHalo = 48;               // staged behind a tile: 40 bytes of an entry, to 16
constexpr uint32_t kPhBlock = 256;             // 4 tiles per workgroup
constexpr uint32_t kPhScan = 1024;             // headers per workgroup of the numbering scan
// a tile starts at most ceil(kPhTile / 37) entries: one lane each in pass 2
static_assert((kPhTile + 36) / 37 <= 64, "a tile's entries must fit one wave");
static_assert(kPhTile % 16 == 0 && kPhTile <= (1u << 11),
"PhWalk packs a tile position in 11 bits");

// A tile as a function of the state at its first byte, for one value of that
// state (the phase: the distance from the tile's first byte to the first
// entry start at or after it).
struct PhWalk {
    uint64_t sum;     // of the lengths of the entries started
    uint32_t packed;  // exit phase [0,6) | entries started [6,12) | tree entries [12,18) |
                      // error [18,20) (RCDC_PKHDR_BAD_TYPE / _CUT_SHORT) | its position [20,31)
    uint32_t pad;
};
// The state at a tile's first byte, on the header's true chain.
struct PhTileIn {
    uint32_t phase;
    uint32_t entry;   // entries of the header before the tile
    uint64_t offset;  // sum of their lengths
};
struct PhHeaderTmp {
    uint64_t sum;       // of all lengths
    uint64_t err_pos;
    uint32_t status, type, count, tree, err_entry, pad;
};

struct PhArgs {
    const uint8_t *plain;
    uint64_t plain_len;
    const rcdc_pkhdr_ref *refs;  // device copy
    const uint32_t *tile_first;  // n_headers + 1
    uint32_t n_headers, n_tiles;
    // scratch
    PhWalk *walks;               // n_tiles x kPhPhases
    uint8_t *exits;              // n_tiles x kPhPhases: the walks' exit phases on their own
    PhTileIn *ins;               // n_tiles
    PhHeaderTmp *tmp;            // n_headers
    void *adds;                  // four uint32 per header, + 1: packs[2], entries[2] before it
    void *add_sums;              // the same per workgroup of the scan, + 1
    // outputs (device)
    uint8_t *ids[2];
    rcdc_dindex_loc *locs[2];
    uint64_t cap_entries;
    uint32_t pack_base[2];
    rcdc_pkhdr_header *headers;
};

// every kernel of the call, in order
hipError_t launch_ph_parse(const PhArgs &a, hipStream_t st);

}  // namespace rcdc
