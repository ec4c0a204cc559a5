// rcdc_dindex: what the host half (rcdc_dindex.cpp) and the kernels
// (rcdc_dindex.hip) share.  Included by those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"

namespace rcdc {

// An empty slot.  A used slot is (entry << 32) | tag; entry 0xFFFFFFFF is
// never given out (rcdc_dindex_add refuses size + n >= 2^32 - 1).
constexpr uint64_t kDxEmpty = ~0ull;
constexpr uint32_t kDxBlock = 256;

// The table and the entries it points into.  nslots is a power of two and at
// least twice the entries that are or will be in it, so every probe ends at
// an empty slot.
struct DxTable {
    uint64_t *slots;   // nslots words
    uint32_t *counts;  // nslots: entries of the slot's id beyond the first
    uint64_t mask;     // nslots - 1
    const uint8_t *ids;            // 32 B per entry, 16-byte aligned
    const rcdc_dindex_loc *locs;   // 16 B per entry
};

// entries [first, first + n) -> pack = NO_PACK, the rest 0
hipError_t launch_dx_fill_locs(rcdc_dindex_loc *locs, uint64_t first, uint64_t n, hipStream_t st);
// insert entries [first, first + n) into t; *keys += the ids that were new
hipError_t launch_dx_insert(DxTable t, uint64_t first, uint64_t n, unsigned long long *keys,
                            hipStream_t st);
hipError_t launch_dx_lookup(DxTable t, const uint8_t *q, uint64_t n, rcdc_dindex_hit *hits,
                            hipStream_t st);
// scratch: a cleared table of >= 2 n slots whose "entries" are the batch's
// positions (ids = q).  Two kernels: candidates in, then first occurrences out.
hipError_t launch_dx_first_new(DxTable t, const uint8_t *q, uint64_t n, const uint8_t *select,
                               uint8_t *out, uint64_t *scratch, uint64_t smask, hipStream_t st);

}  // namespace rcdc
