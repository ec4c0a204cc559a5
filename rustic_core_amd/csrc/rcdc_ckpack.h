// rcdc_check_packs: what the host half (rcdc_ckpack.cpp) and the kernels
// (rcdc_ckpack.hip) share.  Included by those two units and rcdc_ctx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"

namespace rcdc {

constexpr uint32_t kCkBlock = 256;  // threads per pack: 4 waves
constexpr uint32_t kCkSortMax = RCDC_CKPACK_SORT_MAX;
constexpr uint32_t kCkNeedsSort = 2;  // CkPack::status between the judge and the sort pass
static_assert((kCkSortMax & (kCkSortMax - 1)) == 0, "the bitonic network sorts a power of two");
static_assert(kCkSortMax * 16u + 1024u <= 160u * 1024u, "the sort's keys must fit the CU's LDS");

// the entry arrays as the caller gave them
struct CkEntries {
    const uint8_t *ids, *off, *len, *ulen, *types;
    uint64_t id_stride, off_stride, len_stride, ulen_stride;
    uint32_t loc_records;  // off/len/ulen are rcdc_dindex_loc records on a 16-byte boundary
    uint32_t id_rows;      // ids have stride 32 on a 16-byte boundary
};

struct CkArgs {
    CkEntries e;
    const rcdc_prune_range *ranges;  // device copy
    const uint32_t *prefix;          // entries of the packs before p: its rows in order_tmp
    const rcdc_ckpack_hdr *hdrs;     // device copy or null
    const uint8_t *hdr_ids[2];
    const rcdc_dindex_loc *hdr_locs[2];
    uint32_t n_packs;
    // scratch
    uint32_t *order_tmp;      // per pack that was sorted: the entry (pack-local) at each position
    uint64_t *totals;         // [0] findings, [1] packs HOST, [2] packs sorted here
    uint32_t *list;           // the packs the sort pass, then the emit pass, has work for
    uint32_t *list_n;         // [0] of the sort pass, [1] of the emit pass
    // outputs (device)
    rcdc_ckpack_pack *packs;  // copied to the host at the end
    rcdc_ckpack_finding *findings;
    uint64_t cap_findings;
    uint32_t *order;          // or null
};

// every kernel of the call, in order
hipError_t launch_ck_packs(const CkArgs &a, hipStream_t st);

}  // namespace rcdc
