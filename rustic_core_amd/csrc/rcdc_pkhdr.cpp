// rcdc_pack_header_parse (include/rcdc.h): the host half -- argument checks,
// the tile table, scratch memory and the launch.  The kernels are in
// rcdc_pkhdr.hip.
//
// Nothing is sized from a device count (every array follows from the refs),
// so the call stops the stream once, at the end, to hand the per-header
// records and the totals to the caller.  Scratch lives for one call.

#include <hip/hip_runtime.h>

#include <vector>

#include "rcdc_host.h"
#include "rcdc_pkhdr.h"

using namespace rcdc;

extern "C" {

uint64_t rcdc_pack_header_parse_bound(uint64_t len) { return len / 37u; }

uint32_t rcdc_pack_header_parse_tile(void) { return RCDC_PKHDR_TILE; }

rcdc_status rcdc_pack_header_parse(rcdc_ctx *ctx, const void *d_plain, uint64_t plain_len,
                                   const rcdc_pkhdr_ref *refs, uint32_t n_headers,
                                   const uint32_t pack_base[2], void *const d_ids[2],
                                   rcdc_dindex_loc *const d_locs[2], uint64_t cap_entries,
                                   rcdc_pkhdr_header *headers, rcdc_pkhdr_result *result,
                                   void *hip_stream) {
    if (!ctx) return invalid("rcdc_pack_header_parse: ctx is NULL");
    if (!result) return invalid("rcdc_pack_header_parse: result is NULL");
    if (n_headers && (!refs || !headers || !pack_base || !d_ids || !d_locs))
        return invalid("rcdc_pack_header_parse: null array");
    uint64_t need_entries = 0, n_tiles = 0;
    std::vector<uint32_t> tile_first;
    switch (tile_table(refs, n_headers, plain_len, d_plain, kPhTile, tile_first, n_tiles,
                       [&](uint64_t len) {
        need_entries += rcdc_pack_header_parse_bound(len);
        return need_entries < 0xFFFFFFFFull;
    })) {
    case TileTable::RefOutside:
        return invalid("rcdc_pack_header_parse: a ref lies outside the arena");
    case TileTable::ArenaNull: return invalid("rcdc_pack_header_parse: d_plain is NULL");
    case TileTable::TooMany:
        return invalid("rcdc_pack_header_parse: the batch may hold 2^32 - 1 entries or more");
    case TileTable::Ok: break;
    }
    if (cap_entries < need_entries)
        return invalid("rcdc_pack_header_parse: cap_entries below rcdc_pack_header_parse_bound");
    for (int t = 0; t < 2 && n_headers; t++)
        if (((uintptr_t)d_ids[t] & 15u) || ((uintptr_t)d_locs[t] & 15u))
            return invalid("rcdc_pack_header_parse: the entry arrays must be 16-byte aligned");
    *result = rcdc_pkhdr_result{};
    if (n_headers == 0) return RCDC_OK;

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch sc;
    PhArgs a = {};
    a.plain = static_cast<const uint8_t *>(d_plain);
    a.plain_len = plain_len;
    a.n_headers = n_headers;
    a.n_tiles = (uint32_t)n_tiles;
    rcdc_pkhdr_ref *d_refs = nullptr;
    uint32_t *d_tile_first = nullptr, *adds = nullptr, *add_sums = nullptr;
    HIP_TRY(sc.get(&d_refs, n_headers));
    HIP_TRY(sc.get(&d_tile_first, n_headers + 1ull));
    HIP_TRY(sc.get(&a.walks, n_tiles * kPhPhases));
    HIP_TRY(sc.get(&a.exits, n_tiles * kPhPhases));
    HIP_TRY(sc.get(&a.ins, n_tiles));
    HIP_TRY(sc.get(&a.tmp, n_headers));
    HIP_TRY(sc.get(&adds, (n_headers + 1ull) * 4));
    HIP_TRY(sc.get(&add_sums, ((uint64_t)n_headers / kPhScan + 2) * 4));
    HIP_TRY(sc.get(&a.headers, n_headers));
    HIP_TRY(hipMemcpyAsync(d_refs, refs, n_headers * sizeof *refs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tile_first, tile_first.data(), (n_headers + 1ull) * 4,
                          hipMemcpyHostToDevice, st));
    a.refs = d_refs;
    a.tile_first = d_tile_first;
    a.adds = adds;
    a.add_sums = add_sums;
    for (int t = 0; t < 2; t++) {
        a.ids[t] = static_cast<uint8_t *>(d_ids[t]);
        a.locs[t] = d_locs[t];
        a.pack_base[t] = pack_base[t];
    }
    a.cap_entries = cap_entries;
    HIP_TRY(launch_ph_parse(a, st));
    uint32_t tot[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, adds + (uint64_t)n_headers * 4, sizeof tot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(headers, a.headers, n_headers * sizeof *headers, hipMemcpyDeviceToHost,
                          st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[2] > cap_entries || tot[3] > cap_entries)
        return set_error(RCDC_ERR_INTERNAL,
                         "rcdc_pack_header_parse: more output than the bound allows");
    result->packs[0] = tot[0];
    result->packs[1] = tot[1];
    result->entries[0] = tot[2];
    result->entries[1] = tot[3];
    for (uint32_t h = 0; h < n_headers; h++)
        result->headers_not_parsed += headers[h].status != RCDC_PKHDR_OK;
    return RCDC_OK;
}

}  // extern "C"
