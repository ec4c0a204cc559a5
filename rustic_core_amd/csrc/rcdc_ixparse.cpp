// rcdc_index_parse (include/rcdc.h): the host half -- argument checks, the
// tile table, scratch memory and the order of the launches.  The kernels are
// in rcdc_ixparse.hip.
//
// The call stops the stream twice: once after the structural pass, to size
// the record arrays from its four totals, and once at the end, to hand the
// per-file and per-pack results to the caller.  Scratch lives for one call.

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rcdc_host.h"
#include "rcdc_ixparse.h"

using namespace rcdc;

extern "C" {

void rcdc_index_parse_bound(uint64_t len, uint64_t *max_entries, uint64_t *max_packs) {
    // n blobs and their commas: 110 n - 1 bytes; n packs: 85 n - 1 (rcdc.h)
    if (max_entries) *max_entries = (len + 1) / 110;
    if (max_packs) *max_packs = (len + 1) / 85;
}

uint32_t rcdc_index_parse_tile(void) { return RCDC_IXPARSE_TILE; }

rcdc_status rcdc_index_parse(rcdc_ctx *ctx, const void *d_json, uint64_t json_len,
                             const rcdc_ixparse_ref *refs, uint32_t n_files,
                             const uint32_t pack_base[2], void *const d_ids[2],
                             rcdc_dindex_loc *const d_locs[2], uint64_t cap_entries,
                             rcdc_ixparse_file *files, rcdc_ixparse_pack *packs,
                             uint64_t cap_packs, rcdc_ixparse_result *result, void *hip_stream) {
    if (!ctx) return invalid("rcdc_index_parse: ctx is NULL");
    if (!result) return invalid("rcdc_index_parse: result is NULL");
    if (n_files && (!refs || !files || !pack_base || !d_ids || !d_locs))
        return invalid("rcdc_index_parse: null array");
    uint64_t need_entries = 0, need_packs = 0, n_tiles = 0;
    std::vector<uint32_t> tile_first;
    switch (tile_table(refs, n_files, json_len, d_json, kIxTile, tile_first, n_tiles,
                       [&](uint64_t len) {
        uint64_t e = 0, p = 0;
        rcdc_index_parse_bound(len, &e, &p);
        need_entries += e;
        need_packs += p;
        return need_entries < 0xFFFFFFFFull;
    })) {
    case TileTable::RefOutside: return invalid("rcdc_index_parse: a ref lies outside the arena");
    case TileTable::ArenaNull: return invalid("rcdc_index_parse: d_json is NULL");
    case TileTable::TooMany:
        return invalid("rcdc_index_parse: the batch may hold 2^32 - 1 entries or more");
    case TileTable::Ok: break;
    }
    if (cap_entries < need_entries || cap_packs < need_packs)
        return invalid("rcdc_index_parse: capacities below rcdc_index_parse_bound");
    if (need_packs && !packs) return invalid("rcdc_index_parse: packs is NULL");
    for (int t = 0; t < 2 && n_files; t++)
        if (((uintptr_t)d_ids[t] & 15u) || ((uintptr_t)d_locs[t] & 15u))
            return invalid("rcdc_index_parse: the entry arrays must be 16-byte aligned");
    *result = rcdc_ixparse_result{};
    if (n_files == 0) return RCDC_OK;

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    Scratch sc;
    IxArgs a = {};
    a.json = static_cast<const uint8_t *>(d_json);
    a.json_len = json_len;
    a.n_files = n_files;
    a.n_tiles = (uint32_t)n_tiles;
    rcdc_ixparse_ref *d_refs = nullptr;
    uint32_t *d_tile_first = nullptr;
    HIP_TRY(sc.get(&d_refs, n_files));
    HIP_TRY(sc.get(&d_tile_first, n_files + 1ull));
    HIP_TRY(sc.get(&a.sums, n_tiles));
    HIP_TRY(sc.get(&a.ins, n_tiles));
    HIP_TRY(sc.get(&a.counts, n_tiles + 1));
    HIP_TRY(hipMemcpyAsync(d_refs, refs, n_files * sizeof *refs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tile_first, tile_first.data(), (n_files + 1ull) * 4,
                          hipMemcpyHostToDevice, st));
    a.refs = d_refs;
    a.tile_first = d_tile_first;
    HIP_TRY(launch_ix_structure(a, st));
    HIP_TRY(hipMemcpyAsync(&a.total, a.counts + n_tiles, sizeof a.total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    HIP_TRY(sc.get(&a.blob_open, a.total.n[kIxBlob]));
    HIP_TRY(sc.get(&a.pack_open, a.total.n[kIxPack]));
    HIP_TRY(sc.get(&a.c4, a.total.n[kIxC4]));
    HIP_TRY(sc.get(&a.c2, a.total.n[kIxC2]));
    HIP_TRY(sc.get(&a.tmp_ids, (uint64_t)a.total.n[kIxBlob] * 32));
    HIP_TRY(sc.get(&a.tmp_blobs, a.total.n[kIxBlob]));
    HIP_TRY(sc.get(&a.tmp_packs, a.total.n[kIxPack]));
    HIP_TRY(sc.get(&a.tmp_files, n_files));
    HIP_TRY(sc.get(&a.file_bad, n_files));
    uint32_t *adds = nullptr;
    HIP_TRY(sc.get(&adds, ((uint64_t)a.total.n[kIxPack] + 1) * 4));
    a.adds = adds;
    HIP_TRY(sc.get(&a.files, n_files));
    HIP_TRY(sc.get(&a.packs, cap_packs));
    HIP_TRY(sc.get(&a.result, 4));
    HIP_TRY(hipMemsetAsync(a.file_bad, 0, n_files * 4ull, st));
    for (int t = 0; t < 2; t++) {
        a.ids[t] = static_cast<uint8_t *>(d_ids[t]);
        a.locs[t] = d_locs[t];
        a.pack_base[t] = pack_base[t];
    }
    a.cap_entries = cap_entries;
    a.cap_packs = cap_packs;
    HIP_TRY(launch_ix_parse(a, st));
    uint64_t tot[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, a.result, sizeof tot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(files, a.files, n_files * sizeof *files, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t n_packs = tot[0] + tot[1];
    if (n_packs > cap_packs || tot[2] > cap_entries || tot[3] > cap_entries)
        return set_error(RCDC_ERR_INTERNAL, "rcdc_index_parse: more output than the bound allows");
    if (n_packs) {
        HIP_TRY(hipMemcpyAsync(packs, a.packs, n_packs * sizeof *packs, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    result->packs[0] = tot[0];
    result->packs[1] = tot[1];
    result->entries[0] = tot[2];
    result->entries[1] = tot[3];
    for (uint32_t f = 0; f < n_files; f++)
        result->files_not_parsed += files[f].status != RCDC_IXPARSE_OK;
    return RCDC_OK;
}

}  // extern "C"
