// rcdc_ctx.h -- the context, and what the units that work on it share:
// rcdc_runtime.cpp (chunking, lanes, streams; it defines the helpers below)
// and one unit per kernel family (rcdc_aead.cpp, rcdc_zstd_host.cpp,
// rcdc_place.cpp, rcdc_ckpack.cpp).  Each family keeps its lock, scratch, events and
// page-locked memory in one member struct, which frees what it owns; the
// other units (ingest, dindex, ixparse, prune) see the context only through
// the narrow exports of rcdc_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <mutex>
#include <vector>

#include "../../include/rcdc.h"
#include "rcdc_host.h"
#include "rcdc_internal.h"
#include "rcdc_place.h"

struct Lane;  // rcdc_runtime.cpp

namespace rcdc {

// blob encryption and pack building (rcdc_aead.cpp): calls on one context
// take turns, and so do the range copies (rcdc_copy_ranges, raw packs), whose
// unit list lives here until the copy has run
struct AeadState {
    std::mutex mu;
    uint8_t key[64] = {0};  // the key d_key was made from
    bool key_set = false;
    DevBuf<AeadKeyDev> d_key;
    DevBuf<AeadBlob> d_blobs;
    DevBuf<AeadUnit> d_units;
    DevBuf<uint32_t> d_unit0, d_partials, d_status;
    DevBuf<uint8_t> d_stage;  // pack headers
    PinnedBuf h_up;           // page-locked source of a call's uploads
    hipEvent_t done = nullptr;  // made by the first call
    DevBuf<uint64_t> d_copy_units;
    ~AeadState() {
        if (done) (void)hipEventDestroy(done);
    }
};

// blob compression (rcdc_zstd_compress): calls on one context take turns
struct ZstdEncState {
    std::mutex mu;
    DevBuf<ZstdTables> d_tabs;
    DevBuf<ZstdBlob> d_blobs;
    DevBuf<ZstdBlk> d_blks;
    DevBuf<uint2> d_res;
    DevBuf<uint64_t> d_bpos, d_lens, d_seq;
    DevBuf<uint32_t> d_queue;  // per window: blocks taken past the first grid
    DevBuf<uint8_t> d_slots;
    DevBuf<uint32_t> d_far;  // far candidates: tables + maps per block (levels >= 3)
};

// frame checks (rcdc_zstd_check): calls on one context take turns
struct ZckState {
    std::mutex mu;
    DevBuf<uint64_t> d_refs;
    DevBuf<uint32_t> d_order, d_status;
    DevBuf<uint8_t> d_scratch;
    DevBuf<uint64_t> d_blk0;  // block-parallel pass: per-frame block slots
    DevBuf<uint8_t> d_blks;
};

// frame decompression (rcdc_zstd_decompress): calls on one context take turns
struct ZdxState {
    std::mutex mu;
    DevBuf<uint64_t> d_refs, d_lens;
    DevBuf<ZdxFrame> d_frm;
    DevBuf<ZdxPlace> d_place;
    DevBuf<uint32_t> d_order, d_status;
    DevBuf<uint8_t> d_ws;  // the workspace (ZdxLayout)
    uint64_t stats[8] = {0};  // the last call's counters (rcdc_zstd_decompress_stats)
};

// blobs placed into files (rcdc_place_blobs): calls on one context take turns
struct PlaceState {
    std::mutex mu;
    DevBuf<PlaceTile> d_tiles;
    DevBuf<uint64_t> d_dests;
    DevBuf<uint32_t> d_nz;
    PinnedBuf h_buf;  // page-locked: destination addresses, read-back, tiles
    // tile windows are uploaded on a stream of their own, so that window
    // k + 1 arrives while window k runs; one event per window of a round.
    // Both are made by the first call that needs them.
    hipStream_t up = nullptr;
    hipEvent_t ev[16] = {};
    ~PlaceState() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (up) (void)hipStreamDestroy(up);
    }
};

// check's index pass (rcdc_check_packs): calls on one context take turns
struct CkpackState {
    std::mutex mu;
    DevBuf<rcdc_prune_range> d_ranges;
    DevBuf<rcdc_ckpack_hdr> d_hdrs;
    DevBuf<rcdc_ckpack_pack> d_packs;
    DevBuf<uint32_t> d_prefix;
    DevBuf<uint32_t> d_order;  // of the packs sorted on the device
    DevBuf<uint32_t> d_list, d_list_n;  // the packs the sort and emit passes have work for
    DevBuf<uint64_t> d_totals;
};

}  // namespace rcdc

// Destroyed by rcdc_ctx_destroy with its device current and its stream idle:
// the members free what they own.
struct rcdc_ctx {
    int device = 0;
    uint64_t poly = 0, min = 0, avg = 0, max = 0;
    int deg = 0;
    int num_cus = 0;
    int variant = rcdc::kDefaultScanCode;  // scan-kernel configuration (RCDC_SCAN_VARIANT)
    hipStream_t stream = nullptr;
    uint64_t *d_tables = nullptr;
    // host-buffer path: a pool of lanes (RCDC_LANES, default 16)
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    std::vector<Lane *> lanes, free_lanes;
    uint32_t max_lanes = 16;
    // ordering of calls on the context's stream (hip_stream == 0) with the
    // legacy default stream (null_enter / null_leave)
    hipEvent_t ev_null_in = nullptr, ev_null_out = nullptr;
    // device tails of open streams (max + 256 bytes each): a pool, so opening
    // and closing streams never calls hipMalloc / hipFree (which synchronise
    // the device) once warm
    std::mutex tail_mu;
    std::vector<uint8_t *> tail_pool, tail_all;
    // one member per kernel family
    rcdc::AeadState aead;
    rcdc::ZstdEncState zenc;
    rcdc::ZckState zck;
    rcdc::ZdxState zdx;
    rcdc::PlaceState place;
    rcdc::CkpackState ckpack;
};

namespace rcdc {

// ---- defined in rcdc_runtime.cpp ---------------------------------------------
// sets the calling thread's rcdc_last_error text (printf-style), returns st
rcdc_status fail(rcdc_status st, const char *fmt, ...);
bool valid_ctx(const rcdc_ctx *c);
// hip_stream == 0 selects the context's own stream, ordered with the legacy
// default stream: after the work queued there before the call (null_enter)
// and before the work queued there after it (null_leave).
rcdc_status null_enter(rcdc_ctx *ctx, const void *hip_stream, hipStream_t *st);
rcdc_status null_leave(rcdc_ctx *ctx, const void *hip_stream, hipStream_t st);
// waits that poll (hipEventQuery + a 50 us sleep) instead of blocking in HIP
hipError_t poll_event(hipEvent_t ev);
hipError_t poll_stream(hipStream_t st);

}  // namespace rcdc
