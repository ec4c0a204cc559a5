// rcdc_place.cpp -- host half of rcdc_place_blobs: decoded blobs to their
// file positions (restore.rs:630-668).  Its state is the context's PlaceState
// (rcdc_ctx.h); validation and the tile list are in rcdc_family_plans.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "rcdc_ctx.h"
#include "rcdc_family_plans.h"

using namespace rcdc;
using namespace rcdc::plans;

static_assert(sizeof(rcdc_place_blob) == 32, "rcdc_place_blob is 32 B");
static_assert(sizeof(rcdc_place_dest) == 16, "rcdc_place_dest is 16 B");

namespace {

// Tiles a call keeps at once, in page-locked memory and on the device (32 MiB
// of descriptors, 64 GiB of source).  A call with more runs in rounds: the
// stream is drained and the buffers are filled again.  RCDC_PLACE_TILES:
// another cap (the tests' rounds).
uint64_t place_tile_cap() {
    uint64_t cap = 1u << 20;
    if (const char *e = getenv("RCDC_PLACE_TILES")) cap = (uint64_t)atoll(e);
    return std::min<uint64_t>(std::max<uint64_t>(cap, 1), 1u << 20);
}

rcdc_status place_args(rcdc_ctx *ctx, const void *const *d_ins, const uint64_t *in_lens,
                       uint32_t n_ins, const rcdc_place_blob *blobs, uint32_t nblobs,
                       const rcdc_place_dest *dests, uint32_t ndests_total, void *const *d_outs,
                       const uint64_t *out_lens, uint32_t n_outs, uint32_t flags) {
    if (!valid_ctx(ctx)) return fail(RCDC_ERR_INVALID_INPUT, "ctx is NULL");
    if (flags & ~RCDC_PLACE_SKIP_ZERO)
        return fail(RCDC_ERR_INVALID_INPUT, "flags: unknown bits 0x%x", flags & ~RCDC_PLACE_SKIP_ZERO);
    if (nblobs && !blobs) return fail(RCDC_ERR_INVALID_INPUT, "blobs is NULL with nblobs %u", nblobs);
    if (ndests_total && !dests)
        return fail(RCDC_ERR_INVALID_INPUT, "dests is NULL with ndests_total %u", ndests_total);
    if (n_ins && (!d_ins || !in_lens))
        return fail(RCDC_ERR_INVALID_INPUT, "%s is NULL with n_ins %u", d_ins ? "in_lens" : "d_ins",
                    n_ins);
    if (n_outs && (!d_outs || !out_lens))
        return fail(RCDC_ERR_INVALID_INPUT, "%s is NULL with n_outs %u",
                    d_outs ? "out_lens" : "d_outs", n_outs);
    return RCDC_OK;
}

// One call's view of its inputs, its buffers (R tiles) and its stream.
struct PlaceCall {
    rcdc_ctx *ctx;
    const void *const *d_ins;
    const rcdc_place_blob *blobs;
    uint32_t nblobs;
    uint64_t R;
    const uint64_t *daddr;  // page-locked, as are the tiles
    PlaceTile *tiles;
    uint32_t cus;
    hipStream_t st;
    bool whole = false;    // the device holds the tile list of the whole call,
    uint64_t whole_n = 0;  // this many tiles
};

// Uploads and launches the window being built.
rcdc_status place_flush(PlaceCall &C, PlaceWindow &W, bool write, bool zero_test, bool skip_zero) {
    PlaceState &P = C.ctx->place;
    if (W.pos == W.w0) return RCDC_OK;
    // no window of a round overwrites another, and the round before
    // has run: the upload need not wait for the kernels in flight
    const bool side = W.win < sizeof P.ev / sizeof P.ev[0];
    HIP_TRY(hipMemcpyAsync(P.d_tiles + W.w0, C.tiles + W.w0, (W.pos - W.w0) * sizeof(PlaceTile),
                           hipMemcpyHostToDevice, side ? P.up : C.st));
    if (side) {
        hipEvent_t &ev = P.ev[W.win];
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, P.up));
        HIP_TRY(hipStreamWaitEvent(C.st, ev, 0));
    }
    HIP_TRY(launch_place(P.d_tiles + W.w0, (uint32_t)(W.pos - W.w0), P.d_dests, P.d_nz, write,
                         zero_test, skip_zero, C.cus, C.st));
    W.sent();
    return RCDC_OK;
}

// One pass over all tiles, window by window.
rcdc_status place_pass(PlaceCall &C, bool write, bool zero_test, bool skip_zero) {
    PlaceWindow W;
    PlaceCursor cur;
    for (;;) {
        cur = place_fill(C.d_ins, C.blobs, C.nblobs, C.daddr, zero_test, C.tiles, &W.pos,
                         W.limit(C.R), cur);
        if (cur.blob == C.nblobs) break;
        if (rcdc_status fs = place_flush(C, W, write, zero_test, skip_zero)) return fs;
        if (W.pos == C.R) {
            // the buffers are full: a new round once this one has run
            HIP_TRY(poll_stream(C.st));
            W.new_round();
        }
    }
    C.whole = W.rounds == 0 && zero_test;  // (a pass without the zero test leaves blobs out)
    C.whole_n = W.pos;
    return place_flush(C, W, write, zero_test, skip_zero);
}

// Sizes the device buffers, uploads the destination addresses, clears the
// non-zero words, and makes the upload stream on first use.
rcdc_status place_prepare(PlaceCall &C, uint32_t ndests_total, bool want_zero) {
    PlaceState &P = C.ctx->place;
    rcdc_status rs;
    if ((rs = P.d_tiles.ensure(C.R))) return rs;
    if ((rs = P.d_dests.ensure(std::max<uint64_t>(ndests_total, 1))))
        return rs;
    if (ndests_total)
        HIP_TRY(hipMemcpyAsync(P.d_dests, C.daddr, (size_t)ndests_total * 8, hipMemcpyHostToDevice, C.st));
    if (want_zero) {
        if ((rs = P.d_nz.ensure(C.nblobs))) return rs;
        HIP_TRY(hipMemsetAsync(P.d_nz, 0, (size_t)C.nblobs * 4, C.st));
    }
    if (!P.up) HIP_TRY(hipStreamCreateWithFlags(&P.up, hipStreamNonBlocking));
    return RCDC_OK;
}

}  // namespace

extern "C" {

// Everything is validated before the first launch; then the tile list
// (rcdc_place.h) is built blob by blob in page-locked memory and launched in
// windows that grow from 4096 tiles, doubling: the first launch goes out
// early, later ones are few, and the host builds window k + 1 while window k
// runs.
rcdc_status rcdc_place_blobs(rcdc_ctx *ctx, const void *const *d_ins, const uint64_t *in_lens,
                             uint32_t n_ins, const rcdc_place_blob *blobs, uint32_t nblobs,
                             const rcdc_place_dest *dests, uint32_t ndests_total,
                             void *const *d_outs, const uint64_t *out_lens, uint32_t n_outs,
                             uint32_t flags, uint8_t *zero, void *hip_stream) {
    rcdc_status rs;
    if ((rs = place_args(ctx, d_ins, in_lens, n_ins, blobs, nblobs, dests, ndests_total, d_outs,
                         out_lens, n_outs, flags)))
        return rs;
    if (!nblobs) return RCDC_OK;

    PlaceState &P = ctx->place;
    std::lock_guard<std::mutex> lk(P.mu);
    DeviceGuard g(ctx->device);
    // page-locked: every destination's device address, the non-zero words
    // read back, the tiles
    uint64_t ntiles = 0;
    for (uint32_t i = 0; i < nblobs; i++) ntiles += (blobs[i].len >> 16) + 1;  // an upper bound
    const uint64_t R = std::min<uint64_t>(ntiles, place_tile_cap());
    const uint64_t o_nz = ((uint64_t)ndests_total * 8 + 15) / 16 * 16;
    const uint64_t o_tiles = (o_nz + (uint64_t)nblobs * 4 + 31) / 32 * 32;
    const uint64_t need = o_tiles + R * sizeof(PlaceTile);
    if ((rs = P.h_buf.ensure(need, need + need / 4 + 4096))) return rs;
    uint64_t *daddr = reinterpret_cast<uint64_t *>(P.h_buf.get());
    uint32_t *h_nz = reinterpret_cast<uint32_t *>(P.h_buf.get() + o_nz);
    char msg[kMsg];
    if ((rs = place_validate(d_ins, in_lens, n_ins, blobs, nblobs, dests, ndests_total, d_outs,
                             out_lens, n_outs, daddr, msg)))
        return fail(rs, "%s", msg);

    const bool skip = (flags & RCDC_PLACE_SKIP_ZERO) != 0, want_zero = skip || zero;
    PlaceCall C{ctx, d_ins, blobs, nblobs, R, daddr,
                reinterpret_cast<PlaceTile *>(P.h_buf.get() + o_tiles),
                (uint32_t)std::max(ctx->num_cus, 1), nullptr};
    if ((rs = null_enter(ctx, hip_stream, &C.st))) return rs;
    hipStream_t st = C.st;
    if ((rs = place_prepare(C, ndests_total, want_zero))) return rs;
    if (skip) {
        // every tile of a blob has been tested before any of it is written
        if ((rs = place_pass(C, false, true, false))) return rs;
        if (C.whole) {
            // the same list again: tiles of blobs without a destination fall out in the kernel
            HIP_TRY(launch_place(P.d_tiles, (uint32_t)C.whole_n, P.d_dests, P.d_nz, true, false, true,
                                 C.cus, st));
        } else {
            HIP_TRY(poll_stream(st));  // the first pass's uploads have left the host buffer
            if ((rs = place_pass(C, true, false, true))) return rs;
        }
    } else {
        if ((rs = place_pass(C, true, want_zero, false))) return rs;
    }
    if (zero)
        HIP_TRY(hipMemcpyAsync(h_nz, P.d_nz, (size_t)nblobs * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(poll_stream(st));
    if (zero)
        for (uint32_t i = 0; i < nblobs; i++) zero[i] = h_nz[i] ? 0 : 1;
    return null_leave(ctx, hip_stream, st);
}

}  // extern "C"
