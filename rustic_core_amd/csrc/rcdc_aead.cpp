// rcdc_aead.cpp -- host half of blob encryption (crypto/aespoly1305.rs:88-135
// over HBM), pack building and device range copies: rcdc_aead_seal / open,
// rcdc_pack_build*, rcdc_copy_ranges.  Their state is the context's AeadState
// (rcdc_ctx.h); what a call uploads is planned in rcdc_family_plans.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "rcdc_ctx.h"
#include "rcdc_family_plans.h"
#include "rcdc_launch.h"

using namespace rcdc;
using namespace rcdc::plans;

namespace {

uint64_t r16(uint64_t x) { return (x + 15) & ~15ull; }

// The device key material of `key`, made and uploaded when the key changes.
rcdc_status aead_key_upload(AeadState &A, const uint8_t key[64]) {
    rcdc_status rs;
    if ((rs = A.d_key.ensure(1))) return rs;
    if (!A.key_set || memcmp(A.key, key, 64) != 0) {
        AeadKeyDev K;
        aead_key_material(key, &K);
        HIP_TRY(hipMemcpy(A.d_key, &K, sizeof K, hipMemcpyHostToDevice));
        memcpy(A.key, key, 64);
        A.key_set = true;
    }
    return RCDC_OK;
}

// Closes the batches' unit0 lists and sizes the scratch for them: the
// descriptors, and the page-locked buffer the call's uploads go through.
rcdc_status aead_size(AeadState &A, std::vector<AeadBatch *> &bt, const std::vector<uint8_t> *staging,
                      uint64_t *nblobs) {
    uint64_t nb = 0, nu = 0;
    for (AeadBatch *B : bt) {
        B->unit0.push_back((uint32_t)B->units.size());
        nb += B->blobs.size();
        nu += B->units.size();
    }
    rcdc_status rs;
    if ((rs = A.d_blobs.ensure(nb))) return rs;
    if ((rs = A.d_units.ensure(nu))) return rs;
    if ((rs = A.d_unit0.ensure(nb + bt.size()))) return rs;
    if ((rs = A.d_partials.ensure(nu * 5))) return rs;
    if ((rs = A.d_status.ensure(nb))) return rs;
    // the call's uploads go async on st from one page-locked buffer (free
    // again: the last call's work is done, every call ends synchronised).
    // Synchronous copies from pageable memory queued behind other streams'
    // multi-GiB copies on the DMA engine (the ingest engine's batches) and
    // stalled the calling thread for up to a whole copy.
    uint64_t up = staging ? r16(staging->size()) : 0;
    for (AeadBatch *B : bt)
        up += r16(B->blobs.size() * sizeof(AeadBlob)) + r16(B->unit0.size() * 4) +
              r16(B->units.size() * sizeof(AeadUnit));
    *nblobs = nb;
    return A.h_up.ensure(up, up + up / 2 + 4096);
}

// Launch the batches (each its own input base) on one context scratch.
// `staging` (optional) is copied to the scratch input buffer first and a
// batch whose `in` is nullptr reads from it.  open: status per blob of the
// batches in order (synchronous).  Calls on one context take turns.
rcdc_status aead_launch(rcdc_ctx *ctx, bool open, const uint8_t key[64], std::vector<AeadBatch *> bt,
                        uint8_t *out, hipStream_t st, const std::vector<uint8_t> *staging,
                        std::vector<uint32_t> *status) {
    AeadState &A = ctx->aead;
    std::lock_guard<std::mutex> lk(A.mu);
    DeviceGuard g(ctx->device);
    // (the last call's work is done: every call ends synchronised)
    if (!A.done) HIP_TRY(hipEventCreateWithFlags(&A.done, hipEventDisableTiming));
    rcdc_status rs;
    uint64_t nb = 0;
    if ((rs = aead_key_upload(A, key))) return rs;
    if ((rs = aead_size(A, bt, staging, &nb))) return rs;
    uint64_t hp = 0;
    auto upload = [&](void *dst, const void *src, uint64_t n) -> hipError_t {
        if (!n) return hipSuccess;
        memcpy(A.h_up.get() + hp, src, n);
        const hipError_t e = hipMemcpyAsync(dst, A.h_up.get() + hp, n, hipMemcpyHostToDevice, st);
        hp += r16(n);
        return e;
    };
    if (staging && !staging->empty()) {
        if ((rs = A.d_stage.ensure(staging->size() + 16)))
            return rs;
        HIP_TRY(upload(A.d_stage, staging->data(), staging->size()));
    }
    uint64_t ob = 0, ou = 0, o0 = 0;
    for (AeadBatch *Bp : bt) {
        AeadBatch &B = *Bp;
        const uint32_t m = (uint32_t)B.blobs.size(), u = (uint32_t)B.units.size();
        if (m) {
            HIP_TRY(upload(A.d_blobs + ob, B.blobs.data(), m * sizeof(AeadBlob)));
            HIP_TRY(upload(A.d_unit0 + o0, B.unit0.data(), (m + 1) * 4));
        }
        if (u) HIP_TRY(upload(A.d_units + ou, B.units.data(), u * sizeof(AeadUnit)));
        const uint8_t *in = B.in ? B.in : A.d_stage;
        HIP_TRY(launch_aead(open, in, out, A.d_blobs + ob, m, A.d_units + ou, u, A.d_unit0 + o0,
                            A.d_key, A.d_partials + ou * 5, A.d_status + ob,
                            (uint32_t)std::max(ctx->num_cus, 1), st));
        ob += m;
        ou += u;
        o0 += m + 1;
    }
    // The call returns once its work is done: the context's scratch is then
    // free for the next call with no event kept across calls.  (An event
    // recorded on the caller's stream and synchronised in the next call
    // failed once that stream had been destroyed in between, r5g; one
    // recorded on the context's stream waited behind whatever long kernel
    // shared that stream's hardware queue, r5l.)
    HIP_TRY(hipEventRecord(A.done, st));
    HIP_TRY(poll_event(A.done));
    if (open && status) {
        HIP_TRY(poll_event(A.done));
        status->assign(nb, 0);
        if (nb) {  // on st (see plan_finish: not the legacy default stream)
            HIP_TRY(hipMemcpyAsync(status->data(), A.d_status, nb * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(poll_stream(st));
        }
    }
    return RCDC_OK;
}

rcdc_status aead_run(rcdc_ctx *ctx, bool open, const uint8_t key[64], const void *d_in,
                     const rcdc_aead_ref *refs, uint32_t n, void *d_out, uint32_t *status,
                     void *hip_stream) {
    if (!valid_ctx(ctx) || !key || (n && (!refs || !d_in || !d_out)) || (open && n && !status))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    AeadBatch bt;
    bt.in = (const uint8_t *)d_in;
    std::vector<uint32_t> which;  // device blob -> caller index
    char msg[kMsg];
    rcdc_status rs;
    for (uint32_t i = 0; i < n; i++) {
        const rcdc_aead_ref &r = refs[i];
        if (open && r.len < 32) {
            // no room for nonce + tag: aespoly1305.rs:89-94 (< 16 bytes) and
            // the AEAD's own length check (16..31) both fail before any MAC
            status[i] = r.len < 16 ? 2u : 1u;
            continue;
        }
        AeadBlob b{};
        b.in_off = r.in_off;
        b.len = open ? r.len - 32 : r.len;
        b.out_off = r.out_off;
        memcpy(b.nonce, r.nonce, 16);  // little-endian words of the nonce bytes
        if ((rs = aead_add(bt, b, i, msg))) return fail(rs, "%s", msg);
        which.push_back(i);
    }
    std::vector<uint32_t> ds;
    hipStream_t st;
    {
        DeviceGuard g(ctx->device);
        if ((rs = null_enter(ctx, hip_stream, &st))) return rs;
        if ((rs = aead_launch(ctx, open, key, {&bt}, (uint8_t *)d_out, st, nullptr,
                              open ? &ds : nullptr)))
            return rs;
        if ((rs = null_leave(ctx, hip_stream, st))) return rs;
    }
    if (open)
        for (size_t j = 0; j < which.size(); j++) status[which[j]] = ds[j];
    return RCDC_OK;
}

static_assert(sizeof(rcdc_pack_blob) == 72, "rcdc_pack_blob is 72 B");
static_assert(sizeof(rcdc_pack) == 48, "rcdc_pack is 48 B");

// Device range copies (push_copy's units) into d_out on st.  The unit list
// lives in the context until the copy has run: calls take turns under the
// AEAD lock.
rcdc_status copy_units_run(rcdc_ctx *ctx, const std::vector<uint64_t> &copies, void *d_out,
                           hipStream_t st) {
    if (copies.empty()) return RCDC_OK;
    AeadState &A = ctx->aead;
    std::lock_guard<std::mutex> lk(A.mu);
    const uint64_t nu = copies.size() / 4;
    rcdc_status rs;
    if ((rs = A.d_copy_units.ensure(copies.size()))) return rs;
    HIP_TRY(hipMemcpyAsync(A.d_copy_units, copies.data(), copies.size() * 8,
                           hipMemcpyHostToDevice, st));
    HIP_TRY(launch_copy_ranges((uint8_t *)d_out, A.d_copy_units, (uint32_t)nu,
                               (uint32_t)std::max(ctx->num_cus, 1), st));
    // the host vector dies with the caller's call
    HIP_TRY(poll_stream(st));
    return RCDC_OK;
}

// Plan (pack_plan), then the raw blobs' copies and the sealing of blobs and
// headers on one stream.
rcdc_status pack_build(rcdc_ctx *ctx, const uint8_t key[64], const void *d_in,
                       const rcdc_pack_blob *blobs, uint32_t nblobs, rcdc_pack *packs,
                       uint32_t npacks, void *d_out, uint64_t out_len, uint32_t *blob_offsets,
                       void *hip_stream, bool raw, const void *const *srcs = nullptr,
                       uint32_t n_src = 0) {
    PackPlan pp;
    char msg[kMsg];
    rcdc_status rs;
    if ((rs = pack_plan(valid_ctx(ctx) && key, d_in, blobs, nblobs, packs, npacks, d_out, out_len,
                        blob_offsets, raw, srcs, n_src, pp, msg)))
        return fail(rs, "%s", msg);
    DeviceGuard g(ctx->device);
    hipStream_t st;
    if ((rs = null_enter(ctx, hip_stream, &st))) return rs;
    if ((rs = copy_units_run(ctx, pp.copies, d_out, st))) return rs;
    if ((rs = aead_launch(ctx, false, key, {&pp.data, &pp.headers}, (uint8_t *)d_out, st, &pp.hdr,
                          nullptr)))
        return rs;
    return null_leave(ctx, hip_stream, st);
}

}  // namespace

extern "C" {

rcdc_status rcdc_aead_seal(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                           const rcdc_aead_ref *refs, uint32_t n, void *d_out, void *hip_stream) {
    return aead_run(ctx, false, key, d_in, refs, n, d_out, nullptr, hip_stream);
}

rcdc_status rcdc_aead_open(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                           const rcdc_aead_ref *refs, uint32_t n, void *d_out, uint32_t *status,
                           void *hip_stream) {
    return aead_run(ctx, true, key, d_in, refs, n, d_out, status, hip_stream);
}

rcdc_status rcdc_pack_build(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                            const rcdc_pack_blob *blobs, uint32_t nblobs, rcdc_pack *packs,
                            uint32_t npacks, void *d_out, uint64_t out_len,
                            uint32_t *blob_offsets, void *hip_stream) {
    return pack_build(ctx, key, d_in, blobs, nblobs, packs, npacks, d_out, out_len, blob_offsets,
                      hip_stream, false);
}

rcdc_status rcdc_pack_build_raw(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                                const rcdc_pack_blob *blobs, uint32_t nblobs, rcdc_pack *packs,
                                uint32_t npacks, void *d_out, uint64_t out_len,
                                uint32_t *blob_offsets, void *hip_stream) {
    return pack_build(ctx, key, d_in, blobs, nblobs, packs, npacks, d_out, out_len, blob_offsets,
                      hip_stream, true);
}

rcdc_status rcdc_pack_build_raw_multi(rcdc_ctx *ctx, const uint8_t *key,
                                      const void *const *d_ins, uint32_t n_ins,
                                      const rcdc_pack_blob *blobs, uint32_t nblobs,
                                      rcdc_pack *packs, uint32_t npacks, void *d_out,
                                      uint64_t out_len, uint32_t *blob_offsets, void *hip_stream) {
    if (n_ins == 0) return fail(RCDC_ERR_INVALID_INPUT, "no input buffers");
    return pack_build(ctx, key, nullptr, blobs, nblobs, packs, npacks, d_out, out_len,
                      blob_offsets, hip_stream, true, d_ins, n_ins);
}

rcdc_status rcdc_copy_ranges(rcdc_ctx *ctx, const void *const *d_ins, uint32_t n_ins,
                             const rcdc_copy_ref *refs, uint32_t n, void *d_out,
                             void *hip_stream) {
    if (!valid_ctx(ctx) || (n && (!refs || !d_out || !d_ins || !n_ins)))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    std::vector<uint64_t> copies;
    copies.reserve(4 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        const rcdc_copy_ref &c = refs[i];
        if (c.src >= n_ins || !d_ins[c.src])
            return fail(RCDC_ERR_INVALID_INPUT, "copy %u: source %u of %u", i, c.src, n_ins);
        push_copy(copies, d_ins[c.src], c.in_off, c.out_off, c.len);
    }
    DeviceGuard g(ctx->device);
    hipStream_t st;
    rcdc_status rs;
    if ((rs = null_enter(ctx, hip_stream, &st))) return rs;
    if ((rs = copy_units_run(ctx, copies, d_out, st))) return rs;
    return null_leave(ctx, hip_stream, st);
}

}  // extern "C"
