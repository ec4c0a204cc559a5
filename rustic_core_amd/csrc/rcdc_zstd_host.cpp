// rcdc_zstd_host.cpp -- host half of the zstd families (RFC 8878): blob
// compression (rcdc_zstd_compress), the frame check (rcdc_zstd_check), frame
// decompression (rcdc_zstd_decompress) and the header walk on the host
// (rcdc_zstd_frame_info).  Their state is the context's ZstdEncState,
// ZckState and ZdxState (rcdc_ctx.h); windows, groups and work lists are
// planned in rcdc_family_plans.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "rcdc_ctx.h"
#include "rcdc_family_plans.h"
#include "rcdc_launch.h"

using namespace rcdc;
using namespace rcdc::plans;

namespace {

// ---- blob compression ----------------------------------------------------------

// FSE_buildCTable of a normalized distribution (the format's symbol spread:
// RFC 8878 4.1.1; zstd lib/compress/fse_compress.c): state table sorted by
// symbol, and per symbol {deltaFindState, deltaNbBits}.
void fse_build_ctable(const int16_t *norm, int nsym, int tlog, ZstdFseSym *tt, uint16_t *st) {
    const int size = 1 << tlog, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    std::vector<int> sym(size), cumul(nsym + 1);
    int high = size - 1;
    for (int u = 1; u <= nsym; u++) {
        if (norm[u - 1] == -1) {
            cumul[u] = cumul[u - 1] + 1;
            sym[high--] = u - 1;
        } else {
            cumul[u] = cumul[u - 1] + norm[u - 1];
        }
    }
    int pos = 0;
    for (int s = 0; s < nsym; s++)
        for (int k = 0; k < norm[s]; k++) {
            sym[pos] = s;
            pos = (pos + step) & mask;
            while (pos > high) pos = (pos + step) & mask;
        }
    for (int u = 0; u < size; u++) st[cumul[sym[u]]++] = (uint16_t)(size + u);
    int total = 0;
    for (int s = 0; s < nsym; s++) {
        const int c = norm[s];
        if (c == -1 || c == 1) {
            tt[s].nbits = ((uint32_t)tlog << 16) - (uint32_t)size;
            tt[s].find = total - 1;
            total++;
        } else if (c > 1) {
            const int mbo = tlog - (31 - __builtin_clz((uint32_t)(c - 1)));
            tt[s].nbits = ((uint32_t)mbo << 16) - ((uint32_t)c << mbo);
            tt[s].find = total - c;
            total += c;
        } else {
            tt[s].nbits = ((uint32_t)(tlog + 1) << 16) - (uint32_t)size;
            tt[s].find = 0;
        }
    }
}

// The predefined distributions and code tables (RFC 8878 3.1.1.3.2.1-2).
const ZstdTables &zstd_tables() {
    static ZstdTables T;
    static std::once_flag once;
    std::call_once(once, [] {
        static const int16_t ll_norm[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                            2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
        static const int16_t ml_norm[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                            1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                            1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
        static const int16_t of_norm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                            1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
        static const uint32_t ll_base[36] = {0,  1,  2,   3,   4,   5,   6,    7,    8,    9,
                                             10, 11, 12,  13,  14,  15,  16,   18,   20,   22,
                                             24, 28, 32,  40,  48,  64,  128,  256,  512,  1024,
                                             2048, 4096, 8192, 16384, 32768, 65536};
        static const uint8_t ll_bits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                            1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
        static const uint32_t ml_base[53] = {
            3,  4,  5,  6,  7,  8,  9,  10, 11,  12,  13,  14,   15,   16,   17,   18,   19, 20,
            21, 22, 23, 24, 25, 26, 27, 28, 29,  30,  31,  32,   33,   34,   35,   37,   39, 41,
            43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
        static const uint8_t ml_bits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                            0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1,
                                            2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
        memset(&T, 0, sizeof T);
        fse_build_ctable(ll_norm, 36, 6, T.ll, T.llst);
        fse_build_ctable(ml_norm, 53, 6, T.ml, T.mlst);
        fse_build_ctable(of_norm, 29, 5, T.of, T.ofst);
        for (uint32_t v = 0; v < 64; v++) {
            int c = 0;
            while (c + 1 < 36 && ll_base[c + 1] <= v) c++;
            T.llcode[v] = (uint8_t)c;
        }
        for (uint32_t v = 0; v < 128; v++) {
            int c = 0;
            while (c + 1 < 53 && ml_base[c + 1] - 3 <= v) c++;
            T.mlcode[v] = (uint8_t)c;
        }
        memcpy(T.llbits, ll_bits, sizeof ll_bits);
        memcpy(T.mlbits, ml_bits, sizeof ml_bits);
    });
    return T;
}

// Blocks per launch window: bounds the per-block scratch (32768 x 128 KiB);
// windows run back to back on the stream, reusing it.
constexpr uint64_t kZstdWindowBlocks = 32768;

// RCDC_ZSTD_WINDOW_BLOCKS (tests): a smaller window, so a modest batch runs
// the multi-window path (per-window queues, rebased indices, reused slots)
uint64_t zstd_window_blocks() {
    if (const char *e = getenv("RCDC_ZSTD_WINDOW_BLOCKS")) {
        const long long v = atoll(e);
        if (v > 0) return std::min<uint64_t>((uint64_t)v, kZstdWindowBlocks);
    }
    return kZstdWindowBlocks;
}

// What a compress call sizes its scratch by.
struct ZstdSizes {
    uint32_t grid;
    uint64_t nbl, nbo, maxw, farw, nwin;
    uint64_t seq_words() const { return (uint64_t)grid * kZstdMaxSeq + 8; }
    uint64_t queue_words() const { return nwin * 128; }
};

// The scratch the compress kernels are launched with: the context's buffers,
// or RCDC_ZSTD_GUARD's.
struct ZstdScratch {
    ZstdBlob *blobs;
    ZstdBlk *blks;
    ZstdTables *tabs;
    uint8_t *slots;
    uint64_t *seq, *bpos, *lens;
    uint2 *res;
    uint32_t *queue, *far;
};

rcdc_status zstd_enc_size(ZstdEncState &Z, const ZstdSizes &S, ZstdScratch *sc) {
    rcdc_status rs;
    if (!Z.d_tabs) {
        if ((rs = Z.d_tabs.ensure(1))) return rs;
        HIP_TRY(hipMemcpy(Z.d_tabs, &zstd_tables(), sizeof(ZstdTables), hipMemcpyHostToDevice));
    }
    // (+ 8 words: the last wave's 16-byte literal loads may pass its region by 20 bytes)
    if ((rs = Z.d_seq.ensure(S.seq_words())))
        return rs;
    if ((rs = Z.d_blobs.ensure(S.nbo))) return rs;
    if ((rs = Z.d_blks.ensure(S.nbl))) return rs;
    if ((rs = Z.d_res.ensure(S.nbl))) return rs;
    if ((rs = Z.d_bpos.ensure(S.nbl))) return rs;
    if ((rs = Z.d_lens.ensure(S.nbo))) return rs;
    if ((rs = Z.d_slots.ensure(S.maxw * kZstdSlot))) return rs;
    if (S.farw && (rs = Z.d_far.ensure(S.farw))) return rs;
    // the block kernel's queue: 8 counters 64 B apart per window
    if ((rs = Z.d_queue.ensure(S.queue_words()))) return rs;
    *sc = {Z.d_blobs, Z.d_blks, Z.d_tabs, Z.d_slots, Z.d_seq, Z.d_bpos,
           Z.d_lens,  Z.d_res,  Z.d_queue, S.farw ? Z.d_far.get() : nullptr};
    return RCDC_OK;
}

// RCDC_ZSTD_DBG & 32: the buffers, to place a fault
void zstd_dbg_buffers(const ZstdEncState &Z, const ZstdSizes &S, const void *d_in, const void *d_out,
                      int level) {
    auto rng = [](const char *nm, const void *p, uint64_t bytes) {
        fprintf(stderr, "rcdc zstd buf %-6s [%p, %p) %llu B\n", nm, p, (const void *)((const char *)p + bytes),
                (unsigned long long)bytes);
    };
    rng("seq", Z.d_seq, Z.d_seq.capacity() * 8);
    rng("slots", Z.d_slots, Z.d_slots.capacity());
    rng("far", Z.d_far, Z.d_far.capacity() * 4);
    rng("res", Z.d_res, Z.d_res.capacity() * 8);
    rng("bpos", Z.d_bpos, Z.d_bpos.capacity() * 8);
    rng("blobs", Z.d_blobs, Z.d_blobs.capacity() * sizeof(ZstdBlob));
    rng("blks", Z.d_blks, Z.d_blks.capacity() * sizeof(ZstdBlk));
    rng("tabs", Z.d_tabs, Z.d_tabs.capacity() * sizeof(ZstdTables));
    rng("queue", Z.d_queue, Z.d_queue.capacity() * 4);
    rng("in", d_in, 0);
    rng("out", d_out, 0);
    fprintf(stderr, "rcdc zstd grid %u nblk %llu maxw %llu level %d\n", S.grid, (unsigned long long)S.nbl,
            (unsigned long long)S.maxw, level);
}

// RCDC_ZSTD_GUARD=1 (debugging): every scratch buffer of a call is a fresh
// allocation with 16 MiB of 0xCD before and after it, checked after the
// call; a kernel that strays past one is reported, not faulted.
class ZstdGuard {
public:
    static bool on() {
        static const bool zguard = getenv("RCDC_ZSTD_GUARD") != nullptr;
        return zguard;
    }
    ~ZstdGuard() {
        for (const GBuf &gb : gbufs_) (void)hipFree(gb.base);
    }

    // Replaces every buffer of `sc` and fills the ones the host writes.
    rcdc_status take(ZstdScratch *sc, const ZstdSizes &S, const ZstdWindows &W, hipStream_t st) {
        HIP_TRY(hipStreamSynchronize(st));
        sc->blobs = (ZstdBlob *)alloc("blobs", S.nbo * sizeof(ZstdBlob));
        sc->blks = (ZstdBlk *)alloc("blks", S.nbl * sizeof(ZstdBlk));
        sc->tabs = (ZstdTables *)alloc("tabs", sizeof(ZstdTables));
        sc->slots = alloc("slots", S.maxw * kZstdSlot);
        sc->seq = (uint64_t *)alloc("seq", S.seq_words() * 8);
        sc->bpos = (uint64_t *)alloc("bpos", S.nbl * 8);
        sc->lens = (uint64_t *)alloc("lens", S.nbo * 8);
        sc->res = (uint2 *)alloc("res", S.nbl * 8);
        sc->queue = (uint32_t *)alloc("queue", S.queue_words() * 4);
        if (S.farw) sc->far = (uint32_t *)alloc("far", S.farw * 4);
        if (failed_) return fail(RCDC_ERR_INTERNAL, "zstd guard allocation");
        HIP_TRY(hipMemcpy(sc->blobs, W.blobs.data(), S.nbo * sizeof(ZstdBlob), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sc->blks, W.blks.data(), S.nbl * sizeof(ZstdBlk), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sc->tabs, &zstd_tables(), sizeof(ZstdTables), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(sc->queue, 0, S.queue_words() * 4));
        for (const GBuf &gb : gbufs_)
            fprintf(stderr, "rcdc zstd guarded %-6s [%p, %p)\n", gb.name, (void *)(gb.base + kG),
                    (void *)(gb.base + kG + gb.bytes));
        return RCDC_OK;
    }

    // After the launches: reports every guard byte that was written.
    rcdc_status report(hipStream_t st) {
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<uint8_t> gh(kG);
        for (const GBuf &gb : gbufs_)
            for (int side = 0; side < 2; side++) {
                const uint8_t *gp = side ? gb.base + kG + gb.bytes : gb.base;
                HIP_TRY(hipMemcpy(gh.data(), gp, kG, hipMemcpyDeviceToHost));
                int64_t lo = -1, hi = -1;
                for (uint64_t i = 0; i < kG; i++)
                    if (gh[i] != 0xCD) {
                        if (lo < 0) lo = (int64_t)i;
                        hi = (int64_t)i;
                    }
                if (lo >= 0)
                    fprintf(stderr, "rcdc zstd GUARD HIT %s %s: guard bytes %lld..%lld written\n", gb.name,
                            side ? "after" : "before", (long long)lo, (long long)hi);
            }
        return RCDC_OK;
    }

private:
    struct GBuf {
        uint8_t *base = nullptr;
        uint64_t bytes = 0;
        const char *name = "";
    };
    static constexpr uint64_t kG = 16ull << 20;
    std::vector<GBuf> gbufs_;
    bool failed_ = false;

    uint8_t *alloc(const char *nm, uint64_t bytes) {
        GBuf b;
        b.name = nm;
        b.bytes = bytes;
        if (hipMalloc((void **)&b.base, bytes + 2 * kG) != hipSuccess) {
            failed_ = true;
            return nullptr;
        }
        (void)hipMemset(b.base, 0xCD, bytes + 2 * kG);
        gbufs_.push_back(b);
        return b.base + kG;
    }
};

rcdc_status zstd_compress_args(rcdc_ctx *ctx, int level, const void *d_in, const rcdc_zstd_ref *refs,
                               uint32_t n, void *d_out, uint64_t *out_lens) {
    if (!valid_ctx(ctx) || (n && (!refs || !d_in || !d_out || !out_lens)))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    // zstd's accepted levels (ZSTD_minCLevel() .. ZSTD_maxCLevel(); decrypt.rs:20-24)
    if (level < -(1 << 17) || level > 22)
        return fail(RCDC_ERR_INVALID_INPUT, "zstd level %d outside [-131072, 22]", level);
    for (uint32_t i = 0; i < n; i++)
        if (refs[i].len > 0xFFFFFFFFull)  // decrypt.rs:479-487: data length must fit u32
            return fail(RCDC_ERR_UNSUPPORTED, "blob %u: %llu bytes", i,
                        (unsigned long long)refs[i].len);
    return RCDC_OK;
}

}  // namespace

extern "C" {

uint64_t rcdc_zstd_bound(uint64_t len) {
    return len + 3 * zstd_blocks(len) + (len > kZstdSingleMax ? 10 : 9);  // + the window byte
}

void rcdc_zstd_tables(void *out) { memcpy(out, &zstd_tables(), sizeof(ZstdTables)); }

uint64_t rcdc_zstd_tables_size(void) { return sizeof(ZstdTables); }

// Validate and plan the windows; lock and enter; size the scratch; upload the
// descriptors; one launch per window; read the frame lengths back; leave.
rcdc_status rcdc_zstd_compress(rcdc_ctx *ctx, int level, const void *d_in,
                               const rcdc_zstd_ref *refs, uint32_t n, void *d_out,
                               uint64_t *out_lens, void *hip_stream) {
    rcdc_status rs;
    if ((rs = zstd_compress_args(ctx, level, d_in, refs, n, d_out, out_lens))) return rs;
    if (!n) return RCDC_OK;
    const ZstdWindows W = zstd_windows(refs, n, zstd_window_blocks());
    ZstdEncState &Z = ctx->zenc;
    std::lock_guard<std::mutex> lk(Z.mu);
    DeviceGuard g(ctx->device);
    hipStream_t st;
    if ((rs = null_enter(ctx, hip_stream, &st))) return rs;
    ZstdSizes S;
    S.grid = zstd_block_grid((uint32_t)std::max(ctx->num_cus, 1), level);
    S.nbl = W.blks.size();
    S.nbo = W.blobs.size();
    S.maxw = W.maxw;
    S.farw = zstd_far_words(level, W.maxw);
    S.nwin = W.wins.size();
    ZstdScratch sc;
    if ((rs = zstd_enc_size(Z, S, &sc))) return rs;
    HIP_TRY(hipMemsetAsync(Z.d_queue, 0, S.queue_words() * 4, st));
    HIP_TRY(hipMemcpyAsync(Z.d_blobs, W.blobs.data(), S.nbo * sizeof(ZstdBlob),
                           hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Z.d_blks, W.blks.data(), S.nbl * sizeof(ZstdBlk),
                           hipMemcpyHostToDevice, st));
    if (const char *e = getenv("RCDC_ZSTD_DBG"); e && (atoi(e) & 32))
        zstd_dbg_buffers(Z, S, d_in, d_out, level);
    ZstdGuard guard;
    if (ZstdGuard::on() && (rs = guard.take(&sc, S, W, st))) return rs;
    for (size_t k = 0; k < W.wins.size(); k++) {
        const ZstdWin &w = W.wins[k];
        HIP_TRY(launch_zstd((const uint8_t *)d_in, (uint8_t *)d_out, sc.blobs + w.blob0,
                            (uint32_t)w.nblob, sc.blks + w.blk0, (uint32_t)w.nblk, sc.tabs,
                            sc.slots, sc.seq, S.grid, sc.res + w.blk0, sc.bpos + w.blk0,
                            sc.lens + w.blob0, sc.queue + 128 * k, sc.far, level, st));
    }
    if (ZstdGuard::on()) {
        if ((rs = guard.report(st))) return rs;
        HIP_TRY(hipMemcpy(out_lens, sc.lens, S.nbo * 8, hipMemcpyDeviceToHost));
        return null_leave(ctx, hip_stream, st);
    }
    HIP_TRY(hipMemcpyAsync(out_lens, Z.d_lens, S.nbo * 8, hipMemcpyDeviceToHost, st));
    // the host descriptors die with this call
    HIP_TRY(poll_stream(st));
    if (const char *e = getenv("RCDC_ZSTD_DBG"))
        if (atoi(e) & 4) zstd_prof_dump();
    return null_leave(ctx, hip_stream, st);
}

}  // extern "C"

// ---- frame checks ------------------------------------------------------------------

namespace {

// The block-parallel pass: a wave per block at the position it has when the
// frame's blocks are 128 KiB.  `order` gets the frames it could not settle.
rcdc_status zck_block_pass(ZckState &K, const uint8_t *frames, const uint8_t *data,
                           const rcdc_zstd_check_ref *refs, uint32_t n, uint32_t grid,
                           uint32_t *status, std::vector<uint32_t> &order, hipStream_t st) {
    uint32_t *ctr = K.d_order + n;
    std::vector<uint64_t> blk0(n + 1, 0);
    for (uint32_t i = 0; i < n; i++)
        blk0[i + 1] = blk0[i] + std::max<uint64_t>((refs[i].data_len + kZstdBlock - 1) / kZstdBlock, 1);
    const uint64_t nblk = blk0[n];
    rcdc_status rs;
    if ((rs = K.d_blk0.ensure(n + 1ull))) return rs;
    if ((rs = K.d_blks.ensure(nblk * zstd_blkdesc_bytes())))
        return rs;
    HIP_TRY(hipMemcpyAsync(K.d_blk0, blk0.data(), 8ull * (n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ctr, 0, 4, st));
    HIP_TRY(launch_zstd_check_blocks(frames, data, K.d_refs, K.d_blk0, n, K.d_blks, nblk,
                                     K.d_scratch, grid, K.d_status, ctr, st));
    HIP_TRY(hipMemcpyAsync(status, K.d_status, 4ull * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(poll_stream(st));
    for (uint32_t i = 0; i < n; i++)
        if (status[i] == 3u) order.push_back(i);
    return RCDC_OK;
}

}  // namespace

extern "C" {

// Frame checks.  Compressed frames: the block-parallel pass (a wave per
// block at the position it has when the frame's blocks are 128 KiB), then
// the frames it could not settle checked in order, a wave per frame, longest
// first.  Stored bytes: a wave per blob.
rcdc_status rcdc_zstd_check(rcdc_ctx *ctx, const void *d_frames, const void *d_data,
                            const rcdc_zstd_check_ref *refs, uint32_t n, uint32_t flags,
                            uint32_t *status, void *hip_stream) {
    if (!valid_ctx(ctx) || (n && (!refs || !d_frames || !d_data || !status)))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (!n) return RCDC_OK;
    const bool stored = (flags & RCDC_CHECK_STORED) != 0;
    static const bool blockpar = !(getenv("RCDC_CHECK_BLOCKS") && atoi(getenv("RCDC_CHECK_BLOCKS")) == 0);
    ZckState &K = ctx->zck;
    std::lock_guard<std::mutex> lk(K.mu);
    DeviceGuard g(ctx->device);
    hipStream_t st;
    rcdc_status rs;
    if ((rs = null_enter(ctx, hip_stream, &st))) return rs;
    // resident waves per CU (12 or 16, by the registers' budget)
    const uint32_t grid = (uint32_t)std::max(ctx->num_cus, 1) * zstd_check_waves_per_cu();
    if ((rs = K.d_refs.ensure(4ull * n))) return rs;
    if ((rs = K.d_order.ensure((uint64_t)n + 16))) return rs;
    if ((rs = K.d_status.ensure(n))) return rs;
    if ((rs = K.d_scratch.ensure(zstd_check_scratch_bytes(grid))))
        return rs;
    uint32_t *ctr = K.d_order + n;  // the queue counter sits after the order array
    const uint8_t *frames = (const uint8_t *)d_frames, *data = (const uint8_t *)d_data;
    HIP_TRY(hipMemcpyAsync(K.d_refs, refs, sizeof(rcdc_zstd_check_ref) * n, hipMemcpyHostToDevice, st));
    std::vector<uint32_t> order;
    if (!stored && blockpar) {
        if ((rs = zck_block_pass(K, frames, data, refs, n, grid, status, order, st))) return rs;
    } else {
        order.resize(n);
        for (uint32_t i = 0; i < n; i++) order[i] = i;
    }
    if (!order.empty()) {
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return refs[a].frame_len > refs[b].frame_len;
        });
        HIP_TRY(hipMemsetAsync(ctr, 0, 4, st));
        HIP_TRY(hipMemcpyAsync(K.d_order, order.data(), 4ull * order.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_zstd_check(frames, data, K.d_refs, K.d_order, (uint32_t)order.size(), stored,
                                  K.d_scratch, grid, K.d_status, ctr, st));
        HIP_TRY(hipMemcpyAsync(status, K.d_status, 4ull * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(poll_stream(st));
    }
    if (const char *e = getenv("RCDC_ZSTD_DBG"))
        if (atoi(e) & 8) zstd_check_prof_dump();
    return null_leave(ctx, hip_stream, st);
}

}  // extern "C"

// ---- frame decompression -------------------------------------------------------------

namespace {

// RCDC_ZDX_TIME: HIP-event times of the entropy kernels and of the copy
// kernel into the counters (tools/zstd_prof.py); a sync per group
struct ZdxTimer {
    const bool on;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ZdxTimer() : on(enabled()) {}
    ~ZdxTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    static bool enabled() {
        static const bool timed = getenv("RCDC_ZDX_TIME") && atoi(getenv("RCDC_ZDX_TIME"));
        return timed;
    }
    rcdc_status create() {
        if (on)
            for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
        return RCDC_OK;
    }
    rcdc_status mark(int k, hipStream_t st) {
        if (on) HIP_TRY(hipEventRecord(ev[k], st));
        return RCDC_OK;
    }
    rcdc_status add(uint64_t stats[8]) {
        float a = 0, c = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&c, ev[1], ev[2]));
        stats[6] += (uint64_t)(a * 1e3f);
        stats[7] += (uint64_t)(c * 1e3f);
        return RCDC_OK;
    }
};

struct ZdxCall {
    const uint8_t *frames;
    const rcdc_zstd_dec_ref *refs;
    uint32_t n, grid;
    bool blockpar;
    uint8_t *d_out;
    hipStream_t st;
};

// One group: descriptors, entropy (parallel, then in order), copy.  Indices
// inside a group count from its first frame.
rcdc_status zdx_run_group(ZdxState &X, const ZdxCall &C, const ZdxGroup &G,
                          const std::vector<uint32_t> &list, const std::vector<uint32_t> &order,
                          ZdxTimer &T) {
    const uint32_t m = G.b - G.a;
    const ZdxLayout lay = zdx_layout(G.nblk, G.data);
    uint32_t *d_list = X.d_order, *d_ord = X.d_order + C.n, *ctr = X.d_order + 2ull * C.n;
    const uint64_t *grefs = X.d_refs + 4ull * G.a;
    ZdxFrame *gfrm = X.d_frm + G.a;
    const ZdxPlace *gplace = X.d_place + G.a;
    hipStream_t st = C.st;
    rcdc_status rs;
    HIP_TRY(hipMemsetAsync(ctr, 0, 16, st));
    if (!list.empty())
        HIP_TRY(hipMemcpyAsync(d_list, list.data(), 4ull * list.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ord, order.data(), 4ull * m, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_zdx_blocks(C.frames, grefs, m, true, !C.blockpar, gplace, lay, X.d_ws, gfrm, st));
    if ((rs = T.mark(0, st))) return rs;
    if (C.blockpar)
        HIP_TRY(launch_zdx_entropy(C.frames, gfrm, lay, X.d_ws, G.nblk, C.grid, ctr, st));
    HIP_TRY(launch_zdx_inorder(C.frames, gfrm, gplace, d_list, (uint32_t)list.size(), lay, X.d_ws,
                               C.grid, ctr + 1, st));
    if ((rs = T.mark(1, st))) return rs;
    HIP_TRY(launch_zdx_copy(C.frames, grefs, gfrm, gplace, d_ord, m, lay, X.d_ws, C.d_out,
                            X.d_lens + G.a, X.d_status + G.a, C.grid, ctr + 2, st));
    return T.mark(2, st);
}

rcdc_status zdx_size(ZdxState &X, uint32_t n) {
    rcdc_status rs;
    if ((rs = X.d_refs.ensure(4ull * n))) return rs;
    if ((rs = X.d_lens.ensure(n))) return rs;
    if ((rs = X.d_frm.ensure(n))) return rs;
    if ((rs = X.d_place.ensure(n))) return rs;
    if ((rs = X.d_order.ensure(2ull * n + 16))) return rs;
    return X.d_status.ensure(n);
}

}  // namespace

extern "C" {

// Frame decompression: the header walk (counting), the workspace laid out
// from what it found, then per group of whole frames the header walk again
// (writing block descriptors), the parallel entropy stage, the in-order
// entropy pass for the flagged frames, and the copy stage.
rcdc_status rcdc_zstd_decompress(rcdc_ctx *ctx, const void *d_frames, const rcdc_zstd_dec_ref *refs,
                                 uint32_t n, uint32_t flags, void *d_out, uint64_t *out_lens,
                                 uint32_t *status, void *hip_stream) {
    if (!valid_ctx(ctx) || (n && (!refs || !d_frames || !d_out || !out_lens || !status)))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (flags) return fail(RCDC_ERR_INVALID_INPUT, "rcdc_zstd_decompress: unknown flags");
    // the data region's cap (the one rcdc_zstd_compress documents for its slots)
    static const uint64_t ws_max = getenv("RCDC_ZDX_WS_MAX")
                                       ? std::max<uint64_t>(strtoull(getenv("RCDC_ZDX_WS_MAX"), nullptr, 10), 1)
                                       : 4ull << 30;
    static const bool blockpar = !(getenv("RCDC_ZDX_BLOCKS") && atoi(getenv("RCDC_ZDX_BLOCKS")) == 0);
    ZdxState &X = ctx->zdx;
    std::lock_guard<std::mutex> lk(X.mu);
    memset(X.stats, 0, sizeof X.stats);
    if (!n) return RCDC_OK;
    DeviceGuard g(ctx->device);
    ZdxCall C{(const uint8_t *)d_frames, refs, n, 0, blockpar, (uint8_t *)d_out, nullptr};
    rcdc_status rs;
    if ((rs = null_enter(ctx, hip_stream, &C.st))) return rs;
    hipStream_t st = C.st;
    C.grid = (uint32_t)std::max(ctx->num_cus, 1) * zdx_waves_per_cu();
    if ((rs = zdx_size(X, n))) return rs;
    HIP_TRY(hipMemcpyAsync(X.d_refs, refs, sizeof(rcdc_zstd_dec_ref) * n, hipMemcpyHostToDevice, st));
    // 1. count: blocks and workspace bytes per frame
    const ZdxLayout none = zdx_layout(0, 0);
    HIP_TRY(launch_zdx_blocks(C.frames, X.d_refs, n, false, !blockpar, nullptr, none, nullptr, X.d_frm, st));
    std::vector<ZdxFrame> hf(n);
    HIP_TRY(hipMemcpyAsync(hf.data(), X.d_frm, sizeof(ZdxFrame) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(poll_stream(st));
    // 2. groups of whole frames within the cap
    const ZdxGroups R = zdx_groups(hf.data(), n, ws_max);
    if ((rs = X.d_ws.ensure(R.peak))) return rs;
    HIP_TRY(hipMemcpyAsync(X.d_place, R.place.data(), sizeof(ZdxPlace) * n, hipMemcpyHostToDevice, st));
    std::vector<uint32_t> list, order;
    ZdxTimer T;
    if ((rs = T.create())) return rs;
    // 3. per group: its work lists, then its kernels
    for (const ZdxGroup &G : R.groups) {
        zdx_group_lists(hf.data(), refs, G, list, order, X.stats);
        if ((rs = zdx_run_group(X, C, G, list, order, T))) return rs;
        // the next group's uploads reuse list / order: this group's are read
        if (R.groups.size() > 1 || T.on) HIP_TRY(poll_stream(st));
        if (T.on && (rs = T.add(X.stats))) return rs;
    }
    HIP_TRY(hipMemcpyAsync(status, X.d_status, 4ull * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_lens, X.d_lens, 8ull * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(poll_stream(st));
    X.stats[0] = n;
    X.stats[4] = R.groups.size();
    X.stats[5] = R.peak;
    return null_leave(ctx, hip_stream, st);
}

rcdc_status rcdc_zstd_decompress_stats(rcdc_ctx *ctx, uint64_t out[8]) {
    if (!valid_ctx(ctx) || !out) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    std::lock_guard<std::mutex> lk(ctx->zdx.mu);
    memcpy(out, ctx->zdx.stats, sizeof ctx->zdx.stats);
    return RCDC_OK;
}

// The header walk on the host: the first frame of `frame`.
rcdc_status rcdc_zstd_frame_info(const uint8_t *f, uint64_t len, uint64_t *content_size,
                                 uint64_t *out_bound, uint32_t *nblocks) {
    if (!f || !content_size || !out_bound || !nblocks)
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (len < 6 || f[0] != 0x28 || f[1] != 0xB5 || f[2] != 0x2F || f[3] != 0xFD)
        return fail(RCDC_ERR_INVALID_INPUT, "not a zstd frame");
    const uint32_t fhd = f[4];
    if (fhd & 8u) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: reserved bit set");
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, cksum = (fhd >> 2) & 1u,
                   did_flag = fhd & 3u;
    uint64_t q = 5 + (single ? 0 : 1);
    const uint32_t did_len = did_flag == 0 ? 0 : did_flag == 1 ? 1 : did_flag == 2 ? 2 : 4;
    const uint32_t fcs_len = fcs_flag == 0 ? (single ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
    if (q + did_len + fcs_len > len) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: header cut off");
    uint32_t did = 0;
    for (uint32_t j = 0; j < did_len; j++) did |= (uint32_t)f[q + j] << (8 * j);
    if (did) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: dictionaries are not supported");
    q += did_len;
    uint64_t fcs = 0;
    for (uint32_t j = 0; j < fcs_len; j++) fcs |= (uint64_t)f[q + j] << (8 * j);
    if (fcs_len == 2) fcs += 256;
    q += fcs_len;
    uint64_t bound = 0;
    uint32_t nb = 0;
    for (;;) {
        if (q + 3 > len) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: block header past the end");
        const uint32_t bh = f[q] | (f[q + 1] << 8) | ((uint32_t)f[q + 2] << 16);
        q += 3;
        const uint32_t last = bh & 1u, btype = (bh >> 1) & 3u, bsize = bh >> 3;
        const uint64_t csz = btype == 1 ? 1u : bsize;
        if (btype == 3) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: reserved block type");
        if (q + csz > len) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: block past the end");
        bound += btype == 2 ? (bsize ? kZstdBlock : 0u) : bsize;
        q += csz;
        nb++;
        if (last) break;
    }
    if (cksum && q + 4 > len) return fail(RCDC_ERR_INVALID_INPUT, "zstd frame: checksum cut off");
    *content_size = fcs_len ? fcs : UINT64_MAX;
    *out_bound = bound;
    *nblocks = nb;
    return RCDC_OK;
}

}  // extern "C"
