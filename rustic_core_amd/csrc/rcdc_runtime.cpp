// rcdc_runtime.cpp -- host runtime behind include/rcdc.h: errors, the
// context's create and destroy and what the family units share (rcdc_ctx.h),
// plans, lanes, the host-buffer path, streams and the SHA-256 entry points.
// The other kernel families have a unit each: rcdc_aead.cpp,
// rcdc_zstd_host.cpp, rcdc_place.cpp, rcdc_dindex.cpp, rcdc_ixparse.cpp.
//
// Owns the device (tables, work lists, summaries, cut lists, pinned staging)
// and maps the reference's chunker surface onto the two kernels:
//   rcdc_check_params  <- crates/core/src/chunker/rabin.rs:17-42
//   rcdc_parse_poly    <- crates/core/src/repofile/configfile.rs:165-175
//   rcdc_ctx_create    <- crates/core/src/chunker.rs:29-38 (Rabin64 tables once)
//   rcdc_chunk_batch   <- per-file parallel ChunkIter (archiver.rs:195)
//   rcdc_stream_*      <- one ChunkIter over a Read (rabin.rs:110-191)
//   rcdc_plan_*        <- device-resident batches (the measured path)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/rcdc.h"
#include "rcdc_ctx.h"
#include "rcdc_host.h"
#include "rcdc_internal.h"
#include "rcdc_launch.h"

using namespace rcdc;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
namespace {
thread_local std::string g_err;
}

rcdc_status rcdc::fail(rcdc_status st, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

namespace {

// ---------------------------------------------------------------------------
// GF(2) polynomial arithmetic for the Rabin64 tables (rustic_cdc Polynom64)
// ---------------------------------------------------------------------------
int poly_degree(uint64_t p) { return p ? 63 - __builtin_clzll(p) : -1; }

uint64_t poly_mod(uint64_t p, uint64_t m) {
    const int dm = poly_degree(m);
    while (p) {
        const int dp = poly_degree(p);
        if (dp < dm) break;
        p ^= m << (dp - dm);
    }
    return p;
}

// Device table image: [0,256) out[b] << 8, [256,512) mod[i]
// out[b] = b * x^(8*63) mod P;  mod[i] = ((i << deg) mod P) | (i << deg).
void build_tables(uint64_t poly, uint64_t *img) {
    const int deg = poly_degree(poly);
    for (uint64_t b = 0; b < 256; b++) {
        uint64_t h = poly_mod(b, poly);
        for (int i = 0; i < kWindow - 1; i++) h = poly_mod(h << 8, poly);
        img[b] = h << 8;
        const uint64_t p = b << deg;
        img[256 + b] = poly_mod(p, poly) | p;
    }
}

uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
}  // namespace

// ---------------------------------------------------------------------------
// context / plan objects
// ---------------------------------------------------------------------------
// What exists once per run in flight: the buffers one run's hashing kernels
// (scan, walk) write and its chain kernels (resolve, check, fixup, assemble)
// read, and what orders the two.  A plan runs on set 0; a pipelined plan
// (rcdc_plan_set_pipeline) alternates between sets 0 and 1.  Sized and
// cleared by plan_size_set.
struct WalkSet {
    DevBuf<uint4> sums;      // scan summaries
    DevBuf<uint64_t> masks;  // per scan item
    DevBuf<uint64_t> wpiece, pstatus;  // walk piece cuts and status
    DevBuf<uint64_t> wstate;           // WalkParams.wstate
    DevBuf<BoundRes> bres;
    DevBuf<uint32_t> ctr;
    DevBuf<uint32_t> fixlist;
    DevBuf<uint64_t> fixcuts;
    DevBuf<FixRes> fixres;
    // kWalkStats work counters.  Set 0: four slots (WalkParams.stats_next),
    // of which slot 0 is also its single buffer when counters are reset by
    // memsets; set 1: one slot, used only without kWalkKReset
    DevBuf<unsigned long long> wstats;
    // walk queue order.  Set 0: the plan's static order, then (cost
    // ordering) this set's sorted order and one key byte per piece; set 1:
    // its sorted order and key bytes only
    DevBuf<uint32_t> worder;
    uint32_t qbase = 0;  // walk queue counter at the set's next run (WalkParams.qbase)
    hipStream_t hstream = nullptr;  // hashing stream of a pipelined run
    hipEvent_t ev_in = nullptr, ev_scan = nullptr, ev_res = nullptr;
    bool res_pending = false;
};

struct rcdc_plan {
    rcdc_ctx *ctx = nullptr;
    uint32_t n = 0;
    uint64_t arena_len = 0;
    uint32_t seg_bytes = 0;
    uint32_t blocks = 0;
    uint64_t nseg = 0, ncuts = 0, scanned = 0;
    // capacity plans (single-stream host passes): the scan runs the first
    // run_items items (0: all) on run_blocks workgroups; set by plan_set_len
    uint32_t run_items = 0, run_blocks = 0;
    std::vector<ScanItem> items;
    std::vector<StreamDesc> sds;
    std::vector<uint64_t> cut_base;
    std::vector<ResolveUnit> units;
    std::vector<StitchDesc> stitches;
    uint64_t npiece_cuts = 0;
    // device
    DevBuf<ScanItem> d_items;
    DevBuf<StreamDesc> d_sds;
    DevBuf<ResolveUnit> d_units;
    DevBuf<StitchDesc> d_stitches;
    DevBuf<uint64_t> d_piece_cuts;
    DevBuf<uint64_t> d_piece_counts;
    DevBuf<uint64_t> d_cuts;
    DevBuf<uint64_t> d_counts;
    // walk path (long streams, rcdc_walk.hip)
    bool no_walk = false;             // force the scan path (fallback re-runs)
    bool no_pieces = false;           // one resolve unit per stream (capacity plans)
    std::vector<WalkUnit> wunits;
    std::vector<uint32_t> wstream_u0;  // unit0 of every walked stream
    std::vector<uint32_t> worder;      // walk queue order (big pieces first)
    uint32_t nsmall_units = 0;         // the split pieces at worder's end
    bool walk_many = false;            // pieces outnumber 2x the wave slots
    bool walk_cost = false;            // the queue is cost-sorted on every run
    uint64_t walk_small = 0;           // Ls of the split pieces
    std::vector<uint8_t> walked;       // per stream: on the walk path
    uint64_t nwpiece_cuts = 0;
    WalkParams wprm{};
    DevBuf<WalkUnit> d_wunits;
    DevBuf<uint32_t> d_wsu0;
    DevBuf<unsigned long long> d_wtrace;  // per-unit trace (RCDC_WALK_TRACE=1)
    uint64_t walk_epoch = 0;  // runs of the walk kernel (WalkParams.epoch)
    const void *last_arena = nullptr;  // of the last run (fallback re-runs)
    hipStream_t last_stream = nullptr;
    hipEvent_t done = nullptr;
    bool ran = false;
    // pipelined runs (rcdc_plan_set_pipeline): run k's hashing kernels (scan,
    // walk) go to hashing stream k % 2, its chain kernels (resolve, check,
    // fixup, assemble) to the chain stream.  Hashing k + 1 thus overlaps
    // chain k, and the next walk fills the tail of the previous one.  Every
    // per-run buffer the chain reads ping-pongs between the two sets.
    WalkSet sets[2];
    bool pipelined = false;
    // boundary-check workgroups of a pipelined run: the check is latency
    // bound and each workgroup holds a whole CU (128 KiB of LDS tables), so
    // overlapped with the next walk it runs on few CUs (RCDC_CHK_BLOCKS)
    uint32_t chk_blocks_pipe = 64;
    uint32_t fix_blocks_pipe = 64;  // chain workgroups beside the next walk (RCDC_CHAIN_BLOCKS;
                                    // 64 vs 32: C3 -0.7 %, C4 +1.5 %, profiles/r04/chain_blocks.txt)
    bool flush_next = false;          // the next pipelined run is the last: its chain runs on
                                      // every CU (rcdc_plan_set_pipeline(plan, 2))
    uint32_t pp = 0;                  // buffer set of the next run
    uint64_t wruns = 0;               // walk runs (the work-counter slot: wruns % 4)
    const unsigned long long *last_wstats = nullptr;  // the work counters the last run wrote
    hipStream_t rstream = nullptr;
    // SHA-256 of every chunk (rcdc_plan_hash), slot-indexed like d_cuts
    DevBuf<uint32_t> d_dig;
    DevBuf<uint32_t> d_shaw;   // length-bucket counters + total
    DevBuf<uint32_t> d_order;  // slots sorted by chunk length, longest first
    bool hashed = false;
    bool finished = false;           // rcdc_plan_finish done for the last run
    std::vector<uint64_t> fin_counts;  // per-stream counts after the finish
    // optional per-run kernel timing
    bool timing = false;
    uint32_t tperiod = 1;         // record every tperiod-th run (rcdc_plan_set_timing)
    uint64_t tcalls = 0;          // runs since timing was enabled
    std::vector<hipEvent_t> tev;  // 3 per timed run: before scan, after scan, after resolve
    uint64_t truns = 0;

    // Whoever destroys a plan has made its context's device current
    // (plan_free, plan_finish's temporary): the buffers are freed after this
    // body, by their own destructors.
    ~rcdc_plan() {
        for (WalkSet &S : sets) {
            if (S.ev_in) (void)hipEventDestroy(S.ev_in);
            if (S.ev_scan) (void)hipEventDestroy(S.ev_scan);
            if (S.ev_res) (void)hipEventDestroy(S.ev_res);
            if (S.hstream) (void)hipStreamDestroy(S.hstream);
        }
        if (rstream) (void)hipStreamDestroy(rstream);
        if (done) (void)hipEventDestroy(done);
        for (hipEvent_t e : tev) (void)hipEventDestroy(e);
    }
};

// One host-buffer worker of a context ("lane"): a HIP stream of its own, two
// pinned staging slots (the caller's pageable bytes are copied into one while
// the other's DMA runs), a device arena and a cached plan.  Calling threads
// take a free lane for the duration of a call, so concurrent files
// (archiver.rs:195) run on separate streams without a context-wide lock.
struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t *pinned[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t nslots = 2;
    uint64_t stage = 0;  // bytes per staging slot
    DevBuf<uint8_t> d_arena;
    rcdc_plan *plan = nullptr;
    std::vector<uint64_t> lay_offs, lay_lens;  // layout of the cached plan
    uint64_t lay_arena = 0;
    bool lay_cap = false;  // a capacity plan (one stream, length set per pass)
};

struct rcdc_stream {
    rcdc_ctx *ctx = nullptr;
    std::vector<uint8_t> pending;  // bytes from the current chunk start
    uint64_t base = 0;             // absolute offset of pending[0]
    uint64_t batch = 0;            // bytes buffered before a device pass
    bool done = false;
    std::deque<uint64_t> out;      // final cuts not yet handed to the caller
    // the same pending bytes, kept on the device after a pass, so the next
    // pass sends only the new bytes over PCIe (tail_len == pending.size()
    // when valid, 0 otherwise)
    uint8_t *d_tail = nullptr;  // from the context's pool, ctx->max + 256 bytes
    uint64_t tail_len = 0;
    hipEvent_t tail_ev = nullptr;  // the copy into d_tail (on the last pass's lane stream)
};

namespace rcdc {

// hip_stream == 0 selects the context's own stream.  That stream is created
// non-blocking, so on its own it is not ordered with the legacy default
// stream (torch's default stream is that stream).  A call given 0 is ordered
// as if it ran there: after the work queued on the default stream before
// the call (null_enter) and before the work queued there after it
// (null_leave).
rcdc_status null_enter(rcdc_ctx *ctx, const void *hip_stream, hipStream_t *st) {
    if (hip_stream) {
        *st = (hipStream_t)hip_stream;
        return RCDC_OK;
    }
    *st = ctx->stream;
    HIP_TRY(hipEventRecord(ctx->ev_null_in, nullptr));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_null_in, 0));
    return RCDC_OK;
}

rcdc_status null_leave(rcdc_ctx *ctx, const void *hip_stream, hipStream_t st) {
    if (hip_stream) return RCDC_OK;
    HIP_TRY(hipEventRecord(ctx->ev_null_out, st));
    HIP_TRY(hipStreamWaitEvent(nullptr, ctx->ev_null_out, 0));
    return RCDC_OK;
}

// Waits of the library's own calls poll (hipEventQuery + a 50 us sleep)
// instead of blocking in HIP: a thread blocked in hipStreamSynchronize /
// hipEventSynchronize held up other threads' launches and copies (the
// ingest engine's threads, r5r).  RCDC_POLL=0: blocking calls.
static bool poll_mode() {
    static const bool p = !(getenv("RCDC_POLL") && atoi(getenv("RCDC_POLL")) == 0);
    return p;
}

hipError_t poll_event(hipEvent_t ev) {
    if (!poll_mode()) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// One polling event per device and thread: an event can only be recorded on
// a stream of the device it was created on, and a thread may serve contexts
// on several GPUs.  The events are destroyed when the thread exits.
struct PollEvents {
    static constexpr int kMaxDev = 64;
    hipEvent_t ev[kMaxDev] = {};
    ~PollEvents() {
        for (int d = 0; d < kMaxDev; d++)
            if (ev[d] && hipSetDevice(d) == hipSuccess) (void)hipEventDestroy(ev[d]);
    }
};

hipError_t poll_stream(hipStream_t st) {
    if (!poll_mode()) return hipStreamSynchronize(st);
    thread_local PollEvents pe;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);  // the caller's DeviceGuard: the stream's device
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= PollEvents::kMaxDev) return hipStreamSynchronize(st);
    hipEvent_t &ev = pe.ev[dev];
    if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) {
        ev = nullptr;
        return e;
    }
    if ((e = hipEventRecord(ev, st)) != hipSuccess) return e;
    return poll_event(ev);
}

}  // namespace rcdc

namespace {

// Choose the per-lane segment S (multiple of 128 in [512, 4096]): the scan
// runs ceil(items / wave_slots) rounds of S + 64 slides per lane (64 = the
// warm-up window), items = sum over streams of ceil(ceil(span / S) / 64).
// Minimise rounds * (S + 64); ties go to the smaller S (finer summaries).
uint32_t choose_segment(const std::vector<uint64_t> &spans, int cus, int chains, int threads) {
    const uint64_t slots = (uint64_t)std::max(cus, 1) * (threads / 64) * chains;
    uint64_t best_cost = ~0ull;
    uint32_t best = 2048;
    for (uint32_t S = 512; S <= 4096; S += 128) {
        uint64_t items = 0;
        for (uint64_t sp : spans) items += ((sp + S - 1) / S + 63) / 64;
        const uint64_t rounds = std::max<uint64_t>((items + slots - 1) / slots, 1);
        const uint64_t cost = rounds * (S + kWindow);
        if (cost < best_cost) {
            best_cost = cost;
            best = S;
        }
    }
    return best;
}

// Arena offset of lane 0's first byte for a stream at `off`: aligned to
// `align` (a power of two, 16..128) unless that would start before the
// stream's first byte - 64, then 16-aligned.  64 (default) puts every 64-B
// register unit of every lane in one cache-line half: the unaligned layout
// fetched each line twice (profiles/r01_pmc_hbm.txt).  128 adds up to 63
// bytes per stream, which on 1 MiB streams costs an extra segment.
static inline uint64_t stream_q0(uint64_t off, uint64_t pos_lo, uint64_t align) {
    const uint64_t x = off + pos_lo - 65;
    const uint64_t q = x & ~(align - 1);
    return q + 64 >= off ? q : (x & ~(uint64_t)15);
}

static uint64_t q0_align() {
    const char *e = getenv("RCDC_Q0_ALIGN");  // experiments: 16, 32, 64, 128
    const uint64_t v = e ? (uint64_t)atoll(e) : 64;
    return (v == 128 || v == 64 || v == 32 || v == 16) ? v : (uint64_t)64;
}

// Resolver work list.  A stream of N >= kPieceStreams * min bytes is cut into
// pieces of Lp bytes (a multiple of min, >= 16 min), resolved speculatively in
// parallel and stitched (rcdc_resolve.hip).  Lp ~ sqrt(N * min / 2) balances
// the hops of one piece (Lp / chunk) against the stitch's per-piece step.
constexpr uint64_t kPieceStreams = 64;  // in units of min

static uint64_t piece_bytes(uint64_t N, uint64_t mn) {
    if (const char *e = getenv("RCDC_PIECE_BYTES")) {  // experiments; 0 disables
        const uint64_t v = (uint64_t)atoll(e);
        return v ? std::max<uint64_t>(v / mn, 1) * mn : 0;
    }
    if (N < kPieceStreams * mn) return 0;
    const double lp = std::sqrt((double)N * (double)mn / 2.0);
    return std::max<uint64_t>((uint64_t)(lp / (double)mn), 16) * mn;
}

void build_resolve_units(rcdc_plan *pl, uint64_t mn) {
    pl->units.clear();
    pl->stitches.clear();
    pl->npiece_cuts = 0;
    for (uint32_t i = 0; i < pl->n; i++) {
        if (pl->walked[i]) continue;
        const StreamDesc &d = pl->sds[i];
        const uint64_t N = d.n;
        const uint64_t Lp = pl->no_pieces ? 0 : piece_bytes(N, mn);
        if (Lp == 0 || N <= 2 * Lp) {
            ResolveUnit u{};
            u.start = 0;
            u.stop = N;
            u.out_base = d.cut_base;
            u.out_cap = (uint32_t)std::min<uint64_t>(d.cut_cap, 0xFFFFFFFFu);
            u.stream = i;
            u.direct = 1;
            pl->units.push_back(u);
            continue;
        }
        StitchDesc sd{};
        sd.stream = i;
        sd.unit0 = (uint32_t)pl->units.size();
        for (uint64_t a = 0; a < N; a += Lp) {
            ResolveUnit u{};
            u.start = a;
            u.stop = std::min(a + Lp, N);
            u.out_base = pl->npiece_cuts;
            // chunks >= min except the last: (stop - start) / min + the crossing cut
            u.out_cap = (uint32_t)((u.stop - u.start) / mn + 3);
            u.stream = i;
            u.direct = 0;
            pl->npiece_cuts += u.out_cap;
            pl->units.push_back(u);
        }
        sd.npieces = (uint32_t)pl->units.size() - sd.unit0;
        pl->stitches.push_back(sd);
    }
}

// Walk-path selection (rcdc_walk.hip).  The walk hashes what the reference
// hashes (~2/3 of random bytes, ~nothing of zero runs) but parallelises only
// over pieces of Lp bytes, so it needs many of them to fill the chip: a
// stream of N >= 2 Lp is walked when the plan's walkable bytes give at least
// kWalkMinPieces pieces.  Lp ~ walkable / (4 x 4096 wave slots), so the
// dynamic queue balances cheap (zero) and expensive (random) pieces, clamped
// to [4 MiB, 32 MiB] and a multiple of min.  RCDC_WALK_PIECE (bytes; 0 = scan
// path only) and RCDC_WALK_MIN_PIECES override.
constexpr uint64_t kWalkMinPieces = 1024;

static uint64_t walk_piece_bytes(const uint64_t *lens, uint32_t n, uint64_t mn, uint64_t mx) {
    uint64_t lp_env = ~0ull, min_pieces = kWalkMinPieces;
    if (const char *e = getenv("RCDC_WALK_PIECE")) lp_env = (uint64_t)atoll(e);
    if (const char *e = getenv("RCDC_WALK_MIN_PIECES")) min_pieces = (uint64_t)atoll(e);
    if (lp_env == 0) return 0;
    // Floor 4 MiB for files averaging >= 256 MiB, 3 MiB below (round-4 sweep
    // with seeded starts, profiles/r04/piece_sweep.txt: C4's 4-256 MiB files
    // +1.8 % at 3 MiB, C3's 1 GiB files -1.5 %).
    const uint64_t hi = 32ull << 20;
    uint64_t total = 0, nbig = 0;
    for (uint32_t i = 0; i < n; i++)
        if (lens[i] >= 6ull << 20) total += lens[i], nbig++;
    const uint64_t lo = nbig && total / nbig >= 256ull << 20 ? 4ull << 20 : 3ull << 20;
    uint64_t lp = lp_env != ~0ull ? lp_env : std::min(std::max(total / 32768, lo), hi);
    lp = std::max<uint64_t>(lp / mn, 1) * mn;
    (void)mx;
    uint64_t walkable = 0;
    for (uint32_t i = 0; i < n; i++)
        if (lens[i] >= 2 * lp) walkable += lens[i];
    if (walkable / lp < min_pieces) return 0;
    return lp;
}

// Sizes buffer set k of a built plan and clears what a first run expects
// cleared; work on `up` (nullptr: synchronous).  plan_build calls it for set
// 0, and for set 1 once rcdc_plan_set_pipeline has allocated that set, so a
// rebuild of a pipelined plan sizes both sets.  The two sets differ only in
// their order and work-counter buffers (WalkSet).
rcdc_status plan_size_set(rcdc_plan *pl, uint32_t k, hipStream_t up) {
    WalkSet &S = pl->sets[k];
    auto clear = [up](void *p, size_t bytes) {
        return up ? hipMemsetAsync(p, 0, bytes, up) : hipMemset(p, 0, bytes);
    };
    rcdc_status st;
    if ((st = S.sums.ensure(pl->nseg))) return st;
    if ((st = S.masks.ensure(pl->items.size()))) return st;
    const uint64_t nw = pl->wunits.size();
    if (!nw) return RCDC_OK;
    const uint64_t sorted = pl->walk_cost ? nw + (nw + 3) / 4 : 0;  // the order and its key bytes
    if (k == 0) {
        if ((st = S.worder.ensure(nw + sorted))) return st;
        HIP_TRY(up ? hipMemcpyAsync(S.worder, pl->worder.data(), nw * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, up)
                   : hipMemcpy(S.worder, pl->worder.data(), nw * sizeof(uint32_t),
                               hipMemcpyHostToDevice));
        if ((st = S.wstats.ensure(4 * kWalkStats))) return st;
        HIP_TRY(clear(S.wstats, 4 * kWalkStats * 8));
    } else {
        if (sorted && (st = S.worder.ensure(sorted))) return st;
        if ((st = S.wstats.ensure(kWalkStats))) return st;
    }
    if ((st = S.wpiece.ensure(pl->nwpiece_cuts))) return st;
    if ((st = S.pstatus.ensure(nw))) return st;
    if ((st = S.wstate.ensure(2 * nw))) return st;
    // epoch 0 = no run (a rebuilt plan keeps counting its runs)
    HIP_TRY(clear(S.wstate, 2 * nw * 8));
    if ((st = S.bres.ensure(nw))) return st;
    if ((st = S.ctr.ensure(4))) return st;
    HIP_TRY(clear(S.ctr, 16));
    S.qbase = 0;
    if ((st = S.fixlist.ensure(nw))) return st;
    if ((st = S.fixcuts.ensure(nw * pl->wprm.fix_cap))) return st;
    if ((st = S.fixres.ensure(nw))) return st;
    return RCDC_OK;
}

// up: the stream the work lists are uploaded on (nullptr: synchronous copies).
// Uploads from the plan's own host vectors, which stay unchanged until the
// next build of this plan (after its previous run has been waited for).
rcdc_status plan_build(rcdc_ctx *ctx, rcdc_plan *pl, const uint64_t *offs, const uint64_t *lens,
                       uint32_t n, uint64_t arena_len, hipStream_t up = nullptr) {
    const uint64_t pos_lo = ctx->min + kWindow;  // first pure-window test position
    pl->ctx = ctx;
    pl->n = n;
    pl->arena_len = arena_len;
    for (uint32_t i = 0; i < n; i++)
        if (offs[i] > arena_len || lens[i] > arena_len - offs[i])
            return fail(RCDC_ERR_INVALID_INPUT, "stream %u [%llu,+%llu) outside arena of %llu B", i,
                        (unsigned long long)offs[i], (unsigned long long)lens[i],
                        (unsigned long long)arena_len);
    const uint64_t Lp = pl->no_walk ? 0 : walk_piece_bytes(lens, n, ctx->min, ctx->max);
    pl->walked.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) pl->walked[i] = Lp && lens[i] >= 2 * Lp;
    std::vector<uint64_t> spans;
    spans.reserve(n);
    for (uint32_t i = 0; i < n; i++)
        if (!pl->walked[i] && lens[i] > pos_lo)
            spans.push_back(lens[i] - (stream_q0(offs[i], pos_lo, q0_align()) - offs[i] + 65));
    const int nc = 1;
    const int nthreads = scan_threads(ctx->variant);
    uint32_t S = choose_segment(spans, ctx->num_cus, nc, nthreads);
    if (const char *e = getenv("RCDC_SEG_BYTES")) S = (uint32_t)(atoi(e) / 128 * 128);  // experiments
    pl->seg_bytes = S;
    pl->items.clear();
    pl->sds.assign(n, StreamDesc{});
    pl->cut_base.assign(n, 0);
    uint64_t nseg = 0, ncut = 0;
    pl->scanned = 0;
    for (uint32_t i = 0; i < n; i++) {
        StreamDesc &d = pl->sds[i];
        const uint64_t N = lens[i], off = offs[i];
        d.off = off;
        d.n = N;
        d.cut_base = ncut;
        d.cut_cap = N / ctx->min + 1;
        pl->cut_base[i] = ncut;
        ncut += d.cut_cap;
        d.sum_base = nseg;
        d.item_base = pl->items.size();
        if (N <= pos_lo || pl->walked[i]) continue;
        // lane start q (arena offset) 16-aligned; tests positions q+65 ..
        const uint64_t q0 = stream_q0(off, pos_lo, q0_align());
        const uint64_t p0 = q0 - off + 65;
        const uint64_t segs = (N - p0 + S - 1) / S;
        d.pos0 = p0;
        d.nseg = segs;
        pl->scanned += segs * (uint64_t)S;
        for (uint64_t j = 0; j < segs; j += 64) {
            ScanItem it{};
            it.q0 = q0 + j * S;
            it.pos0 = p0 + j * S;
            it.lo = pos_lo;
            it.hi = N;
            it.sum_idx = nseg + j;
            const uint64_t rest = arena_len > it.q0 ? arena_len - it.q0 : 0;
            it.rec_bytes = std::min<uint64_t>(rest, 0xFFFFFFFFull);
            it.nvalid = (uint32_t)std::min<uint64_t>(64, segs - j);
            it.stream = i;
            pl->items.push_back(it);
        }
        nseg += segs;
    }
    pl->nseg = nseg;
    pl->ncuts = ncut;
    build_resolve_units(pl, ctx->min);
    // walk units: pieces of Lp bytes of every walked stream (the last one to
    // N), except that the last RCDC_WALK_SPLIT % (default 20) of a stream's
    // pieces are cut into pieces of Ls = Lp / 4 (a multiple of min).  Units
    // stay in stream order (the chain kernels need that); the walk kernel's
    // queue hands out all big pieces first and the small ones last, so the
    // last pieces the waves take are short and the grid drains evenly.
    pl->wunits.clear();
    pl->wstream_u0.clear();
    pl->worder.clear();
    pl->nwpiece_cuts = 0;
    {
        // splitting pays only when a wave takes several pieces (the tail is
        // then the last pieces' length); with about one piece per wave slot
        // (C5: 3200 pieces, 4096 slots) it only adds boundaries
        // a stream of N bytes has round(N / Lp) pieces of Lp, the last one
        // running to N (0.5 - 1.5 Lp): with floor(N / Lp) a stream just under
        // 3 Lp ended in a piece of ~2 Lp, the longest job of the queue (C4's
        // 8-12 MiB files: 8 MiB pieces started last and set the makespan)
        auto npieces = [Lp](uint64_t N) { return std::max<uint64_t>((N + Lp / 2) / Lp, 1); };
        uint64_t big_total = 0;
        for (uint32_t i = 0; i < n && Lp; i++)
            if (pl->walked[i]) big_total += npieces(lens[i]);
        const uint64_t slots = (uint64_t)std::max(ctx->num_cus, 1) * 16;
        pl->walk_many = big_total >= 2 * slots;
        uint64_t split_pct = pl->walk_many ? 20 : 0;
        if (const char *e = getenv("RCDC_WALK_SPLIT")) split_pct = std::min<uint64_t>(atoll(e), 100);
        const uint64_t Ls = Lp ? std::max<uint64_t>(Lp / 4 / ctx->min, 1) * ctx->min : 0;
        pl->walk_small = Ls;
        std::vector<uint32_t> small;
        for (uint32_t i = 0; i < n && Lp; i++) {
            if (!pl->walked[i]) continue;
            const uint64_t N = lens[i];
            const uint64_t P = npieces(N);
            const uint64_t nsplit = Ls < Lp ? (P * split_pct + 50) / 100 : 0;
            const uint32_t u0 = (uint32_t)pl->wunits.size();
            pl->wstream_u0.push_back(u0);
            uint32_t j = 0;
            auto add = [&](uint64_t a, uint64_t e, bool is_small) {
                WalkUnit u{};
                u.start = a;
                u.stop = e;
                u.out_base = pl->nwpiece_cuts;
                // cuts in [start, first cut >= stop]: >= min apart, plus the crossing and EOF cuts
                u.out_cap = (uint32_t)((e - a) / ctx->min + ctx->max / ctx->min + 4);
                u.stream = i;
                u.piece = j++;
                u.unit0 = u0;
                pl->nwpiece_cuts += u.out_cap;
                (is_small ? small : pl->worder).push_back((uint32_t)pl->wunits.size());
                pl->wunits.push_back(u);
            };
            for (uint64_t b = 0; b < P; b++) {
                const uint64_t a = b * Lp, e = b + 1 < P ? (b + 1) * Lp : N;
                if (b + nsplit < P) {
                    add(a, e, false);
                } else {
                    const uint64_t q = std::max<uint64_t>((e - a) / Ls, 1);
                    for (uint64_t k = 0; k < q; k++)
                        add(a + k * Ls, k + 1 < q ? a + (k + 1) * Ls : e, true);
                }
            }
            for (uint32_t k = u0; k < (uint32_t)pl->wunits.size(); k++) {
                pl->wunits[k].npieces = j;
                pl->wunits[k].nbig = (uint32_t)(P - nsplit);
            }
        }
        pl->worder.insert(pl->worder.end(), small.begin(), small.end());
        pl->nsmall_units = (uint32_t)small.size();
    }
    WalkParams &wp = pl->wprm;
    wp = WalkParams{};
    wp.min_size = ctx->min;
    wp.max_size = ctx->max;
    wp.arena_len = arena_len;
    wp.piece_bytes = Lp ? Lp : 1;
    wp.small_bytes = pl->walk_small ? pl->walk_small : wp.piece_bytes;
    // 64 lanes x 1.5 KiB per round: a chunk's search stops in its last
    // round (sized to the known search end), so shorter rounds hash less past
    // the cut and longer ones warm up less (64 B per segment); on C3 1536
    // beats 1024 by ~0.9 % and 768 / 2048 by 1-2 % (profiles/r03f)
    wp.seg_bytes = 1536;
    if (const char *e = getenv("RCDC_WALK_SEG")) wp.seg_bytes = (uint32_t)std::max(atoi(e) / 128 * 128, 128);
    wp.mask = (uint32_t)(ctx->avg - 1);
    wp.idx_shift = (uint32_t)(ctx->deg - 32);
    wp.shift = (uint32_t)(ctx->deg - 8);
    wp.nunits = (uint32_t)pl->wunits.size();
    // the walk's tail: waves without a piece hash rounds for the busy ones
    // (up to wp.helpers rounds posted per round of the walker's own, <= 15)
    wp.helpers = 7;
    if (const char *e = getenv("RCDC_WALK_HELPMAX")) wp.helpers = (uint32_t)std::min(std::max(atoi(e), 1), 15);
    if (const char *e = getenv("RCDC_WALK_HELP"); e && atoi(e) == 0) wp.helpers = 0;
    // a fixup walks until it meets a piece's chain: a few chunks, longer only
    // through phase-shifted zero runs (min-sized chunks); more -> host redo
    wp.fix_cap = (uint32_t)(4 * (Lp ? Lp : 1) / ctx->min + ctx->max / ctx->min + 64);
    wp.fix_seg = 512;
    wp.chk_budget = 4 * ctx->max;  // gap hashing in the check kernel (64 lanes) before the fixup (1024)
    // seeded piece starts (a walker continues its finished predecessor's chain)
    wp.seed = 1;
    if (const char *e = getenv("RCDC_WALK_SEED")) wp.seed = atoi(e) != 0;
    // queue classes by piece index mod K: even pieces before odd ones (K = 2)
    // for streams of many pieces; thirds (K = 3) when streams average under
    // 64 pieces (C4 share +1.2 %, lane/ref 1.110 -> 1.102; C3's 256-piece
    // streams lose 0.3 % at K = 3, profiles/r04/seed_classes.txt)
    const uint64_t nws = std::max<uint64_t>(pl->wstream_u0.size(), 1);
    wp.seed_classes = pl->wunits.size() / nws < 64 ? 3 : 2;
    // (RCDC_WALK_CLASSES: 1-8, experiments)
    if (const char *e = getenv("RCDC_WALK_CLASSES")) wp.seed_classes = (uint32_t)std::min(std::max(atoi(e), 1), 8);
    // a hit round stops early and spreads the lanes' owed tails (round_first)
    wp.early = 1;
    if (const char *e = getenv("RCDC_WALK_EARLY")) wp.early = atoi(e) != 0;
    // round 5: fast zones, in-kernel counter resets (RCDC_WALK_ZONEFAST /
    // RCDC_WALK_KRESET = 0 turn them off for A/B runs); the cost kernel on a
    // few fat workgroups with RCDC_COST_BLOCKS <= 256 (16: 312 us against 48 us
    // on the default grid, r5e)
    wp.flags = kWalkZoneFast | kWalkKReset;
    if (const char *e = getenv("RCDC_WALK_ZONEFAST"); e && atoi(e) == 0) wp.flags &= ~kWalkZoneFast;
    if (const char *e = getenv("RCDC_WALK_KRESET"); e && atoi(e) == 0) wp.flags &= ~kWalkKReset;
    wp.flags |= kWalkStatic;
    if (const char *e = getenv("RCDC_WALK_STATIC"); e && atoi(e) == 0) wp.flags &= ~kWalkStatic;
    wp.cost_blocks = 4096;
    wp.cost_samples = 64;
    if (const char *e = getenv("RCDC_COST_SAMPLES")) {
        const int v = atoi(e);
        wp.cost_samples = v >= 64 ? 64u : v >= 32 ? 32u : 16u;
    }
    if (const char *e = getenv("RCDC_COST_BLOCKS")) wp.cost_blocks = (uint32_t)std::max(atoi(e), 1);
    if (const char *e = getenv("RCDC_CHECK_BUDGET")) wp.chk_budget = strtoull(e, nullptr, 10);
    if (const char *e = getenv("RCDC_FIX_SEG")) wp.fix_seg = (uint32_t)std::max(atoi(e) / 128 * 128, 128);
    if (const char *e = getenv("RCDC_WALK_FIXCAP")) wp.fix_cap = (uint32_t)std::max(atoi(e), 1);  // tests
    const uint64_t supers = (pl->items.size() + nc - 1) / nc;
    const uint64_t waves_needed = (supers + nthreads / 64 - 1) / (nthreads / 64);
    pl->blocks = (uint32_t)std::min<uint64_t>(waves_needed, (uint64_t)std::max(ctx->num_cus, 1));

    DeviceGuard g(ctx->device);
    auto upload = [up](void *dst, const void *src, size_t bytes) {
        return up ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, up)
                  : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    rcdc_status st;
    if ((st = pl->d_items.ensure(pl->items.size()))) return st;
    if ((st = pl->d_sds.ensure(n))) return st;
    const uint64_t nw = pl->wunits.size();
    // the queue is cost-sorted only when waves take several pieces each: with
    // about one piece per wave slot the order hardly matters and the two
    // extra launches are most of C5's latency-bound step
    pl->walk_cost = nw && pl->walk_many;
    if (const char *e = getenv("RCDC_WALK_COSTSORT"); e && nw) pl->walk_cost = atoi(e) != 0;
    // (the sets here, before the cut arrays: a scan plan's allocations keep
    // the order they have always had)
    if ((st = plan_size_set(pl, 0, up))) return st;
    if (pl->sets[1].sums && (st = plan_size_set(pl, 1, up))) return st;  // a pipelined plan
    if ((st = pl->d_cuts.ensure(ncut))) return st;
    if ((st = pl->d_counts.ensure(n))) return st;
    if ((st = pl->d_units.ensure(pl->units.size()))) return st;
    if ((st = pl->d_stitches.ensure(pl->stitches.size()))) return st;
    if ((st = pl->d_piece_cuts.ensure(pl->npiece_cuts))) return st;
    if ((st = pl->d_piece_counts.ensure(pl->units.size()))) return st;
    if (nw) {
        if ((st = pl->d_wunits.ensure(nw))) return st;
        if ((st = pl->d_wsu0.ensure(pl->wstream_u0.size()))) return st;
        pl->wprm.nbig_units = (uint32_t)(nw - pl->nsmall_units);
        pl->wruns = 0;
        pl->wprm.trace = nullptr;
        if (const char *e = getenv("RCDC_WALK_TRACE"); e && atoi(e) > 0) {
            if ((st = pl->d_wtrace.ensure(2 * nw * kTraceWords))) return st;
            HIP_TRY(hipMemset(pl->d_wtrace, 0, 2 * nw * kTraceWords * 8));
            pl->wprm.trace = pl->d_wtrace;
        }
        HIP_TRY(upload(pl->d_wunits, pl->wunits.data(), nw * sizeof(WalkUnit)));

        HIP_TRY(upload(pl->d_wsu0, pl->wstream_u0.data(),
                          pl->wstream_u0.size() * sizeof(uint32_t)));
    }
    if (!pl->units.empty())
        HIP_TRY(upload(pl->d_units, pl->units.data(), pl->units.size() * sizeof(ResolveUnit)));
    if (!pl->stitches.empty())
        HIP_TRY(upload(pl->d_stitches, pl->stitches.data(),
                          pl->stitches.size() * sizeof(StitchDesc)));
    if (!pl->items.empty())
        HIP_TRY(upload(pl->d_items, pl->items.data(), pl->items.size() * sizeof(ScanItem)));
    if (n)
        HIP_TRY(upload(pl->d_sds, pl->sds.data(), n * sizeof(StreamDesc)));
    if (!pl->done) HIP_TRY(hipEventCreateWithFlags(&pl->done, hipEventDisableTiming));
    pl->ran = false;
    return RCDC_OK;
}

rcdc_status plan_run(rcdc_plan *pl, const void *d_arena, hipStream_t stream) {
    rcdc_ctx *ctx = pl->ctx;
    if (((uintptr_t)d_arena & 255u) != 0)
        return fail(RCDC_ERR_INVALID_INPUT, "device arena %p is not 256-byte aligned", d_arena);
    DeviceGuard g(ctx->device);
    const void *caller_stream = stream;
    if (rcdc_status ns = null_enter(ctx, caller_stream, &stream)) return ns;
    ScanParams sp{};
    sp.seg_bytes = pl->seg_bytes;
    sp.mask = (uint32_t)(ctx->avg - 1);
    sp.idx_shift = (uint32_t)(ctx->deg - 32);
    hipEvent_t *ev = nullptr;
    if (pl->timing && (pl->tcalls++ % pl->tperiod) == 0) {
        if (pl->tev.size() < 3 * (pl->truns + 1)) {
            for (int k = 0; k < 3; k++) {
                hipEvent_t e;
                HIP_TRY(hipEventCreate(&e));
                pl->tev.push_back(e);
            }
        }
        ev = &pl->tev[3 * pl->truns];
        pl->truns++;
    }
    const uint32_t set = pl->pipelined ? pl->pp : 0;
    WalkSet &S = pl->sets[set];
    // this run's walk parameters
    WalkParams wprm = pl->wprm;
    pl->walk_epoch = pl->walk_epoch % ((1ull << 21) - 1) + 1;  // 1 .. 2^21 - 1
    wprm.epoch = pl->walk_epoch;
    if (const uint64_t nw = pl->wunits.size()) {
        wprm.wstate = wprm.seed ? S.wstate.get() : nullptr;
        wprm.stats = S.wstats;
        uint32_t *const fixed = pl->sets[0].worder;  // the plan's static order
        wprm.order = fixed;
        if (pl->walk_cost) {  // the cost-sorted queue (and its key bytes) of this run
            wprm.order_in = fixed;
            wprm.order = wprm.order_out = set ? S.worder.get() : fixed + nw;
        }
    }
    bool ordered = false;  // the walk queue's order already enqueued
    if (pl->pipelined) {
        // hashing on this set's stream, after the caller's earlier work and
        // after the chain that last read this set (run k - 2)
        HIP_TRY(hipEventRecord(S.ev_in, stream));
        stream = S.hstream;
        HIP_TRY(hipStreamWaitEvent(stream, S.ev_in, 0));
        // the walk queue's cost order reads only the arena: it need not wait
        // for the chain of run k - 2, and fills CUs the last walk frees
        if (!pl->wunits.empty()) {
            HIP_TRY(launch_walk_order((const uint8_t *)d_arena, pl->d_sds, pl->d_wunits, wprm,
                                      stream));
            ordered = true;
        }
        if (S.res_pending) HIP_TRY(hipStreamWaitEvent(stream, S.ev_res, 0));
    }
    if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
    HIP_TRY(launch_scan(ctx->variant, (const uint8_t *)d_arena, pl->d_items,
                        pl->run_items ? pl->run_items : (uint32_t)pl->items.size(), ctx->d_tables,
                        sp, S.sums, S.masks, pl->run_items ? pl->run_blocks : pl->blocks, stream));
    const uint32_t cus = (uint32_t)std::max(ctx->num_cus, 1);
    static const bool dbg = getenv("RCDC_DEBUG_SYNC") != nullptr;  // stage-by-stage sync
    if (dbg) {
        HIP_TRY(hipStreamSynchronize(stream));
        fprintf(stderr, "rcdc: scan done\n");
    }
    // chain kernels beside the next walk run narrow; the last run of a
    // pipeline (flush) has no next walk and takes every CU
    const bool narrow = pl->pipelined && !pl->flush_next;
    pl->flush_next = false;
    const uint32_t wblocks = (uint32_t)std::min<uint64_t>(cus, (pl->wunits.size() + 15) / 16);
    wprm.qbase = S.qbase;
    wprm.stats_next = nullptr;
    if ((wprm.flags & kWalkKReset) && !pl->wunits.empty()) {
        const uint32_t slot = (uint32_t)(pl->wruns % 4);
        // the four slots of set 0, whichever set runs
        wprm.stats = pl->sets[0].wstats + slot * kWalkStats;
        wprm.stats_next = pl->sets[0].wstats + ((slot + 2) % 4) * kWalkStats;
        pl->wruns++;
    }
    pl->last_wstats = wprm.stats;
    HIP_TRY(launch_walk((const uint8_t *)d_arena, pl->d_sds, pl->d_wunits, wprm, ctx->d_tables,
                        S.wpiece, S.pstatus, S.ctr, wblocks, stream, ordered));
    if (!pl->wunits.empty() && (wprm.flags & kWalkKReset))  // takes of this run: one per
        S.qbase += (uint32_t)pl->wunits.size() +     // piece, one failed per wave;
                           ((wprm.flags & kWalkStatic) ? 0u : wblocks * 16u);  // static: nunits
    if (dbg) {
        HIP_TRY(hipStreamSynchronize(stream));
        uint32_t h[4] = {0, 0, 0, 0};
        if (!pl->wunits.empty()) HIP_TRY(hipMemcpy(h, S.ctr, 16, hipMemcpyDeviceToHost));
        fprintf(stderr, "rcdc: walk done (%zu units; queue %u)\n", pl->wunits.size(), h[0]);
    }
    if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
    const hipStream_t scan_stream = stream;
    if (pl->pipelined) {  // resolve on the plan's own stream, after this scan
        HIP_TRY(hipEventRecord(S.ev_scan, stream));
        stream = pl->rstream;
        HIP_TRY(hipStreamWaitEvent(stream, S.ev_scan, 0));
    }
    ResolveParams rp{};
    rp.min_size = ctx->min;
    rp.max_size = ctx->max;
    rp.seg_bytes = pl->seg_bytes;
    rp.mask = (uint32_t)(ctx->avg - 1);
    rp.shift = (uint32_t)(ctx->deg - 8);
    HIP_TRY(launch_resolve((const uint8_t *)d_arena, pl->d_sds, pl->d_units,
                           (uint32_t)pl->units.size(), pl->d_stitches,
                           (uint32_t)pl->stitches.size(), ctx->d_tables, rp, S.sums,
                           S.masks, pl->d_cuts, pl->d_counts, pl->d_piece_cuts,
                           pl->d_piece_counts, nullptr, stream));
    if (dbg) {
        HIP_TRY(hipStreamSynchronize(stream));
        fprintf(stderr, "rcdc: resolve done\n");
    }
    HIP_TRY(launch_walk_chain((const uint8_t *)d_arena, pl->d_sds, pl->d_wunits, pl->d_wsu0,
                              (uint32_t)pl->wstream_u0.size(), wprm, ctx->d_tables,
                              S.wpiece, S.pstatus, S.bres, S.ctr, S.fixlist,
                              S.fixcuts, S.fixres, pl->d_cuts, pl->d_counts,
                              narrow ? std::min<uint32_t>(cus, pl->fix_blocks_pipe) : cus,
                              narrow ? pl->chk_blocks_pipe : cus, stream,
                              pl->pipelined));
    if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
    if (pl->pipelined) {
        HIP_TRY(hipEventRecord(S.ev_res, stream));
        S.res_pending = true;
        pl->pp ^= 1u;
    }
    (void)scan_stream;
    pl->last_arena = d_arena;
    pl->last_stream = stream;
    HIP_TRY(hipEventRecord(pl->done, stream));
    // (pipelined runs stay asynchronous beyond the caller's stream: their
    // completion is rcdc_plan_finish / the device synchronisation)
    if (!pl->pipelined)
        if (rcdc_status ns = null_leave(ctx, caller_stream, stream)) return ns;
    pl->ran = true;
    pl->hashed = false;
    pl->finished = false;
    return RCDC_OK;
}

// SHA-256 of (offset, length) refs of the plan's last arena into the plan's
// digest slots (a stream the walk path handed back to the scan path).
rcdc_status launch_list_hash(rcdc_plan *pl, const std::vector<ulonglong2> &refs,
                             const std::vector<uint64_t> &slots) {
    DeviceGuard g(pl->ctx->device);
    ulonglong2 *d_refs = nullptr;
    uint32_t *d_out = nullptr;
    std::vector<uint8_t> out(refs.size() * 32);
    hipStream_t st = pl->ctx->stream;
    hipError_t e = hipMalloc((void **)&d_refs, refs.size() * sizeof(ulonglong2));
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, out.size());
    if (e == hipSuccess)
        e = hipMemcpy(d_refs, refs.data(), refs.size() * sizeof(ulonglong2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, pl->done, 0);  // after the plan's hash
    if (e == hipSuccess)
        e = launch_sha256_list((const uint8_t *)pl->last_arena, d_refs, (uint32_t)refs.size(),
                               d_out, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost);
    for (size_t r = 0; r < refs.size() && e == hipSuccess; r++)
        e = hipMemcpy((uint8_t *)pl->d_dig.get() + slots[r] * 32, out.data() + r * 32, 32,
                      hipMemcpyHostToDevice);
    (void)hipFree(d_refs);
    (void)hipFree(d_out);
    HIP_TRY(e);
    return RCDC_OK;
}


// Completes the last run: waits for it, redoes on the scan path any walked
// stream whose fixup overflowed (device count ~0; never seen outside forced
// tests) and writes those cuts -- and, if the run was hashed, their digests
// -- back into the device buffers, so the device views are complete.
rcdc_status plan_finish(rcdc_plan *pl) {
    if (!pl->ran) return fail(RCDC_ERR_INVALID_INPUT, "plan has not been run");
    if (pl->finished) return RCDC_OK;
    DeviceGuard g(pl->ctx->device);
    HIP_TRY(poll_event(pl->done));
    std::vector<uint64_t> &cnt = pl->fin_counts;
    cnt.assign(pl->n, 0);
    // read-backs on the run's own stream, not hipMemcpy: the legacy default
    // stream sits on one of HIP's hardware queues too, and a copy queued
    // there waits for whatever long kernel another stream put on that queue
    // (the ingest's 62 ms chunk-id kernels serialised its batches, r5l)
    if (pl->n) {
        HIP_TRY(hipMemcpyAsync(cnt.data(), pl->d_counts, pl->n * 8, hipMemcpyDeviceToHost,
                               pl->last_stream));
        HIP_TRY(poll_stream(pl->last_stream));
    }
    if (const char *e = getenv("RCDC_WALK_DUMP"); e && !pl->wunits.empty()) {  // debugging aid
        const uint32_t want = (uint32_t)atoi(e);
        const size_t nw = pl->wunits.size();
        std::vector<uint64_t> ps(nw), pc(pl->nwpiece_cuts);
        std::vector<BoundRes> br(nw);
        std::vector<FixRes> fr(nw);
        std::vector<uint64_t> fc(nw * pl->wprm.fix_cap);
        const WalkSet &S = pl->sets[0];  // (of a serial run)
        HIP_TRY(hipMemcpy(ps.data(), S.pstatus, nw * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pc.data(), S.wpiece, pc.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(br.data(), S.bres, nw * sizeof(BoundRes), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(fr.data(), S.fixres, nw * sizeof(FixRes), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(fc.data(), S.fixcuts, fc.size() * 8, hipMemcpyDeviceToHost));
        for (size_t u = 0; u < nw; u++) {
            const WalkUnit &U = pl->wunits[u];
            if (U.stream != want) continue;
            fprintf(stderr, "unit %zu piece %u [%llu,%llu) n=%llu open=%d:", u, U.piece,
                    (unsigned long long)U.start, (unsigned long long)U.stop,
                    (unsigned long long)(ps[u] & 0xFFFFFFFFu), (int)((ps[u] >> 32) & 1));
            for (uint64_t i = 0; i < (ps[u] & 0xFFFFFFFFu); i++) {
                const uint64_t v = pc[U.out_base + i];
                fprintf(stderr, " %llu%c", (unsigned long long)(v & kCutVal), "hmez"[v >> 62]);
            }
            if (U.piece) {
                const BoundRes &B = br[u];
                fprintf(stderr, "\n   bound kind %u nhops %u merge %u/%d fix_from %llu hops:", B.kind,
                        B.nhops, B.merge_unit, B.merge_idx, (unsigned long long)B.fix_from);
                for (uint32_t i = 0; i < B.nhops && i < (uint32_t)kMaxHops; i++)
                    fprintf(stderr, " %llu%s", (unsigned long long)(B.hops[i] & kCutVal),
                            (B.hops[i] >> 62) ? "r" : "");
                if (B.kind == kBoundFixup) {
                    fprintf(stderr, "\n   fix count %u merge %u/%d:", fr[u].count, fr[u].merge_unit,
                            fr[u].merge_idx);
                    for (uint32_t i = 0; i < fr[u].count && i < pl->wprm.fix_cap; i++)
                        fprintf(stderr, " %llu", (unsigned long long)fc[u * pl->wprm.fix_cap + i]);
                }
            }
            fprintf(stderr, "\n");
        }
    }
    std::vector<ulonglong2> refs;
    std::vector<uint64_t> slots;
    for (uint32_t i = 0; i < pl->n; i++) {
        if (cnt[i] != ~0ull) continue;
        rcdc_plan tmp;
        tmp.no_walk = true;
        const uint64_t off = pl->sds[i].off, len = pl->sds[i].n;
        rcdc_status st = plan_build(pl->ctx, &tmp, &off, &len, 1, pl->arena_len);
        if (!st) st = plan_run(&tmp, pl->last_arena, pl->last_stream);
        if (!st) st = tmp.done ? (hipEventSynchronize(tmp.done) == hipSuccess ? RCDC_OK
                                  : fail(RCDC_ERR_INTERNAL, "redo sync")) : RCDC_OK;
        uint64_t c1 = 0;
        std::vector<uint64_t> redo;
        if (!st && hipMemcpy(&c1, tmp.d_counts, 8, hipMemcpyDeviceToHost) != hipSuccess)
            st = fail(RCDC_ERR_INTERNAL, "redo counts");
        if (!st && c1 > pl->sds[i].cut_cap)
            st = fail(RCDC_ERR_INTERNAL, "stream %u: %llu cuts > bound", i, (unsigned long long)c1);
        if (!st) {
            redo.resize(c1);
            if (c1 && hipMemcpy(redo.data(), tmp.d_cuts, c1 * 8, hipMemcpyDeviceToHost) != hipSuccess)
                st = fail(RCDC_ERR_INTERNAL, "redo cuts");
        }
        if (st) return st;
        if (c1) HIP_TRY(hipMemcpy(pl->d_cuts + pl->cut_base[i], redo.data(), c1 * 8,
                                  hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(pl->d_counts + i, &c1, 8, hipMemcpyHostToDevice));
        cnt[i] = c1;
        uint64_t prev = 0;
        for (uint64_t j = 0; j < c1; j++) {
            refs.push_back({pl->sds[i].off + prev, redo[j] - prev});
            slots.push_back(pl->cut_base[i] + j);
            prev = redo[j];
        }
    }
    if (pl->hashed && !refs.empty()) {
        rcdc_status st = launch_list_hash(pl, refs, slots);
        if (st) return st;
    }
    pl->finished = true;
    return RCDC_OK;
}

rcdc_status plan_results(rcdc_plan *pl, uint64_t *cuts, uint64_t cap, uint64_t *counts) {
    rcdc_status st = plan_finish(pl);
    if (st) return st;
    const std::vector<uint64_t> &cnt = pl->fin_counts;
    uint64_t total = 0;
    for (uint32_t i = 0; i < pl->n; i++) {
        if (cnt[i] > pl->sds[i].cut_cap)
            return fail(RCDC_ERR_INTERNAL, "stream %u produced %llu cuts > bound %llu", i,
                        (unsigned long long)cnt[i], (unsigned long long)pl->sds[i].cut_cap);
        counts[i] = cnt[i];
        total += cnt[i];
    }
    if (total > cap) return fail(RCDC_ERR_CAPACITY, "need %llu cut slots, have %llu",
                                 (unsigned long long)total, (unsigned long long)cap);
    DeviceGuard g(pl->ctx->device);
    std::vector<uint64_t> all(pl->ncuts);
    if (pl->ncuts) {
        HIP_TRY(hipMemcpyAsync(all.data(), pl->d_cuts, pl->ncuts * 8, hipMemcpyDeviceToHost,
                               pl->last_stream));
        HIP_TRY(poll_stream(pl->last_stream));
    }
    uint64_t o = 0;
    for (uint32_t i = 0; i < pl->n; i++) {
        memcpy(cuts + o, all.data() + pl->cut_base[i], cnt[i] * 8);
        o += cnt[i];
    }
    return RCDC_OK;
}

void plan_free(rcdc_plan *pl) {
    if (!pl) return;
    DeviceGuard g(pl->ctx ? pl->ctx->device : 0);
    delete pl;
}

void lane_free(rcdc_ctx *ctx, Lane *L) {
    if (!L) return;
    DeviceGuard g(ctx->device);
    if (L->stream) (void)hipStreamSynchronize(L->stream);
    plan_free(L->plan);
    for (int k = 0; k < 4; k++) {
        if (L->ev[k]) (void)hipEventDestroy(L->ev[k]);
        if (L->pinned[k]) (void)hipHostFree(L->pinned[k]);
    }
    L->d_arena.release();
    if (L->stream) (void)hipStreamDestroy(L->stream);
    delete L;
}

// Take a free lane (creating one while fewer than max_lanes exist, else
// waiting for one); give it back with lane_release.
rcdc_status lane_acquire(rcdc_ctx *ctx, Lane **out) {
    std::unique_lock<std::mutex> lk(ctx->pool_mu);
    while (ctx->free_lanes.empty() && ctx->lanes.size() >= ctx->max_lanes) ctx->pool_cv.wait(lk);
    if (!ctx->free_lanes.empty()) {
        *out = ctx->free_lanes.back();
        ctx->free_lanes.pop_back();
        return RCDC_OK;
    }
    Lane *L = new Lane();
    ctx->lanes.push_back(L);  // counted now; its HIP objects are made below
    lk.unlock();
    DeviceGuard g(ctx->device);
    hipError_t e = hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking);
    for (int k = 0; k < 4 && e == hipSuccess; k++)
        e = hipEventCreateWithFlags(&L->ev[k], hipEventDisableTiming);
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> lk2(ctx->pool_mu);
        ctx->lanes.erase(std::find(ctx->lanes.begin(), ctx->lanes.end(), L));
        lane_free(ctx, L);
        ctx->pool_cv.notify_one();
        return fail(RCDC_ERR_INTERNAL, "lane setup: %s", hipGetErrorString(e));
    }
    *out = L;
    return RCDC_OK;
}

void lane_release(rcdc_ctx *ctx, Lane *L) {
    std::lock_guard<std::mutex> lk(ctx->pool_mu);
    ctx->free_lanes.push_back(L);
    ctx->pool_cv.notify_one();
}

// pinned staging per lane: 4 slots of 4 MiB (a 16-24 MiB stream pass's host
// copies run ahead of its own DMA; 2 x 16 MiB: 40-46 GiB/s, 4 x 4 MiB:
// 46.5-47.5 GiB/s through rcdc_stream_feed, tools/gpu_abi.sh)
constexpr uint64_t kStageBytes = 4ull << 20;

// RCDC_STAGE_MIB / RCDC_STAGE_SLOTS: staging slot size and count per lane
// (A/B runs; smaller slots overlap a pass's host copy with its own DMA, more
// slots let the copies run further ahead of the DMA)
static uint64_t stage_bytes() {
    static const uint64_t b = getenv("RCDC_STAGE_MIB")
                                  ? std::max<uint64_t>((uint64_t)atoll(getenv("RCDC_STAGE_MIB")), 1) << 20
                                  : kStageBytes;
    return b;
}

static uint32_t stage_slots() {
    static const uint32_t k = getenv("RCDC_STAGE_SLOTS")
                                  ? std::min<uint32_t>(std::max(atoi(getenv("RCDC_STAGE_SLOTS")), 2), 4)
                                  : 4u;
    return k;
}

// Capacity class of a single-stream host pass: a lane's plan is built for
// the class and reused for every length in it (the stream path's passes are
// 16 MiB plus a tail of up to max bytes: a plan per exact length rebuilt it
// on almost every pass).  Up to 64 MiB, built without walk pieces or
// resolver pieces (one resolve wave per pass: a few tens of hops).
static uint64_t cap_class(const rcdc_ctx *ctx, uint64_t n) {
    const uint64_t c = round_up(std::max<uint64_t>(n, 1), 8ull << 20);
    (void)ctx;
    return c <= (64ull << 20) ? c : 0;
}

// The plan (built for a capacity of one stream) set to length n: the
// stream's descriptor and the first items' end position on the device
// (values as kernel arguments: nothing to copy), and the items the scan runs.
static rcdc_status plan_set_len(rcdc_plan *pl, uint64_t n, hipStream_t st) {
    const StreamDesc &d = pl->sds[0];
    const uint64_t pos_lo = pl->ctx->min + kWindow;
    uint64_t nseg = 0;
    if (n > pos_lo && d.nseg) nseg = std::min<uint64_t>(d.nseg, (n - d.pos0 + pl->seg_bytes - 1) / pl->seg_bytes);
    const uint32_t nit = (uint32_t)((nseg + 63) / 64);
    pl->run_items = nit ? nit : 1;  // (an all-masked item when there is nothing to scan)
    const uint32_t waves = pl->run_items;
    pl->run_blocks = std::min<uint32_t>((waves + 15) / 16, (uint32_t)std::max(pl->ctx->num_cus, 1));
    HIP_TRY(launch_plan_set_len(pl->d_sds, pl->d_items, nit ? nit : (uint32_t)std::min<size_t>(1, pl->items.size()),
                                n, nseg, st));
    return RCDC_OK;
}

// Host-path phase timing (RCDC_HOST_PROFILE=1: summary on stderr when the
// context is destroyed): staging copies, waits for a staging slot, plan
// (re)builds, device run + result copy.
struct HostProfile {
    std::atomic<uint64_t> ns[4] = {{0}, {0}, {0}, {0}};
    std::atomic<uint64_t> passes{0}, bytes{0}, builds{0};
};
HostProfile g_hprof;
const bool g_hprof_on = getenv("RCDC_HOST_PROFILE") != nullptr;

inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Whether a host address lies in page-locked memory HIP knows of (pageable
// memory answers with an error or "unregistered"; the error is cleared so no
// later launch check sees it).
bool host_pinned(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// One piece of host memory at an arena offset.
struct HostPiece {
    uint64_t off;
    const uint8_t *p;
    uint64_t n;
};

// Host bytes -> pinned staging (two slots, copy k + 1 overlapping the DMA of
// copy k) -> the lane's device arena -> plan -> cuts, all on the lane's
// stream.  Stream i of the batch is the concatenation of its pieces (a
// streaming caller's buffered tail and its new read need no intermediate
// copy).  The plan is rebuilt only when the batch layout changes.
// d_prefix (optional): the first prefix_len bytes of the arena come from
// device memory (a stream's tail kept from its previous pass), not the host.
rcdc_status run_host_pieces(rcdc_ctx *ctx, Lane *L, const std::vector<uint64_t> &lens,
                            const std::vector<HostPiece> &pieces, uint64_t *cuts, uint64_t cap,
                            uint64_t *counts, const uint8_t *d_prefix = nullptr,
                            uint64_t prefix_len = 0, hipEvent_t prefix_ready = nullptr) {
    const uint32_t n = (uint32_t)lens.size();
    std::vector<uint64_t> offs(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        offs[i] = total;
        total = round_up(total + lens[i], 256);
    }
    const uint64_t arena_len = total + 256;
    // one stream short of pieces and walk: a plan per capacity class, set
    // to this pass's length on the device; otherwise a plan per exact layout
    static const bool capacity = !getenv("RCDC_EXACT_PLANS");
    const uint64_t cap1 = (capacity && n == 1) ? cap_class(ctx, lens[0]) : 0;
    std::vector<uint64_t> klens = cap1 ? std::vector<uint64_t>{cap1} : lens;
    const uint64_t karena = cap1 ? round_up(cap1, 256) + 256 : arena_len;
    DeviceGuard g(ctx->device);
    rcdc_status st;
    if ((st = L->d_arena.ensure(std::max(arena_len, karena)))) return st;
    if (!L->pinned[0]) {
        L->stage = stage_bytes();
        L->nslots = stage_slots();
        for (uint32_t k = 0; k < L->nslots; k++)
            HIP_TRY(hipHostMalloc((void **)&L->pinned[k], L->stage, hipHostMallocDefault));
    }
    uint64_t t_copy = 0, t_wait = 0, t0 = g_hprof_on ? now_ns() : 0;
    // From the first copy on, an early error return must not leave a DMA
    // from the caller's buffer (direct) or the lane's slots (staged) in
    // flight: the header promises the buffer is free on return, and the lane
    // goes back to the pool.  Disarmed once plan_results has waited.
    struct DrainOnError {
        hipStream_t s;
        bool armed = true;
        ~DrainOnError() {
            if (armed) (void)hipStreamSynchronize(s);
        }
    } drain{L->stream};
    if (prefix_len) {
        if (prefix_ready) HIP_TRY(hipStreamWaitEvent(L->stream, prefix_ready, 0));
        HIP_TRY(hipMemcpyAsync(L->d_arena, d_prefix, prefix_len, hipMemcpyDeviceToDevice,
                               L->stream));
    }
    // every piece page-locked (rcdc_host_alloc): DMA straight from the
    // caller's buffer; plan_results below waits for the pass, so the buffer
    // is free again when this returns
    static const bool direct_ok = !getenv("RCDC_NO_DIRECT_DMA");
    bool direct = direct_ok && !pieces.empty();
    for (size_t j = 0; direct && j < pieces.size(); j++)
        direct = host_pinned(pieces[j].p) && host_pinned(pieces[j].p + pieces[j].n - 1);
    if (direct)
        for (const HostPiece &pc : pieces)
            HIP_TRY(hipMemcpyAsync(L->d_arena + pc.off, pc.p, pc.n, hipMemcpyHostToDevice,
                                   L->stream));
    // staged copies: block k of the arena goes through slot k & 1
    size_t pi = 0;  // first piece that may overlap the block
    uint64_t k = 0;
    for (uint64_t p = prefix_len; !direct && p < total; p += L->stage, k++) {
        const uint64_t e = std::min(p + L->stage, total);
        const int slot = (int)(k % L->nslots);
        if (k >= L->nslots) {
            const uint64_t w0 = g_hprof_on ? now_ns() : 0;
            HIP_TRY(hipEventSynchronize(L->ev[slot]));  // its previous DMA is done
            if (g_hprof_on) t_wait += now_ns() - w0;
        }
        const uint64_t c0 = g_hprof_on ? now_ns() : 0;
        uint8_t *dst = L->pinned[slot];
        while (pi < pieces.size() && pieces[pi].off + pieces[pi].n <= p) pi++;
        for (size_t j = pi; j < pieces.size() && pieces[j].off < e; j++) {
            const uint64_t a = std::max(pieces[j].off, p), b = std::min(pieces[j].off + pieces[j].n, e);
            if (a < b) memcpy(dst + (a - p), pieces[j].p + (a - pieces[j].off), b - a);
        }
        if (g_hprof_on) t_copy += now_ns() - c0;
        HIP_TRY(hipMemcpyAsync(L->d_arena + p, dst, e - p, hipMemcpyHostToDevice, L->stream));
        HIP_TRY(hipEventRecord(L->ev[slot], L->stream));
    }
    const uint64_t b0 = g_hprof_on ? now_ns() : 0;
    // a lane's capacity plan serves any single-stream pass it covers (the
    // scan runs only the items the pass needs)
    const bool covers = cap1 && L->plan && L->lay_cap && L->lay_offs == offs &&
                        L->lay_lens.size() == 1 && L->lay_lens[0] >= lens[0];
    if (covers) klens = L->lay_lens;
    if (!covers &&
        (!L->plan || L->lay_offs != offs || L->lay_lens != klens || L->lay_arena != karena)) {
        if (!L->plan) L->plan = new rcdc_plan();
        L->plan->no_walk = L->plan->no_pieces = cap1 != 0;
        if ((st = plan_build(ctx, L->plan, offs.data(), klens.data(), n, karena, L->stream))) {
            L->lay_offs.clear();
            return st;
        }
        L->plan->run_items = 0;
        if (cap1 && (!L->plan->wunits.empty() || !L->plan->stitches.empty())) {
            // not the shape a length can be set on: exact plans from here
            L->plan->no_walk = L->plan->no_pieces = false;
            if ((st = plan_build(ctx, L->plan, offs.data(), lens.data(), n, arena_len, L->stream))) {
                L->lay_offs.clear();
                return st;
            }
            klens = lens;
        }
        L->lay_offs = offs;
        L->lay_lens = klens;
        L->lay_cap = cap1 && klens[0] == cap1;
        L->lay_arena = L->lay_cap ? karena : arena_len;
        if (g_hprof_on) g_hprof.builds++;
    }
    if (cap1 && L->lay_cap && (st = plan_set_len(L->plan, lens[0], L->stream))) return st;
    const uint64_t r0 = g_hprof_on ? now_ns() : 0;
    if ((st = plan_run(L->plan, L->d_arena, L->stream))) return st;
    st = plan_results(L->plan, cuts, cap, counts);
    drain.armed = st != RCDC_OK && st != RCDC_ERR_CAPACITY;  // capacity: the pass completed
    if (g_hprof_on) {
        const uint64_t t1 = now_ns();
        g_hprof.ns[0] += t_copy;
        g_hprof.ns[1] += t_wait;
        g_hprof.ns[2] += r0 - b0;
        g_hprof.ns[3] += t1 - r0;
        g_hprof.passes++;
        g_hprof.bytes += total;
        (void)t0;
    }
    return st;
}

rcdc_status run_host_batch(rcdc_ctx *ctx, Lane *L, const rcdc_buf *bufs, uint32_t n,
                           uint64_t *cuts, uint64_t cap, uint64_t *counts) {
    std::vector<uint64_t> lens(n);
    std::vector<HostPiece> pieces;
    pieces.reserve(n);
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (bufs[i].len && !bufs[i].data)
            return fail(RCDC_ERR_INVALID_INPUT, "buffer %u is NULL with length %llu", i,
                        (unsigned long long)bufs[i].len);
        lens[i] = bufs[i].len;
        if (bufs[i].len) pieces.push_back({off, bufs[i].data, bufs[i].len});
        off = round_up(off + bufs[i].len, 256);
    }
    return run_host_pieces(ctx, L, lens, pieces, cuts, cap, counts);
}

}  // namespace

// ---------------------------------------------------------------------------
// internal entry points for the ingest engine (rcdc_ingest.cpp), which is
// otherwise a client of the C ABI below
// ---------------------------------------------------------------------------
namespace rcdc {
bool valid_ctx(const rcdc_ctx *c) { return c != nullptr; }
// Rebuild `pl` (created by rcdc_plan_create, its last run waited for) for a
// new batch layout, reusing its device buffers; uploads on `up`.
rcdc_status plan_relayout(rcdc_plan *pl, const uint64_t *offs, const uint64_t *lens, uint32_t n,
                          uint64_t arena_len, hipStream_t up) {
    if (!pl || !pl->ctx) return fail(RCDC_ERR_INVALID_INPUT, "null plan");
    pl->ran = false;
    pl->finished = false;
    return plan_build(pl->ctx, pl, offs, lens, n, arena_len, up);
}
int ctx_device(const rcdc_ctx *ctx) { return ctx ? ctx->device : 0; }
uint64_t ctx_min_size(const rcdc_ctx *ctx) { return ctx ? ctx->min : 0; }
uint64_t ctx_max_size(const rcdc_ctx *ctx) { return ctx ? ctx->max : 0; }
rcdc_status set_error(rcdc_status st, const char *msg) { return fail(st, "%s", msg); }
}  // namespace rcdc

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

uint32_t rcdc_abi_version(void) { return RCDC_ABI_VERSION; }

const char *rcdc_last_error(void) { return g_err.c_str(); }

rcdc_status rcdc_check_params(uint64_t avg, uint64_t min, uint64_t max) {
    // rabin.rs:21-40, same order and same ErrorKind
    if (avg == 0 || (avg & (avg - 1)) != 0)
        return fail(RCDC_ERR_UNSUPPORTED,
                    "Chunk size must be a power of 2 for the rabin chunker. chunk size = %llu.",
                    (unsigned long long)avg);
    if (min > avg)
        return fail(RCDC_ERR_UNSUPPORTED,
                    "Chunk min size must be smaller or equal than the chunk size.");
    if (max < avg)
        return fail(RCDC_ERR_UNSUPPORTED,
                    "Chunk max size must be larger or equal than the chunk size.");
    // The reference accepts any min, but its iterator is only well defined
    // for min >= BUF_SIZE = 4096 (rabin.rs:12): a chunk that ends mid-buffer
    // leaves up to 4095 read-ahead bytes, and the next chunk does
    // `min_size -= open_buf_len` (rabin.rs:124).  Below 4096 that underflows:
    // a panic under debug assertions (the reference's test profile), and in
    // release a wrap that makes take(huge) return the whole remaining stream
    // as one chunk -- dependent on how the reader splits its reads, not a
    // function of the bytes.  No bit-exact cut list exists there, so such
    // parameters are Unsupported (the same ErrorKind as rabin.rs:22-40).
    if (min < (uint64_t)kRefBufSize)
        return fail(RCDC_ERR_UNSUPPORTED,
                    "Chunk min size must be at least 4096 bytes (the reference's read buffer, "
                    "rabin.rs:12,124). chunk min size = %llu.", (unsigned long long)min);
    if (avg > (1ull << 32) || max > (1ull << 40))
        return fail(RCDC_ERR_UNSUPPORTED, "chunk size > 4 GiB or max size > 1 TiB");
    return RCDC_OK;
}

rcdc_status rcdc_parse_poly(const char *hex, uint64_t *poly) {
    // u64::from_str_radix(s, 16): optional leading '+', hex digits only, no
    // prefix, no whitespace, non-empty, must fit in 64 bits.
    if (!hex || !poly) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    const char *p = hex;
    if (*p == '+') p++;
    if (!*p)
        return fail(RCDC_ERR_INVALID_INPUT,
                    "Parsing u64 from hex failed for polynomial `%s`, the value must be a valid "
                    "hexadecimal string.", hex);
    uint64_t v = 0;
    for (; *p; p++) {
        int d;
        if (*p >= '0' && *p <= '9') d = *p - '0';
        else if (*p >= 'a' && *p <= 'f') d = *p - 'a' + 10;
        else if (*p >= 'A' && *p <= 'F') d = *p - 'A' + 10;
        else
            return fail(RCDC_ERR_INVALID_INPUT,
                        "Parsing u64 from hex failed for polynomial `%s`, the value must be a "
                        "valid hexadecimal string.", hex);
        if (v >> 60)
            return fail(RCDC_ERR_INVALID_INPUT,
                        "Parsing u64 from hex failed for polynomial `%s`, the value must be a "
                        "valid hexadecimal string.", hex);
        v = (v << 4) | (uint64_t)d;
    }
    *poly = v;
    return RCDC_OK;
}

rcdc_status rcdc_ctx_create(uint64_t poly, uint64_t min, uint64_t avg_pow2, uint64_t max,
                            int device, rcdc_ctx **out) {
    if (!out) return fail(RCDC_ERR_INVALID_INPUT, "out is NULL");
    *out = nullptr;
    rcdc_status st = rcdc_check_params(avg_pow2, min, max);
    if (st) return st;
    const int deg = poly_degree(poly);
    // deg <= 56: `h << 8` of the reference's slide must not overflow u64;
    // deg >= 9: polynom_shift = deg - 8 must be positive
    if (deg < 9 || deg > 56)
        return fail(RCDC_ERR_UNSUPPORTED, "polynomial %#llx has degree %d; supported 9..56",
                    (unsigned long long)poly, deg);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(RCDC_ERR_INVALID_INPUT, "device %d not present (%d devices)", device, ndev);
    rcdc_ctx *c = new rcdc_ctx();
    c->device = device;
    c->poly = poly;
    c->min = min;
    c->avg = avg_pow2;
    c->max = max;
    c->deg = deg;
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        delete c;
        return fail(RCDC_ERR_INTERNAL, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    }
    c->num_cus = prop.multiProcessorCount;
    if (const char *v = getenv("RCDC_SCAN_VARIANT")) c->variant = atoi(v);
    if (const char *v = getenv("RCDC_LANES")) c->max_lanes = (uint32_t)std::max(atoi(v), 1);
    uint64_t img[512];
    build_tables(poly, img);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_null_in, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_null_out, hipEventDisableTiming)) != hipSuccess ||
        (e = hipMalloc((void **)&c->d_tables, sizeof img)) != hipSuccess ||
        (e = hipMemcpy(c->d_tables, img, sizeof img, hipMemcpyHostToDevice)) != hipSuccess) {
        rcdc_ctx_destroy(c);
        return fail(RCDC_ERR_INTERNAL, "context setup: %s", hipGetErrorString(e));
    }
    *out = c;
    return RCDC_OK;
}

void rcdc_ctx_destroy(rcdc_ctx *c) {
    if (!c) return;
    if (g_hprof_on && g_hprof.passes)
        fprintf(stderr,
                "rcdc host path: %llu passes, %.1f MiB, %llu plan builds; thread-summed ms: "
                "staging copy %.1f, slot waits %.1f, plan build %.1f, run+results %.1f\n",
                (unsigned long long)g_hprof.passes.load(), g_hprof.bytes.load() / 1048576.0,
                (unsigned long long)g_hprof.builds.load(), g_hprof.ns[0] / 1e6,
                g_hprof.ns[1] / 1e6, g_hprof.ns[2] / 1e6, g_hprof.ns[3] / 1e6);
    {
        DeviceGuard g(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        for (Lane *L : c->lanes) lane_free(c, L);
        (void)hipFree(c->d_tables);
        if (c->ev_null_in) (void)hipEventDestroy(c->ev_null_in);
        if (c->ev_null_out) (void)hipEventDestroy(c->ev_null_out);
        for (uint8_t *t : c->tail_all) (void)hipFree(t);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        delete c;  // what its members own, with the device still current
    }
}

uint64_t rcdc_max_cuts(const rcdc_ctx *c, uint64_t n) { return c ? n / c->min + 1 : 0; }

rcdc_status rcdc_chunk_batch(rcdc_ctx *ctx, const rcdc_buf *bufs, uint32_t n, uint64_t *cuts,
                             uint64_t cuts_cap, uint64_t *cut_counts) {
    if (!valid_ctx(ctx)) return fail(RCDC_ERR_INVALID_INPUT, "ctx is NULL");
    if (n && (!bufs || !cut_counts)) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    Lane *L = nullptr;
    rcdc_status st = lane_acquire(ctx, &L);
    if (st) return st;
    st = run_host_batch(ctx, L, bufs, n, cuts, cuts_cap, cut_counts);
    lane_release(ctx, L);
    return st;
}

rcdc_status rcdc_plan_create(rcdc_ctx *ctx, const uint64_t *offs, const uint64_t *lens,
                             uint32_t n, uint64_t arena_len, rcdc_plan **out) {
    if (!valid_ctx(ctx) || !out || (n && (!offs || !lens)))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    rcdc_plan *pl = new rcdc_plan();
    rcdc_status st = plan_build(ctx, pl, offs, lens, n, arena_len);
    if (st) {
        plan_free(pl);
        return st;
    }
    *out = pl;
    return RCDC_OK;
}

void rcdc_plan_destroy(rcdc_plan *plan) { plan_free(plan); }

rcdc_status rcdc_plan_run(rcdc_plan *plan, const void *d_arena, void *hip_stream) {
    if (!plan || (!d_arena && plan->arena_len))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    return plan_run(plan, d_arena, (hipStream_t)hip_stream);
}

rcdc_status rcdc_plan_results(rcdc_plan *plan, uint64_t *cuts, uint64_t cuts_cap,
                              uint64_t *cut_counts) {
    if (!plan || (plan->n && !cut_counts)) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    return plan_results(plan, cuts, cuts_cap, cut_counts);
}

rcdc_status rcdc_plan_device_results(rcdc_plan *plan, uint64_t *d_cuts, uint64_t *d_counts,
                                     const uint64_t **cut_base) {
    if (!plan || !d_cuts || !d_counts || !cut_base)
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    *d_cuts = (uint64_t)(uintptr_t)plan->d_cuts.get();
    *d_counts = (uint64_t)(uintptr_t)plan->d_counts.get();
    *cut_base = plan->cut_base.data();
    return RCDC_OK;
}

rcdc_status rcdc_plan_window(rcdc_plan *plan, uint32_t stream, uint64_t bound, uint32_t k,
                             uint64_t *d_out, void *hip_stream) {
    if (!plan || !d_out) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (stream >= plan->n)
        return fail(RCDC_ERR_INVALID_INPUT, "stream %u of a %u-stream plan", stream, plan->n);
    if (!plan->ran) return fail(RCDC_ERR_INVALID_INPUT, "plan has not been run");
    if (((uintptr_t)d_out & 7u) != 0) return fail(RCDC_ERR_INVALID_INPUT, "d_out not 8-B aligned");
    rcdc_ctx *ctx = plan->ctx;
    DeviceGuard g(ctx->device);
    hipStream_t st;
    if (rcdc_status ns = null_enter(ctx, hip_stream, &st)) return ns;
    // a pipelined run ends on the plan's chain stream: order after it
    if (plan->pipelined) HIP_TRY(hipStreamWaitEvent(st, plan->done, 0));
    HIP_TRY(launch_window(plan->d_cuts, plan->d_counts, stream, plan->cut_base[stream], bound, k,
                          d_out, st));
    return null_leave(ctx, hip_stream, st);
}

rcdc_status rcdc_plan_set_pipeline(rcdc_plan *plan, int enable) {
    if (!plan) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (!enable) {
        if (plan->pipelined && plan->ran) {
            DeviceGuard g(plan->ctx->device);
            HIP_TRY(hipEventSynchronize(plan->done));
        }
        plan->pipelined = false;
        plan->pp = 0;
        return RCDC_OK;
    }
    if (enable == 2) plan->flush_next = true;  // (set up below on first use)
    if (plan->pipelined) return RCDC_OK;
    DeviceGuard g(plan->ctx->device);
    if (plan->ran) HIP_TRY(hipEventSynchronize(plan->done));  // set 0's buffers are free
    rcdc_status st;
    if ((st = plan_size_set(plan, 1, nullptr))) return st;
    const int prio_mode = getenv("RCDC_PIPE_PRIO") ? atoi(getenv("RCDC_PIPE_PRIO")) : 0;
    int prio_lo = 0, prio_hi = 0;
    if (prio_mode) {
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        if (getenv("RCDC_PIPE_PRIO_PRINT"))
            fprintf(stderr, "rcdc: stream priorities %d..%d\n", prio_lo, prio_hi);
    }
    if (!plan->rstream) {
        if (prio_mode >= 3)  // the chain kernels first on freed CUs
            HIP_TRY(hipStreamCreateWithPriority(&plan->rstream, hipStreamNonBlocking, prio_hi));
        else
            HIP_TRY(hipStreamCreateWithFlags(&plan->rstream, hipStreamNonBlocking));
    }
    for (int k = 0; k < 2; k++) {
        if (!plan->sets[k].hstream) {
            // RCDC_PIPE_PRIO (experiments): the two hashing streams at different
            // priorities, so they sit on different hardware queues and run k + 1's
            // walk can start on the CUs run k's walk frees in its tail
            if (prio_mode == 1 || prio_mode == 2)
                HIP_TRY(hipStreamCreateWithPriority(&plan->sets[k].hstream, hipStreamNonBlocking,
                                                    k ? (prio_mode == 2 ? prio_lo : prio_hi) : prio_lo));
            else if (prio_mode == 4)  // three levels: chain high, the hashing streams low / middle
                HIP_TRY(hipStreamCreateWithPriority(&plan->sets[k].hstream, hipStreamNonBlocking,
                                                    k ? (prio_lo + prio_hi) / 2 : prio_lo));
            else
                HIP_TRY(hipStreamCreateWithFlags(&plan->sets[k].hstream, hipStreamNonBlocking));
        }
        if (!plan->sets[k].ev_in)
            HIP_TRY(hipEventCreateWithFlags(&plan->sets[k].ev_in, hipEventDisableTiming));
        if (!plan->sets[k].ev_scan)
            HIP_TRY(hipEventCreateWithFlags(&plan->sets[k].ev_scan, hipEventDisableTiming));
        if (!plan->sets[k].ev_res)
            HIP_TRY(hipEventCreateWithFlags(&plan->sets[k].ev_res, hipEventDisableTiming));
        plan->sets[k].res_pending = false;
    }
    plan->pp = 0;
    if (const char *e = getenv("RCDC_CHK_BLOCKS")) plan->chk_blocks_pipe = (uint32_t)std::max(atoi(e), 1);
    if (const char *e = getenv("RCDC_CHAIN_BLOCKS")) plan->fix_blocks_pipe = (uint32_t)std::max(atoi(e), 1);
    plan->pipelined = true;
    return RCDC_OK;
}

rcdc_status rcdc_plan_get_info(const rcdc_plan *plan, rcdc_plan_info *info) {
    if (!plan || !info) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    info->scanned_bytes = plan->scanned;
    info->segments = plan->nseg;
    info->segment_bytes = plan->seg_bytes;
    info->work_items = (uint32_t)plan->items.size();
    info->scan_blocks = plan->blocks;
    info->walk_pieces = (uint32_t)plan->wunits.size();
    info->walk_seg_bytes = plan->wprm.seg_bytes;
    info->pad = 0;
    return RCDC_OK;
}

rcdc_status rcdc_plan_walk_stats(rcdc_plan *plan, uint64_t *stats, uint64_t *trace,
                                 uint64_t trace_cap) {
    if (!plan || !stats) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    memset(stats, 0, RCDC_WALK_STATS * sizeof(uint64_t));
    if (plan->wunits.empty()) return RCDC_OK;
    if (!plan->ran) return fail(RCDC_ERR_INVALID_INPUT, "plan has not been run");
    DeviceGuard g(plan->ctx->device);
    HIP_TRY(hipEventSynchronize(plan->done));
    static_assert(RCDC_WALK_STATS == kWalkStats, "stats slots");
    HIP_TRY(hipMemcpy(stats, plan->last_wstats, kWalkStats * 8, hipMemcpyDeviceToHost));
    const uint64_t nw = 2 * plan->wunits.size() * kTraceWords;  // walk rows, then check rows
    if (trace && trace_cap && plan->wprm.trace)
        HIP_TRY(hipMemcpy(trace, plan->d_wtrace, std::min(trace_cap, nw) * 8,
                          hipMemcpyDeviceToHost));
    return RCDC_OK;
}

rcdc_status rcdc_plan_set_timing(rcdc_plan *plan, int enable) {
    if (!plan) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    plan->timing = enable > 0;
    if (enable > 0) {
        plan->truns = 0;
        plan->tcalls = 0;
        plan->tperiod = (uint32_t)enable;
    }
    return RCDC_OK;
}

rcdc_status rcdc_plan_kernel_times(rcdc_plan *plan, uint64_t *runs, double *scan_ms,
                                   double *resolve_ms) {
    if (!plan || !runs || !scan_ms || !resolve_ms)
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    DeviceGuard g(plan->ctx->device);
    double s = 0, r = 0;
    for (uint64_t i = 0; i < plan->truns; i++) {
        hipEvent_t *ev = &plan->tev[3 * i];
        HIP_TRY(hipEventSynchronize(ev[2]));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
        s += a;
        r += b;
    }
    *runs = plan->truns;
    *scan_ms = s;
    *resolve_ms = r;
    return RCDC_OK;
}

uint64_t rcdc_fixed_cuts(uint64_t n, uint64_t size, uint64_t *cuts, uint64_t cap) {
    // fixed_size.rs:41-70: `take(size).read_to_end`, short final chunk, none if empty
    if (size == 0) return 0;
    uint64_t k = 0;
    for (uint64_t s = 0; s < n;) {
        const uint64_t e = (n - s < size) ? n : s + size;
        if (k < cap) cuts[k] = e;
        k++;
        s = e;
    }
    return k;
}

rcdc_status rcdc_host_alloc(uint64_t bytes, void **out) {
    if (!out) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return RCDC_OK;
}

void rcdc_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

// ---- SHA-256 blob ids (crypto/hasher.rs:17-19, file_archiver.rs:151) -----

rcdc_status rcdc_sha256_host(const void *const *ptrs, const uint64_t *lens, uint32_t n,
                             uint8_t *digests) {
    if (n && (!ptrs || !lens || !digests)) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (!ptrs[i] && lens[i]) return fail(RCDC_ERR_INVALID_INPUT, "null buffer");
    if (!host_sha_supported()) return fail(RCDC_ERR_UNSUPPORTED, "CPU without AVX-512F/BW");
    host_sha256_many(reinterpret_cast<const uint8_t *const *>(ptrs), lens, n, digests);
    return RCDC_OK;
}

rcdc_status rcdc_sha256_chunks(rcdc_ctx *ctx, const void *d_arena, const rcdc_chunk_ref *d_refs,
                               uint32_t n, uint8_t *d_digests, void *hip_stream) {
    if (!valid_ctx(ctx) || (n && (!d_arena || !d_refs || !d_digests)))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (((uintptr_t)d_digests & 3) || ((uintptr_t)d_refs & 15))
        return fail(RCDC_ERR_INVALID_INPUT, "digests must be 4-byte and refs 16-byte aligned");
    DeviceGuard g(ctx->device);
    hipStream_t st;
    if (rcdc_status ns = null_enter(ctx, hip_stream, &st)) return ns;
    HIP_TRY(launch_sha256_list((const uint8_t *)d_arena, (const ulonglong2 *)d_refs, n,
                               (uint32_t *)d_digests, st));
    return null_leave(ctx, hip_stream, st);
}

rcdc_status rcdc_plan_hash(rcdc_plan *plan, const void *d_arena, void *hip_stream) {
    if (!plan || (!d_arena && plan->arena_len)) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (!plan->ran) return fail(RCDC_ERR_INVALID_INPUT, "plan has not been run");
    if (d_arena != plan->last_arena)
        return fail(RCDC_ERR_INVALID_INPUT, "arena differs from the last rcdc_plan_run");
    DeviceGuard g(plan->ctx->device);
    hipStream_t st;
    rcdc_status rs;
    if ((rs = null_enter(plan->ctx, hip_stream, &st))) return rs;
    if ((rs = plan->d_dig.ensure(plan->ncuts * 8))) return rs;
    if ((rs = plan->d_shaw.ensure(256))) return rs;
    if ((rs = plan->d_order.ensure(plan->ncuts))) return rs;
    if (st != plan->last_stream) HIP_TRY(hipStreamWaitEvent(st, plan->done, 0));
    HIP_TRY(launch_sha256_plan((const uint8_t *)d_arena, plan->d_sds, plan->n, plan->d_cuts,
                               plan->d_counts, plan->ncuts, plan->ctx->max, plan->d_shaw,
                               plan->d_order, plan->d_dig, st));
    HIP_TRY(hipEventRecord(plan->done, st));
    plan->hashed = true;
    return null_leave(plan->ctx, hip_stream, st);
}

rcdc_status rcdc_plan_hash_many(rcdc_plan *const *plans, uint32_t n,
                                const void *const *d_arenas, void *hip_stream) {
    if (n == 0) return RCDC_OK;
    if (!plans || !d_arenas) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (n > 8) return fail(RCDC_ERR_INVALID_INPUT, "at most 8 plans per call, got %u", n);
    rcdc_ctx *ctx = plans[0] ? plans[0]->ctx : nullptr;
    for (uint32_t j = 0; j < n; j++) {
        rcdc_plan *pl = plans[j];
        if (!pl || (!d_arenas[j] && pl->arena_len)) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
        if (!pl->ran) return fail(RCDC_ERR_INVALID_INPUT, "plan %u has not been run", j);
        if (d_arenas[j] != pl->last_arena)
            return fail(RCDC_ERR_INVALID_INPUT, "arena %u differs from its last rcdc_plan_run", j);
        if (pl->ctx != ctx) return fail(RCDC_ERR_INVALID_INPUT, "plans of different contexts");
        for (uint32_t i = 0; i < j; i++)
            if (plans[i] == pl) return fail(RCDC_ERR_INVALID_INPUT, "plan %u repeated", j);
    }
    DeviceGuard g(ctx->device);
    hipStream_t st;
    if (rcdc_status ns = null_enter(ctx, hip_stream, &st)) return ns;
    const uint8_t *ar[8];
    const StreamDesc *sd[8];
    uint32_t ns[8];
    const uint64_t *cu[8], *co[8];
    uint64_t nsl[8];
    uint32_t *bw[8], *od[8], *dg[8];
    for (uint32_t j = 0; j < n; j++) {
        rcdc_plan *pl = plans[j];
        rcdc_status rs;
        if ((rs = pl->d_dig.ensure(pl->ncuts * 8))) return rs;
        if ((rs = pl->d_shaw.ensure(256))) return rs;
        if ((rs = pl->d_order.ensure(pl->ncuts))) return rs;
        if (st != pl->last_stream) HIP_TRY(hipStreamWaitEvent(st, pl->done, 0));
        ar[j] = (const uint8_t *)d_arenas[j];
        sd[j] = pl->d_sds;
        ns[j] = pl->n;
        cu[j] = pl->d_cuts;
        co[j] = pl->d_counts;
        nsl[j] = pl->ncuts;
        bw[j] = pl->d_shaw;
        od[j] = pl->d_order;
        dg[j] = pl->d_dig;
    }
    HIP_TRY(launch_sha256_multi(n, ar, sd, ns, cu, co, nsl, ctx->max, bw, od, dg, st));
    for (uint32_t j = 0; j < n; j++) {
        HIP_TRY(hipEventRecord(plans[j]->done, st));
        plans[j]->hashed = true;
    }
    return null_leave(ctx, hip_stream, st);
}

rcdc_status rcdc_plan_finish(rcdc_plan *plan) {
    if (!plan) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    return plan_finish(plan);
}

rcdc_status rcdc_plan_digests(rcdc_plan *plan, uint8_t *digests, uint64_t cap_chunks,
                              uint64_t *cut_counts) {
    if (!plan || (plan->n && !cut_counts)) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (!plan->hashed) return fail(RCDC_ERR_INVALID_INPUT, "rcdc_plan_hash has not been run");
    rcdc_status rs = plan_finish(plan);
    if (rs) return rs;
    DeviceGuard g(plan->ctx->device);
    HIP_TRY(hipEventSynchronize(plan->done));  // the hash may follow the finish
    const std::vector<uint64_t> &cnt = plan->fin_counts;
    uint64_t total = 0;
    for (uint32_t i = 0; i < plan->n; i++) {
        cut_counts[i] = cnt[i];
        total += cnt[i];
    }
    if (total > cap_chunks)
        return fail(RCDC_ERR_CAPACITY, "need %llu digest slots, have %llu",
                    (unsigned long long)total, (unsigned long long)cap_chunks);
    std::vector<uint8_t> all(plan->ncuts * 32);
    if (plan->ncuts)
        HIP_TRY(hipMemcpy(all.data(), plan->d_dig, all.size(), hipMemcpyDeviceToHost));
    uint64_t o = 0;
    for (uint32_t i = 0; i < plan->n; i++) {
        memcpy(digests + o * 32, all.data() + plan->cut_base[i] * 32, cnt[i] * 32);
        o += cnt[i];
    }
    return RCDC_OK;
}

rcdc_status rcdc_plan_device_digests(rcdc_plan *plan, uint64_t *d_digests) {
    if (!plan || !d_digests) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    if (!plan->hashed) return fail(RCDC_ERR_INVALID_INPUT, "rcdc_plan_hash has not been run");
    *d_digests = (uint64_t)(uintptr_t)plan->d_dig.get();
    return RCDC_OK;
}

// ---- streaming: one file fed in pieces -------------------------------------

rcdc_status rcdc_stream_open(rcdc_ctx *ctx, rcdc_stream **out) {
    if (!valid_ctx(ctx) || !out) return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    rcdc_stream *s = new rcdc_stream();
    s->ctx = ctx;
    s->batch = rcdc_stream_batch_bytes(ctx);
    s->pending.reserve(s->batch + ctx->max);
    *out = s;
    return RCDC_OK;
}

void rcdc_stream_close(rcdc_stream *st) {
    if (st && st->tail_ev) {  // the last tail copy is done before d_tail is reused
        (void)hipEventSynchronize(st->tail_ev);
        (void)hipEventDestroy(st->tail_ev);
    }
    if (st && st->d_tail) {  // back to the context's pool
        std::lock_guard<std::mutex> lk(st->ctx->tail_mu);
        st->ctx->tail_pool.push_back(st->d_tail);
    }
    delete st;
}

uint64_t rcdc_stream_batch_bytes(const rcdc_ctx *ctx) {
    if (!ctx) return 0;
    // a pass per 16 MiB: large enough that a pass's fixed cost (plan, launch,
    // result copy) is small, small enough that a typical read size triggers a
    // pass straight from the caller's buffer (no intermediate copy)
    uint64_t b = 16ull << 20;
    if (const char *e = getenv("RCDC_STREAM_BATCH")) b = (uint64_t)atoll(e);
    return std::max<uint64_t>(b, 2 * ctx->max + 256);
}

uint64_t rcdc_stream_queued(const rcdc_stream *st) { return st ? st->out.size() : 0; }

// One device pass over the buffered bytes: every cut except the one at the
// end of the buffer depends only on bytes before it, so it is final; the
// end-of-buffer cut is final only at EOF.  The unfinished tail (< max bytes
// from the last final cut) stays buffered and is re-chunked with more data.
static rcdc_status stream_pass(rcdc_stream *st, const uint8_t *data, uint64_t len,
                               bool is_final) {
    rcdc_ctx *ctx = st->ctx;
    const uint64_t P = st->pending.size(), N = P + len;
    if (!N) return RCDC_OK;
    std::vector<uint64_t> tmp(rcdc_max_cuts(ctx, N));
    std::vector<uint64_t> lens{N};
    std::vector<HostPiece> pieces;
    // the pending bytes come from the device copy of the last pass's tail
    // when there is one; otherwise from the host buffer
    const bool dev_tail = P && st->d_tail && st->tail_len == P;
    if (P && !dev_tail) pieces.push_back({0, st->pending.data(), P});
    if (len) pieces.push_back({P, data, len});
    uint64_t cnt = 0;
    Lane *L = nullptr;
    rcdc_status s2 = lane_acquire(ctx, &L);
    if (s2) return s2;
    st->tail_len = 0;
    s2 = run_host_pieces(ctx, L, lens, pieces, tmp.data(), tmp.size(), &cnt,
                         dev_tail ? st->d_tail : nullptr, dev_tail ? P : 0,
                         dev_tail ? st->tail_ev : nullptr);
    uint64_t keep = cnt;
    if (!s2 && !is_final && cnt && tmp[cnt - 1] == N) keep = cnt - 1;
    const uint64_t consumed = keep ? tmp[keep - 1] : 0;
    static const bool devtail = !getenv("RCDC_STREAM_HOSTTAIL");
    if (!s2 && !is_final && N > consumed && devtail) {
        // keep the unfinished tail on the device for the next pass (the lane's
        // arena is reused as soon as the lane is released)
        // (the tail is the last, unfinished chunk: at most max bytes)
        DeviceGuard g(ctx->device);
        if (!st->d_tail) {
            std::lock_guard<std::mutex> lk(ctx->tail_mu);
            if (!ctx->tail_pool.empty()) {
                st->d_tail = ctx->tail_pool.back();
                ctx->tail_pool.pop_back();
            } else if (hipMalloc((void **)&st->d_tail, ctx->max + 256) == hipSuccess) {
                ctx->tail_all.push_back(st->d_tail);
            } else {
                st->d_tail = nullptr;
            }
        }
        // asynchronous: the next pass (any lane) waits on tail_ev before
        // it reads d_tail; the lane's next user queues behind the copy on
        // the same stream before it overwrites the arena
        if (!st->tail_ev && hipEventCreateWithFlags(&st->tail_ev, hipEventDisableTiming) != hipSuccess)
            st->tail_ev = nullptr;
        if (st->d_tail && st->tail_ev && N - consumed <= ctx->max + 256 &&
            hipMemcpyAsync(st->d_tail, L->d_arena + consumed, N - consumed,
                           hipMemcpyDeviceToDevice, L->stream) == hipSuccess &&
            hipEventRecord(st->tail_ev, L->stream) == hipSuccess)
            st->tail_len = N - consumed;
        s2 = RCDC_OK;  // without a device tail the next pass sends the host copy
    }
    lane_release(ctx, L);
    if (s2) return s2;
    for (uint64_t i = 0; i < keep; i++) st->out.push_back(st->base + tmp[i]);
    // the unfinished tail [consumed, N) becomes the new pending bytes (in
    // place: the buffer keeps its capacity)
    if (consumed < P) {
        st->pending.erase(st->pending.begin(), st->pending.begin() + (long)consumed);
        st->pending.insert(st->pending.end(), data, data + len);
    } else {
        const uint64_t d0 = consumed - P;
        st->pending.assign(data + d0, data + len);
    }
    st->base += consumed;
    return RCDC_OK;
}

rcdc_status rcdc_stream_feed(rcdc_stream *st, const uint8_t *data, uint64_t len, int is_final,
                             uint64_t *cuts, uint64_t cap, uint64_t *n_cuts) {
    if (!st || !n_cuts || (len && !data) || (cap && !cuts))
        return fail(RCDC_ERR_INVALID_INPUT, "null argument");
    *n_cuts = 0;
    if (st->done && len) return fail(RCDC_ERR_INVALID_INPUT, "stream already finished");
    if (!st->done) {
        // a device pass once enough bytes are buffered that cuts are certain
        // (every chunk ends by chunk start + max), or at EOF; the new bytes
        // go straight from the caller's buffer to the staging slots
        if (is_final || st->pending.size() + len >= st->batch) {
            rcdc_status s2 = stream_pass(st, data, len, is_final != 0);
            if (s2) {
                // keep the bytes buffered: the caller may retry the feed with
                // len = 0, or close the stream
                st->pending.insert(st->pending.end(), data, data + len);
                return s2;
            }
            if (is_final) {
                st->pending.clear();
                st->done = true;
            }
        } else {
            st->pending.insert(st->pending.end(), data, data + len);
        }
    }
    // hand out what fits; the rest stays queued for the next call
    uint64_t k = 0;
    while (k < cap && !st->out.empty()) {
        cuts[k++] = st->out.front();
        st->out.pop_front();
    }
    *n_cuts = k;
    return RCDC_OK;
}

}  // extern "C"
