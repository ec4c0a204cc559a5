// rcdc_ingest.cpp -- the backup data path from files in host memory to pack
// files and pack ids in host memory, native (include/rcdc.h "ingest").
//
// Reference (rustic_core 0.12.0):
//   FileArchiver::backup_reader (archiver/file_archiver.rs:144-160): read a
//     file, ChunkIter, `hash(&chunk)`, `index.has_data`, `Packer::add`;
//   Packer (blob/packer.rs): process_data = zstd + Key::encrypt_data
//     (backend/decrypt.rs:478-506, 566-572) + extra_verify (:508-529),
//     add_raw (:615-655), should_save / PackSizer (:65-200, 659-671),
//     save + write_header (:693-735), finalize (:385-398);
//   the file writer's pack id: hash_reader of the pack file (:826-836).
//
// The engine is a client of the C ABI (rcdc_plan_*, rcdc_sha256_chunks,
// rcdc_zstd_compress, rcdc_aead_seal / _open, rcdc_zstd_check,
// rcdc_pack_build_raw_multi, rcdc_copy_ranges, the host SHA-256) -- the call
// sequence a Rust integration would run -- with its own threads:
//   callers      reserve space in a page-locked input slot, read a file into
//                it (the reference's Read), commit;
//   worker       per batch (one closed input slot): H2D, chunk, ids of the
//                short chunks on the device, zstd + seal + verify of every
//                chunk (stage A); once the batch's ids are in: dedup in chunk
//                order, per-file results, PackSizer grouping with the packer
//                open across batches, pack build, D2H (stage B);
//   pool         SHA-256 on the host: the long chunks' ids from the input
//                slot (a device lane needs ~0.27 s for an 8 MiB chain, a host
//                core ~4 ms) and the pack ids from the pinned pack buffer;
//   waiter       waits for each batch's pack D2H and hands the packs to the
//                pool, whose last job per pack calls the caller's callback.
// Stage A of batch b + 1 .. b + depth - 1 runs before stage B of batch b, so
// the short ids' device chains of several batches overlap.
//
// Streams (rcdc_ingest_stream_*): a file of any length arrives as pieces in
// several slots.  Each batch chunks a stream's bytes of that batch after
// its carry -- the open chunk of the previous batch, at most max bytes, kept
// in a device carry slot (and a host copy for host-hashed ids) -- as one
// plan stream; all but the last chunk are final (a cut at L depends only on
// the bytes before L and the chunk start, rabin.rs:153-188), the last one
// becomes the next carry.  Pieces that are not contiguous in the slot, or
// follow a carry, are gathered into the arena's assembly region first
// (one D2D copy at HBM rate, against the piece's PCIe copy).  Slots holding
// stream pieces enter the pipeline in the order they closed.
#include <hip/hip_runtime.h>

#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/rcdc.h"
#include "rcdc_host.h"
#include "rcdc_ingest_steps.h"
#include "rcdc_launch.h"

using namespace rcdc;
using steps::PackSizer;

namespace {

constexpr uint32_t kSrcStaging = 0, kSrcCarry = 1;

uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

void random_bytes(uint8_t *p, size_t n) {  // the nonces (aespoly1305.rs:120-121: OS RNG)
    while (n) {
        const ssize_t r = getrandom(p, n, 0);
        if (r <= 0) continue;
        p += r;
        n -= (size_t)r;
    }
}

struct Id32 {
    uint8_t b[32];
    bool operator==(const Id32 &o) const { return memcmp(b, o.b, 32) == 0; }
};
struct Id32Hash {
    size_t operator()(const Id32 &x) const {
        uint64_t v;
        memcpy(&v, x.b, 8);
        return (size_t)v;  // ids are SHA-256 digests: any 8 bytes are uniform
    }
};

// ---- owners: whoever holds one frees it, with the engine's device current --
// A HIP event or stream, move-only.
template <typename H, hipError_t (*Destroy)(H)>
struct HipOwner {
    H h = nullptr;
    HipOwner() = default;
    HipOwner(HipOwner &&o) noexcept : h(o.h) { o.h = nullptr; }
    ~HipOwner() { reset(); }
    void reset() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator H() const { return h; }
};
using Stream = HipOwner<hipStream_t, hipStreamDestroy>;
struct Event : HipOwner<hipEvent_t, hipEventDestroy> {
    hipError_t create() { return hipEventCreateWithFlags(&h, hipEventDisableTiming); }
};

// The engine's allocations: counted (rcdc_ingest_mem_live) and, in create,
// failable on demand (RCDC_INGEST_FAIL_ALLOC).
hipError_t ing_alloc(rcdc_ingest *g, void **p, uint64_t n, bool pinned);
hipError_t ing_free(void *p);

// One buffer of the engine: device memory or page-locked host memory,
// `cap` elements, freed by its holder's destructor.
template <typename T>
struct IngBuf {
    T *p = nullptr;
    uint64_t cap = 0;
    bool pinned = false;
    IngBuf() = default;
    IngBuf(const IngBuf &) = delete;
    ~IngBuf() { (void)release(); }
    operator T *() const { return p; }
    hipError_t release() {
        T *q = p;
        p = nullptr, cap = 0;
        return q ? ing_free(q) : hipSuccess;
    }
    // exactly n elements (create)
    hipError_t alloc(rcdc_ingest *g, uint64_t n, bool pin) {
        pinned = pin;
        const hipError_t e = ing_alloc(g, (void **)&p, n * sizeof(T), pin);
        cap = e == hipSuccess ? n : 0;
        return e;
    }
    // At least `need` elements; when that takes a new allocation, one of
    // `grown` elements -- each site's own headroom rule -- and the contents
    // are lost.  False: the engine's error is set.
    bool ensure(rcdc_ingest *g, uint64_t need, uint64_t grown, const char *what);
};

// One stream (rcdc_ingest_stream_open .. close): its carry between batches
// and its results so far.  Fields by owner: `fed`, `open_pieces`, `closed`
// under the engine's mutex (callers); `base`, `carry_len`, `hcarry`,
// `cslot` on the worker thread (stage A, in batch order); `cuts`, `ids`,
// `nnew` on the back thread (stage B, in batch order).
struct StreamSt {
    uint64_t handle = 0, tag = 0, hint = 0;
    uint64_t fed = 0;          // bytes committed
    uint32_t open_pieces = 0;  // reserved, not committed or cancelled
    bool closed = false, aborted = false;
    int cslot = -1;            // device carry slot
    uint64_t base = 0;         // stream offset of the carry's first byte (the last final cut)
    uint64_t carry_len = 0;
    std::vector<uint8_t> hcarry;
    std::vector<uint64_t> cuts;
    std::vector<uint8_t> ids;
    uint32_t nnew = 0;
};

struct FileEnt {
    uint64_t tag = 0;
    uint64_t off = 0;   // in the batch (whole files 256-aligned)
    uint64_t res = 0;   // bytes reserved
    uint64_t len = 0;   // bytes committed
    bool done = false;
    bool cancelled = false;
    bool final = false;  // a stream's end (close / abort): zero bytes
    std::shared_ptr<StreamSt> st;  // null: a whole file
};

// One plan stream of a batch: a whole file in place, or a stream's bytes of
// this batch (after its carry), in place or gathered in the assembly region.
struct Unit {
    uint64_t tag = 0;
    std::shared_ptr<StreamSt> st;
    bool final = true, aborted = false;
    uint64_t base = 0;       // stream offset of the unit's first byte
    uint64_t carry = 0;      // leading carry bytes
    uint64_t off = 0, len = 0;
    uint64_t fresh = 0;      // bytes new in this batch
    std::vector<std::pair<uint64_t, uint64_t>> segs;          // (slot offset, len)
    std::vector<std::pair<const uint8_t *, uint64_t>> host;   // the unit's bytes in host memory
};

enum SlotState { kFree = 0, kOpen, kClosed, kSubmitted };

struct InSlot {
    IngBuf<uint8_t> host;  // page-locked, batch_cap bytes
    uint64_t used = 0;
    uint32_t open_res = 0;
    SlotState state = kFree;
    std::vector<FileEnt> files;
    Event h2d;
    bool h2d_pending = false;
    std::atomic<int> host_jobs{0};  // long-id jobs still reading this slot
    std::atomic<bool> h2d_issued{false};  // its last H2D piece and h2d are enqueued
    uint64_t close_seq = 0;
    bool has_stream = false;        // holds stream pieces: enters the pipeline in close order
    double t_first = 0;             // its first reservation (slot_max_age_ms)
    void reset(SlotState to) {      // empty again: free, or open for new reservations
        state = to;
        used = 0;
        files.clear();
        has_stream = false;
        t_first = 0;
    }
};

struct OutSlot {
    IngBuf<uint8_t> host;  // page-locked
    std::atomic<int> packs_left{0};
    bool busy = false;
};

// The end of one D2H group: `fin` is recorded after its last piece, `issued`
// set once ev_out and fin are enqueued.  Shared by the copy job (the pump
// records), the wait item (the waiter syncs) and the engine's last_d2h (the
// next pack build waits for `issued`): the last of them frees the event.
struct D2HDone {
    Event fin;
    std::atomic<bool> issued{false};
};

// A batch between stage A and stage B.
struct Batch {
    uint64_t index = 0;
    uint32_t pslot = 0;             // pipeline slot (device buffers, plan)
    InSlot *in = nullptr;
    std::vector<FileEnt> files;
    std::vector<Unit> units;
    std::vector<uint64_t> cuts;     // per unit, consecutive (relative to the unit)
    std::vector<uint32_t> ncuts;    // per unit: chunks final in this batch
    std::vector<uint64_t> c_off, c_len;  // per chunk: arena offset, length
    std::vector<const uint8_t *> c_host;  // long chunks: their bytes in host memory
    std::vector<std::vector<uint8_t>> gathers;  // long chunks split over host pieces; old carries
    std::vector<uint8_t> ids;            // 32 B per chunk
    std::vector<uint32_t> short_idx;     // chunks whose ids the device computes
    std::vector<uint64_t> seal_off, seal_len, ulen;
    std::atomic<int> long_jobs{0};
    // stage B: the open pack's blobs then this batch's new ones; the packs
    // closed (blobs [0, open_from)), laid out back to back in `total` bytes;
    // each blob's offset in its pack; the output slot and the D2H groups
    std::vector<rcdc_pack_blob> blobs;
    std::vector<std::pair<uint32_t, uint32_t>> grp;
    size_t open_from = 0;
    std::vector<rcdc_pack> packs;
    uint64_t total = 0;
    std::vector<uint32_t> boffs;
    OutSlot *out = nullptr;
    std::vector<std::pair<steps::D2HRange, std::shared_ptr<D2HDone>>> d2h;
};

// Device buffers of one pipeline slot.
struct PlanDel {
    void operator()(rcdc_plan *p) const { rcdc_plan_destroy(p); }
};
struct PSlot {
    std::unique_ptr<rcdc_plan, PlanDel> plan;
    IngBuf<uint8_t> arena;
    IngBuf<uint8_t> staging;   // sealed blobs
    IngBuf<uint64_t> d_refs;   // (off, len) of the short chunks: 2 per chunk
    IngBuf<uint64_t> h_refs;   // page-locked upload source
    IngBuf<uint8_t> d_dig;     // 32 B per chunk
    Stream s_ids;
    Event ev_ids;
    Event ev_sealed;   // stage A's device work done (s_comp)
    Event ev_retired;  // stage B done with the staging area (s_back)
    bool busy = false;  // a batch holds this slot (submit .. stage B)
};

struct PackJob {
    OutSlot *out = nullptr;
    uint64_t off = 0, size = 0, seq = 0, batch = 0;
    uint32_t header_len = 0;
    std::vector<rcdc_ingest_blob> blobs;
    uint8_t id[32];
};

// The engine's environment knobs, read by each rcdc_ingest_create.
long long env_num(const char *name, long long dflt) {
    const char *e = getenv(name);
    return e ? strtoll(e, nullptr, 10) : dflt;
}
struct Knobs {
    // the last batches whose chunks above 1 MiB the host hashes too
    size_t tail_batches = (size_t)env_num("RCDC_INGEST_TAIL_BATCHES", 2);
    // bytes of packs per D2H group
    uint64_t d2h_group = (uint64_t)env_num("RCDC_INGEST_D2H_GROUP", 256ll << 20);
    // 0: the last batches' packs go back in such groups too, not one by one
    bool tail_single = env_num("RCDC_INGEST_TAIL_SINGLE", 1) != 0;
    // pool threads that never take a pack-id job
    uint32_t id_threads = (uint32_t)env_num("RCDC_INGEST_ID_THREADS", 0);
    // 0: wait for events in hipEventSynchronize, not by polling
    bool poll = env_num("RCDC_INGEST_POLL", 1) != 0;
    // batch copies by a shader kernel on this many workgroups (0: the DMA engines)
    uint32_t kcopy = (uint32_t)std::max(env_num("RCDC_INGEST_KCOPY", 0), 0ll);
    // bytes per H2D / D2H copy, at least 1 MiB
    uint64_t copy_piece = (uint64_t)std::max(env_num("RCDC_INGEST_COPY_PIECE", 64ll << 20), 1ll << 20);
    // 1: the per-batch timeline on stderr at finish; 2: with the chunking's own ends
    int prof = getenv("RCDC_INGEST_PROF") ? (int)std::max(env_num("RCDC_INGEST_PROF", 0), 1ll) : 0;
    // k: create's k-th allocation fails (tests)
    uint32_t fail_alloc = (uint32_t)std::max(env_num("RCDC_INGEST_FAIL_ALLOC", 0), 0ll);
    // a line on stderr per regrowth
    bool alloc_log = getenv("RCDC_ALLOC_LOG") != nullptr;
};

}  // namespace

// One dedup set (the packer's ids + the index's), shareable by the engines of
// several devices: 64 shards, one lock each.
struct rcdc_index {
    static constexpr int kShards = 64;
    struct Shard {
        std::mutex mu;
        std::unordered_set<Id32, Id32Hash> set;
    };
    Shard sh[kShards];
    // true: the id was not in the set (the caller packs it)
    bool insert(const Id32 &id) {
        Shard &s = sh[id.b[31] & (kShards - 1)];
        std::lock_guard<std::mutex> lk(s.mu);
        return s.set.insert(id).second;
    }
    uint64_t size() {
        uint64_t n = 0;
        for (auto &s : sh) {
            std::lock_guard<std::mutex> lk(s.mu);
            n += s.set.size();
        }
        return n;
    }
};

struct rcdc_ingest {
    rcdc_ctx *ctx = nullptr;
    rcdc_ingest_config cfg{};
    rcdc_ingest_pack_fn pack_cb = nullptr;
    rcdc_ingest_file_fn file_cb = nullptr;
    void *user = nullptr;
    int device = 0;
    int level = 0;
    bool compress = true, verify = true;
    uint64_t batch_cap = 0, long_chunk = 0;
    Knobs knobs;
    uint32_t depth = 4, nin = 4, nout = 4, nthreads = 8;
    PackSizer sizer{};
    // input slots
    std::mutex mu;
    std::condition_variable cv_slot;    // a slot became free / a batch ready
    std::vector<std::unique_ptr<InSlot>> in;
    InSlot *open = nullptr;
    std::deque<InSlot *> ready;         // closed, all commits in: stage A order
    // device pipeline
    std::vector<PSlot> ps;
    IngBuf<uint8_t> frames;  // zstd frames, then the verify's opened frames
    IngBuf<uint8_t> d_packs;
    IngBuf<uint8_t> carry[2];
    int carry_cur = 0;
    std::vector<rcdc_pack_blob> carry_blobs;  // the open pack's blobs (src = kSrcCarry)
    Stream s_in, s_comp, s_out;
    Event ev_comp, ev_out, ev_back;  // (front / back / out)
    std::vector<std::unique_ptr<OutSlot>> outs;
    std::deque<std::unique_ptr<Batch>> submitted;  // H2D issued, stage A next (front thread)
    std::deque<std::unique_ptr<Batch>> inflight;   // stage A done, stage B next (back thread)
    bool front_done = false;                       // every batch has been through stage A
    uint64_t nclosed = 0;                          // input slots closed so far
    Stream s_back;                                 // stage B's device work
    uint64_t nbatches = 0, next_seq = 0;
    rcdc_index *idx = nullptr;  // the index's ids + the packer's (own, or shared)
    std::unique_ptr<rcdc_index> own_idx;
    // streams
    uint64_t max_chunk = 0;          // ctx max: a carry's bound
    uint64_t asm_base = 0, asm_cap = 0;  // the arena's assembly region
    IngBuf<uint8_t> carry_pool;      // max_streams device carry slots of max_chunk bytes
    std::vector<int> free_cslots;
    std::unordered_map<uint64_t, std::shared_ptr<StreamSt>> streams;  // open handles
    uint64_t next_stream = 1;
    uint32_t closing_streams = 0;    // closed, carry slot not yet released
    std::deque<InSlot *> closed_q;   // closed slots not yet ready, in close order
    double pack_t0 = 0;              // the open pack's first blob (MAX_AGE)
    double pack_max_age = 300, slot_max_age = 1;
    uint32_t nalloc = 0;  // allocations so far (knobs.fail_alloc)
    // threads
    std::thread worker, back, waiter, feeder;
    // the feeder's copy pump: batches waiting for their H2D pieces, and the
    // pack bytes' D2H groups, queued by stage B (back thread).  Whoever drops
    // a job frees its events.
    struct CopyJob {
        uint8_t *dst;
        const uint8_t *src;
        uint64_t len, done;
        InSlot *in;                    // H2D: its h2d event ends the copy
        Event after;                   // D2H: the pack build (s_back); the first piece waits on it
        std::shared_ptr<D2HDone> fin;  // D2H
    };
    std::deque<CopyJob> h2d_q;
    std::mutex d2h_mu;
    std::deque<CopyJob> d2h_q;
    std::shared_ptr<D2HDone> last_d2h;  // the last D2H group queued
    int submitting = 0;  // slots taken from `ready` whose batch is not in `submitted` yet
    std::vector<std::thread> pool;
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    std::deque<std::function<void()>> jobs;   // pack ids, in order
    std::deque<std::function<void()>> ujobs;  // long chunk ids (urgent), in order
    uint32_t running_packs = 0;               // pack-id jobs running
    std::mutex wait_mu;
    std::condition_variable wait_cv;
    struct WaitItem {
        std::shared_ptr<D2HDone> done;
        uint64_t batch;
        std::vector<std::shared_ptr<PackJob>> jobs;
    };
    std::deque<WaitItem> wait_q;
    std::mutex cb_mu;  // callbacks run one at a time
    std::atomic<bool> stop{false};
    bool finishing = false, finished = false;
    std::atomic<int> packs_pending{0};
    std::condition_variable cv_done;
    rcdc_status err = RCDC_OK;
    std::string err_msg;
    rcdc_ingest_stats st{};
    double t_first = 0;
    // knobs.prof: per batch (stage A start, sync points, end; stage B start,
    // ids wait end, end), printed by rcdc_ingest_finish
    std::vector<std::vector<double>> tl;
    std::vector<double> tl_d2h, tl_ids;  // per batch: packs landed, last pack id
};

namespace {

using Ing = rcdc_ingest;

void set_err(Ing *g, rcdc_status s, const std::string &m) {
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->err) {
        g->err = s;
        g->err_msg = m;
    }
    g->cv_slot.notify_all();
    g->cv_done.notify_all();
}

#define ING_HIP(g, expr)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            set_err(g, RCDC_ERR_INTERNAL, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
            return false;                                                                 \
        }                                                                                 \
    } while (0)
#define ING_ST(g, expr, what)                                                             \
    do {                                                                                  \
        rcdc_status s_ = (expr);                                                          \
        if (s_ != RCDC_OK) {                                                              \
            set_err(g, s_, std::string(what ": ") + rcdc_last_error());                   \
            return false;                                                                 \
        }                                                                                 \
    } while (0)

// ---- the engine's allocations (IngBuf), counted for rcdc_ingest_mem_live
std::mutex g_alloc_mu;
std::unordered_map<void *, std::pair<uint64_t, bool>> g_allocs;  // ptr -> (bytes, pinned)
uint64_t g_live_pinned = 0, g_live_dev = 0;

hipError_t ing_alloc(Ing *g, void **p, uint64_t n, bool pinned) {
    *p = nullptr;
    if (g && g->knobs.fail_alloc && ++g->nalloc == g->knobs.fail_alloc) return hipErrorOutOfMemory;
    const hipError_t e = pinned ? hipHostMalloc(p, n, hipHostMallocDefault) : hipMalloc(p, n);
    if (e != hipSuccess) {
        *p = nullptr;
        return e;
    }
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    g_allocs[*p] = {n, pinned};
    (pinned ? g_live_pinned : g_live_dev) += n;
    return hipSuccess;
}

hipError_t ing_free(void *q) {
    bool pinned = false;
    {
        std::lock_guard<std::mutex> lk(g_alloc_mu);
        auto it = g_allocs.find(q);
        if (it != g_allocs.end()) {
            pinned = it->second.second;
            (pinned ? g_live_pinned : g_live_dev) -= it->second.first;
            g_allocs.erase(it);
        }
    }
    return pinned ? hipHostFree(q) : hipFree(q);
}

template <typename T>
bool IngBuf<T>::ensure(Ing *g, uint64_t need, uint64_t grown, const char *what) {
    if (p && cap >= need) return true;
    if (g->knobs.alloc_log && p)
        fprintf(stderr, "rcdc ingest: regrow %s %llu -> %llu x %zu B (hipFree: device sync)\n", what,
                (unsigned long long)cap, (unsigned long long)need, sizeof(T));
    ING_HIP(g, release());
    ING_HIP(g, alloc(g, grown, pinned));
    return true;
}
// the device buffers' headroom: an eighth
uint64_t grow8(uint64_t need) { return need + need / 8 + 1; }

// Host SHA-256 jobs; `urgent` ones (the long chunks' ids, which gate a
// batch's stage B) go before the pack ids, in the order posted (longest
// first).  Pack-id jobs hold a thread for tens of ms (4 packs of ~40 MB), so
// knobs.id_threads threads never take one: a long-id job
// then starts at once instead of after the running pack jobs (r5z2: the last
// batches' stage B waited ~14 ms for a free thread).
void post(Ing *g, std::function<void()> fn, bool urgent = false) {
    {
        std::lock_guard<std::mutex> lk(g->pool_mu);
        (urgent ? g->ujobs : g->jobs).push_back(std::move(fn));
    }
    if (urgent) g->pool_cv.notify_all();  // (a thread free for ids may be
    else g->pool_cv.notify_one();         //  among the waiters)
}

void pool_main(Ing *g) {
    const uint32_t reserve = g->knobs.id_threads;
    const uint32_t pack_cap = g->nthreads > reserve ? g->nthreads - reserve : 1u;
    for (;;) {
        std::function<void()> fn;
        bool pack = false;
        {
            std::unique_lock<std::mutex> lk(g->pool_mu);
            g->pool_cv.wait(lk, [&] {
                return g->stop || !g->ujobs.empty() ||
                       (!g->jobs.empty() && g->running_packs < pack_cap);
            });
            if (!g->ujobs.empty()) {
                fn = std::move(g->ujobs.front());
                g->ujobs.pop_front();
            } else if (!g->jobs.empty() && g->running_packs < pack_cap) {
                fn = std::move(g->jobs.front());
                g->jobs.pop_front();
                pack = true;
                g->running_packs++;
            } else {
                return;  // stop, nothing left this thread may take
            }
        }
        fn();
        if (pack) {
            {
                std::lock_guard<std::mutex> lk(g->pool_mu);
                g->running_packs--;
            }
            g->pool_cv.notify_all();
        }
    }
}

// Wait for an event by polling (knobs.poll, default on) instead of
// hipEventSynchronize: a thread blocked in a HIP synchronisation call for a
// 60-70 ms chunk-id kernel held up the other threads' launches (r5r: each
// batch's chunking started only after the previous batch's ids were done).
hipError_t wait_event(Ing *g, hipEvent_t ev) {
    if (!g->knobs.poll) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// Hand one finished pack to the caller (pack ids are computed by then).
void deliver(Ing *g, const std::shared_ptr<PackJob> &pj) {
    rcdc_ingest_pack p{};
    p.data = pj->out->host + pj->off;
    p.size = pj->size;
    p.seq = pj->seq;
    memcpy(p.id, pj->id, 32);
    p.nblobs = (uint32_t)pj->blobs.size();
    p.header_len = pj->header_len;
    p.blobs = pj->blobs.data();
    {
        std::lock_guard<std::mutex> lk(g->cb_mu);
        if (g->pack_cb) g->pack_cb(g->user, &p);
        if (g->knobs.prof) {
            if (g->tl_ids.size() <= pj->batch) g->tl_ids.resize(pj->batch + 1, 0);
            g->tl_ids[pj->batch] = std::max(g->tl_ids[pj->batch], now_s() - g->t_first);
        }
    }
    if (--pj->out->packs_left == 0) {
        std::lock_guard<std::mutex> lk(g->mu);
        pj->out->busy = false;
        g->cv_slot.notify_all();
    }
    if (--g->packs_pending == 0) {
        std::lock_guard<std::mutex> lk(g->mu);
        g->cv_done.notify_all();
    }
}

// Host SHA-256 for pack ids and long chunk ids (RCDC_INGEST_SHA): "ni" (the
// default on CPUs with the SHA extensions) runs `ways` messages interleaved
// per call on one core; "mb" 16 per call in AVX-512 lanes.  On the box's
// cores (r5z, 32 MiB messages, profiles/r05/host_sha_rate.json) SHA-NI gives
// 2.44 / 3.51 / 3.88 / 4.30 GB/s per core at 1 / 2 / 3 / 4 ways and the
// multi-buffer form 4.73: 4 ways match the lanes' throughput at a quarter of
// their latency per message (a 40 MB pack: ~37 ms instead of ~130 ms), and
// the latency of the last batches' ids is the end of the run.
struct ShaPolicy {
    bool mb;
    int ways, ways_last;
};
const ShaPolicy &sha_policy() {
    static const ShaPolicy p = [] {
        ShaPolicy q{};
        const char *m = getenv("RCDC_INGEST_SHA");
        q.mb = host_sha_supported() && (!host_sha_ni() || (m && strcmp(m, "mb") == 0));
        const char *w = getenv("RCDC_SHANI_WAYS"), *wl = getenv("RCDC_SHANI_WAYS_LAST");
        q.ways = std::max(1, std::min(4, w ? atoi(w) : 4));
        q.ways_last = std::max(1, std::min(4, wl ? atoi(wl) : 2));
        return q;
    }();
    return p;
}

// SHA-256 of n host messages (one job's group).
void hash_group(const uint8_t *const *ptrs, const uint64_t *lens, uint32_t n, uint8_t *dig,
                bool mb) {
    if (mb)
        host_sha256_many(ptrs, lens, n, dig);
    else
        host_sha256_ni_many(ptrs, lens, n, dig, (int)n);
}

// After a batch's packs are in host memory: their ids, in groups of `ways`
// interleaved on the SHA extensions (fewer for the last batches, whose ids
// end the run), or 16 per call in AVX-512 lanes ("mb"; the last batches then
// on the SHA extensions).
void hash_packs(Ing *g, std::vector<std::shared_ptr<PackJob>> packs, bool last) {
    const ShaPolicy &pol = sha_policy();
    const bool mb = pol.mb && !last;
    const size_t per = mb ? 16 : (size_t)(last ? pol.ways_last : pol.ways);
    for (size_t a = 0; a < packs.size(); a += per) {
        std::vector<std::shared_ptr<PackJob>> grp(packs.begin() + a,
                                                  packs.begin() + std::min(a + per, packs.size()));
        post(g, [g, grp, mb] {
            std::vector<const uint8_t *> ptrs;
            std::vector<uint64_t> lens;
            std::vector<uint8_t> dig(32 * grp.size());
            for (auto &pj : grp) {
                ptrs.push_back(pj->out->host + pj->off);
                lens.push_back(pj->size);
            }
            hash_group(ptrs.data(), lens.data(), (uint32_t)grp.size(), dig.data(), mb);
            for (size_t i = 0; i < grp.size(); i++) {
                memcpy(grp[i]->id, dig.data() + 32 * i, 32);
                deliver(g, grp[i]);
            }
        });
    }
}

void waiter_main(Ing *g) {
    (void)hipSetDevice(g->device);
    for (;;) {
        Ing::WaitItem w;
        {
            std::unique_lock<std::mutex> lk(g->wait_mu);
            g->wait_cv.wait(lk, [&] { return g->stop || !g->wait_q.empty(); });
            if (g->wait_q.empty()) return;
            w = std::move(g->wait_q.front());
            g->wait_q.pop_front();
        }
        // the pump enqueues the copy's last piece and its event later; an
        // item dropped here (error, stop) lets go of its event like any other
        while (!w.done->issued.load() && !g->err && !g->stop)
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (!w.done->issued.load()) continue;
        if (wait_event(g, w.done->fin) != hipSuccess) {
            set_err(g, RCDC_ERR_INTERNAL, "pack copy-back failed");
            continue;
        }
        if (g->knobs.prof) {
            std::lock_guard<std::mutex> lk(g->cb_mu);
            if (g->tl_d2h.size() <= w.batch) g->tl_d2h.resize(w.batch + 1, 0);
            g->tl_d2h[w.batch] = now_s() - g->t_first;
        }
        bool is_last;
        {
            std::lock_guard<std::mutex> lk(g->mu);
            // the last four batches (every batch after rcdc_ingest_finish
            // was too many: throughput, r5v2; the last one alone left ~100 ms
            // of multi-buffer jobs after the last copy, r5u3).  Once the
            // caller has called finish, the batch count is known: a 16-pack
            // call takes ~115 ms, so a batch landing before the last stage A
            // (front_done) still counts as one of the last.
            is_last = g->front_done && g->inflight.size() <= 2;
            if (!is_last && g->finishing && g->ready.size() + g->nbatches <= w.batch + 4)
                is_last = true;
        }
        hash_packs(g, std::move(w.jobs), is_last);
    }
}

// ---- stage A: one closed input slot becomes a batch in flight ------------
void mark(Ing *g, uint64_t b, double t) {
    if (!g->knobs.prof) return;
    std::lock_guard<std::mutex> lk(g->cb_mu);
    if (g->tl.size() <= b) g->tl.resize(b + 1);
    g->tl[b].push_back(t - g->t_first);
}

// A ready input slot becomes a batch: a free pipeline slot, and its H2D
// enqueued at once on the copy stream (it runs while earlier batches are in
// stage A), in slot order.
bool submit_ready(Ing *g) {
    for (;;) {
        InSlot *in = nullptr;
        uint32_t ps = 0;
        std::unique_ptr<Batch> B;
        {
            std::lock_guard<std::mutex> lk(g->mu);
            if (g->ready.empty()) return true;
            for (ps = 0; ps < g->depth && g->ps[ps].busy; ps++) {
            }
            if (ps == g->depth) return true;
            in = g->ready.front();
            g->ready.pop_front();
            g->submitting++;
            g->ps[ps].busy = true;
            B = std::make_unique<Batch>();
            B->index = g->nbatches++;
            if (g->t_first == 0) g->t_first = now_s();
        }
        B->pslot = ps;
        B->in = in;
        B->files = in->files;
        mark(g, B->index, now_s());
        PSlot &P = g->ps[ps];
        const uint64_t used = in->used;
        const uint64_t need = round_up(used, 256) + 512;
        if (!P.arena.ensure(g, need, grow8(need), "arena")) return false;
        // the arena's previous batch is retired: its ids (the last reader)
        // are done.  The copy goes to the pump (feeder_main), piece by piece.
        in->h2d_issued = false;
        g->h2d_q.push_back({P.arena, in->host, used, 0, in, {}, nullptr});
        std::lock_guard<std::mutex> lk(g->mu);
        g->submitted.push_back(std::move(B));
        g->submitting--;
        g->cv_slot.notify_all();
    }
}

void reap_inputs(Ing *g);
void close_open_locked(Ing *g);

// Feeder thread: a ready input slot's H2D is enqueued as soon as a pipeline
// slot is free, whatever stage A is doing (the front thread used to enqueue
// it only between two stage A runs: each copy then started only after the
// previous batch's stage A, r5g timeline).
//
// It also pumps the H2D copies: at most two 64 MiB pieces are enqueued at a
// time.  HIP's copies go to DMA engine queues in order, and stage A's small
// uploads (plan tables, AEAD and zstd descriptors) landed behind every piece
// already queued: with a whole 2 GiB batch enqueued at once each upload
// waited ~40 ms (r5n: seal 40 ms after zstd; the next batch's stage A
// started only after the previous chunk ids).  With two pieces in flight an
// upload waits ~2.4 ms at most and the engine never idles.
//
// The D2H of the pack bytes goes the same way (small read-backs of stage A
// wait behind a whole 1 GiB pack copy otherwise: r5p, the next batch's
// chunking started only when the previous batch's packs were in host memory).
struct CopyLane {  // one direction's piece events: enqueued, and free
    std::deque<Event> inflight;
    std::vector<Event> free_ev;
    hipError_t create() {
        free_ev.resize(4);
        for (Event &e : free_ev)
            if (hipError_t r = e.create()) return r;
        return hipSuccess;
    }
};

// One pump for both directions: pieces of the front job of `q` (under `mu`,
// if it has one) go to stream `s`; `on_done` runs once a job's last piece is
// enqueued.  A job's first piece waits on its `after` event, if it has one.
template <typename Done>
bool pump(Ing *g, hipStream_t s, std::deque<Ing::CopyJob> &q, std::mutex *mu, hipMemcpyKind kind,
          CopyLane &L, Done on_done) {
    while (!L.inflight.empty() && hipEventQuery(L.inflight.front()) == hipSuccess) {
        L.free_ev.push_back(std::move(L.inflight.front()));
        L.inflight.pop_front();
    }
    std::unique_lock<std::mutex> lq;
    if (mu) lq = std::unique_lock<std::mutex>(*mu);
    while (!q.empty() && L.inflight.size() < 2 && !L.free_ev.empty()) {
        Ing::CopyJob &J = q.front();
        if (J.after) {
            ING_HIP(g, hipStreamWaitEvent(s, J.after, 0));
            J.after.reset();
        }
        const uint64_t n = std::min(g->knobs.copy_piece, J.len - J.done);
        if (n) {
            if (g->knobs.kcopy)
                ING_HIP(g, launch_stream_copy(J.dst + J.done, J.src + J.done, (n + 15) & ~15ull,
                                              g->knobs.kcopy, s));
            else
                ING_HIP(g, hipMemcpyAsync(J.dst + J.done, J.src + J.done, n, kind, s));
            ING_HIP(g, hipEventRecord(L.free_ev.back(), s));
            L.inflight.push_back(std::move(L.free_ev.back()));
            L.free_ev.pop_back();
            J.done += n;
        }
        if (J.done == J.len) {
            if (!on_done(J)) return false;
            q.pop_front();
        }
    }
    return true;
}

bool pump_h2d(Ing *g, CopyLane &L) {
    return pump(g, g->s_in, g->h2d_q, nullptr, hipMemcpyHostToDevice, L, [g](Ing::CopyJob &J) {
        ING_HIP(g, hipEventRecord(J.in->h2d, g->s_in));
        J.in->h2d_issued = true;
        std::lock_guard<std::mutex> lk(g->mu);
        g->cv_slot.notify_all();
        return true;
    });
}

bool pump_d2h(Ing *g, CopyLane &L) {
    return pump(g, g->s_out, g->d2h_q, &g->d2h_mu, hipMemcpyDeviceToHost, L, [g](Ing::CopyJob &J) {
        ING_HIP(g, hipEventRecord(g->ev_out, g->s_out));
        ING_HIP(g, hipEventRecord(J.fin->fin, g->s_out));
        J.fin->issued.store(true);
        return true;
    });
}

void feeder_main(Ing *g) {
    (void)hipSetDevice(g->device);
    CopyLane in, out;
    if (in.create() != hipSuccess || out.create() != hipSuccess) {
        set_err(g, RCDC_ERR_INTERNAL, "feeder events");
        return;
    }
    struct Drain {  // on every way out, before the lanes' events go
        Ing *g;
        ~Drain() {
            (void)hipStreamSynchronize(g->s_in);
            (void)hipStreamSynchronize(g->s_out);
        }
    } drain{g};
    for (;;) {
        reap_inputs(g);
        if (!submit_ready(g) || !pump_h2d(g, in) || !pump_d2h(g, out)) return;
        bool d2h_idle;
        {
            std::lock_guard<std::mutex> lq(g->d2h_mu);
            d2h_idle = g->d2h_q.empty();
        }
        std::unique_lock<std::mutex> lk(g->mu);
        // an open slot with files that stopped filling goes to the device
        // (a trickle of small files is not held back until finish)
        if (g->open && !g->open->files.empty() && now_s() - g->open->t_first >= g->slot_max_age)
            close_open_locked(g);
        // the back thread queues D2H jobs until the very end (finalize)
        if (g->err || (g->finished && g->h2d_q.empty() && d2h_idle)) return;
        // a piece is ~1.2 ms: poll often while copies are queued
        g->cv_slot.wait_for(lk, std::chrono::microseconds(g->h2d_q.empty() && d2h_idle ? 200 : 50));
    }
}

// The bytes [rel, rel + len) of a unit in host memory: a pointer into one of
// its host pieces, or null when they span pieces.
const uint8_t *unit_host(const Unit &u, uint64_t rel, uint64_t len) {
    uint64_t at = 0;
    for (const auto &h : u.host) {
        if (rel >= at && rel + len <= at + h.second) return h.first + (rel - at);
        at += h.second;
    }
    return nullptr;
}

void unit_gather(const Unit &u, uint64_t rel, uint64_t len, uint8_t *dst) {
    uint64_t at = 0;
    for (const auto &h : u.host) {
        const uint64_t a = std::max(rel, at), e = std::min(rel + len, at + h.second);
        if (a < e) memcpy(dst + (a - rel), h.first + (a - at), e - a);
        at += h.second;
    }
}

// The batch's plan streams: whole files in place; per stream, its carry and
// its pieces of this batch, in place when that is one contiguous piece and
// no carry, else gathered into the assembly region (copies appended to cr).
bool build_units(Ing *g, Batch *B, std::vector<rcdc_copy_ref> &cr, uint64_t *asm_used) {
    InSlot *in = B->in;
    std::unordered_map<StreamSt *, size_t> unit_of;
    for (const FileEnt &f : B->files) {
        if (f.cancelled) continue;
        if (!f.st) {
            Unit u;
            u.tag = f.tag;
            u.off = f.off;
            u.len = u.fresh = f.len;
            u.segs.push_back({f.off, f.len});
            B->units.push_back(std::move(u));
            continue;
        }
        auto it = unit_of.find(f.st.get());
        if (it == unit_of.end()) {
            Unit u;
            u.st = f.st;
            u.tag = f.st->tag;
            u.final = false;
            u.base = f.st->base;
            u.carry = f.st->carry_len;
            it = unit_of.emplace(f.st.get(), B->units.size()).first;
            B->units.push_back(std::move(u));
        }
        Unit &u = B->units[it->second];
        if (f.final) {
            u.final = true;
            u.aborted = f.st->aborted;
        }
        if (!f.len) continue;
        if (!u.segs.empty() && u.segs.back().first + u.segs.back().second == f.off)
            u.segs.back().second += f.len;  // laid out back to back (stream_reserve)
        else
            u.segs.push_back({f.off, f.len});
        u.fresh += f.len;
    }
    uint64_t ao = 0;
    for (Unit &u : B->units) {
        if (!u.st) {
            u.host.push_back({in->host + u.off, u.len});
            continue;
        }
        u.len = u.carry + u.fresh;
        if (!u.carry && u.segs.size() <= 1) {  // in place
            u.off = u.segs.empty() ? 0 : u.segs[0].first;
            if (u.fresh) u.host.push_back({in->host + u.off, u.fresh});
            continue;
        }
        u.off = g->asm_base + ao;
        uint64_t o = u.off;
        if (u.carry) {
            rcdc_copy_ref c{};
            c.in_off = (uint64_t)u.st->cslot * g->max_chunk;
            c.out_off = o;
            c.len = u.carry;
            c.src = 1;
            cr.push_back(c);
            u.host.push_back({u.st->hcarry.data(), u.carry});
            o += u.carry;
        }
        for (const auto &sg : u.segs) {
            rcdc_copy_ref c{};
            c.in_off = sg.first;
            c.out_off = o;
            c.len = sg.second;
            c.src = 0;
            cr.push_back(c);
            u.host.push_back({in->host + sg.first, sg.second});
            o += sg.second;
        }
        ao = round_up(ao + u.len, 256);
        if (ao > g->asm_cap) {
            set_err(g, RCDC_ERR_INTERNAL, "ingest: assembly region overflow");
            return false;
        }
    }
    *asm_used = ao;
    return true;
}

// ---- stage A, step by step (stage_a below runs them in this order) ---------

// 1. The H2D (the feeder's pump) lands before the chunking: wait until its
// event is enqueued, then order the compute stream after it.
bool a_wait_h2d(Ing *g, Batch *B) {
    InSlot *in = B->in;
    {
        std::unique_lock<std::mutex> lk(g->mu);
        while (!in->h2d_issued && !g->err) g->cv_slot.wait_for(lk, std::chrono::microseconds(100));
        if (g->err) return false;
    }
    ING_HIP(g, hipStreamWaitEvent(g->s_comp, in->h2d, 0));
    if (g->knobs.prof > 1) mark(g, B->index, now_s());
    return true;
}

// 2. The plan streams; streams' carries and scattered pieces gathered.
// *arena_len: the arena bytes the plan covers.
bool a_gather_units(Ing *g, Batch *B, PSlot &P, uint64_t *arena_len) {
    std::vector<rcdc_copy_ref> gcr;
    uint64_t asm_used = 0;
    if (!build_units(g, B, gcr, &asm_used)) return false;
    if (!gcr.empty()) {
        const void *gsrc[2] = {P.arena, g->carry_pool};
        ING_ST(g, rcdc_copy_ranges(g->ctx, gsrc, 2, gcr.data(), (uint32_t)gcr.size(), P.arena,
                                   g->s_comp),
               "stream gather");
    }
    *arena_len = std::max(round_up(B->in->used, 256) + 256,
                          asm_used ? g->asm_base + asm_used + 256 : 0);
    return true;
}

// 3. Chunk: the slot's plan laid out for the units and run; `cuts` are
// relative to each unit, counts[i] of them per unit, consecutive.
bool a_chunk(Ing *g, Batch *B, PSlot &P, uint64_t arena_len, std::vector<uint64_t> &cuts,
             std::vector<uint64_t> &counts) {
    const uint32_t nf = (uint32_t)B->units.size();
    std::vector<uint64_t> offs(nf), lens(nf);
    uint64_t ubytes = 0;
    for (uint32_t i = 0; i < nf; i++) {
        offs[i] = B->units[i].off;
        lens[i] = B->units[i].len;
        ubytes += lens[i];
    }
    if (!P.plan) {
        rcdc_plan *pl = nullptr;
        ING_ST(g, rcdc_plan_create(g->ctx, offs.data(), lens.data(), nf, arena_len, &pl), "plan");
        P.plan.reset(pl);
    } else {
        ING_ST(g, plan_relayout(P.plan.get(), offs.data(), lens.data(), nf, arena_len, g->s_comp),
               "plan");
    }
    if (g->knobs.prof > 1) mark(g, B->index, now_s());
    ING_ST(g, rcdc_plan_run(P.plan.get(), P.arena, g->s_comp), "chunk");
    if (g->knobs.prof > 1) {  // (RCDC_INGEST_PROF=2: the H2D's and the chunking's own ends)
        (void)hipEventSynchronize(B->in->h2d);
        mark(g, B->index, now_s());
    }
    const uint64_t cap = (uint64_t)nf + ubytes / 4096 + 16;  // min >= 4096 (rcdc_check_params)
    cuts.assign(std::max<uint64_t>(cap, 1), 0);
    counts.assign(std::max<uint32_t>(nf, 1), 0);
    rcdc_status rs = rcdc_plan_results(P.plan.get(), cuts.data(), cuts.size(), counts.data());
    if (rs == RCDC_ERR_CAPACITY) {
        uint64_t tot = 0;
        for (uint32_t i = 0; i < nf; i++) tot += counts[i];
        cuts.resize(tot);
        rs = rcdc_plan_results(P.plan.get(), cuts.data(), cuts.size(), counts.data());
    }
    ING_ST(g, rs, "chunk results");
    mark(g, B->index, now_s());
    return true;
}

// 4. Cut lists (steps::cut_lists): the chunks final in this batch go into B;
// returned with the streams' new carries and their device copies.
steps::CutLists a_cut_lists(Ing *g, Batch *B, const std::vector<uint64_t> &cuts,
                            const std::vector<uint64_t> &counts) {
    std::vector<steps::UnitView> uv;
    for (const Unit &u : B->units)
        uv.push_back({u.st != nullptr, u.final, u.aborted, u.off, u.len, u.st ? u.st->cslot : 0});
    steps::CutLists L = steps::cut_lists(uv, counts.data(), cuts.data(), g->max_chunk);
    B->cuts = std::move(L.cuts);
    B->ncuts = std::move(L.ncuts);
    B->c_off = std::move(L.c_off);
    B->c_len = std::move(L.c_len);
    B->ids.assign(B->c_off.size() * 32, 0);
    return L;
}

// 5. ids: short chunks on the device (own stream per pipeline slot), long
// ones on host threads from the input slot.
// 5a. The split.  The last batches' ids bound the run's end: a batch's
// longest device chain (~34 MB/s per lane: 62 ms for a 2 MiB chunk) holds its
// stage B, and stage B runs in batch order, so the host takes the chunks above
// 1 MiB of the last knobs.tail_batches (default 2) batches too and both sides
// end together (~30 ms).  (The last batch alone: the one before it still
// waited ~40 ms for its device ids, r5y.)
void a_split_ids(Ing *g, Batch *B, std::vector<uint32_t> &long_idx) {
    const uint64_t nchunks = B->c_off.size();
    bool tail;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        const size_t after = g->ready.size() + g->submitted.size() + (size_t)g->submitting +
                             (g->open != nullptr ? 1 : 0);
        tail = g->finishing && after < g->knobs.tail_batches;
    }
    const uint64_t long_thr = tail ? std::min<uint64_t>(g->long_chunk, 1ull << 20) : g->long_chunk;
    for (uint64_t k = 0; k < nchunks; k++)
        (B->c_len[k] > long_thr ? long_idx : B->short_idx).push_back((uint32_t)k);
    // the long chunks' host bytes: in place, or gathered from a stream's
    // host pieces (a chunk that starts in the carry) before the carries move
    B->c_host.assign(nchunks, nullptr);
    if (long_idx.empty()) return;
    std::vector<uint32_t> unit_of(nchunks);
    for (uint32_t i = 0, k = 0; i < B->units.size(); i++)
        for (uint32_t j = 0; j < B->ncuts[i]; j++) unit_of[k++] = i;
    for (uint32_t k : long_idx) {
        const Unit &u = B->units[unit_of[k]];
        const uint64_t rel = B->c_off[k] - u.off;
        B->c_host[k] = unit_host(u, rel, B->c_len[k]);
        if (!B->c_host[k]) {
            B->gathers.emplace_back(B->c_len[k]);
            unit_gather(u, rel, B->c_len[k], B->gathers.back().data());
            B->c_host[k] = B->gathers.back().data();
        }
    }
}

// 5b. The streams' new carries (device: one copy; host: their bytes), and
// the carry slots of streams that ended.
bool a_move_carries(Ing *g, Batch *B, PSlot &P, const steps::CutLists &L) {
    if (!L.copies.empty()) {
        const void *csrc[1] = {P.arena};
        ING_ST(g, rcdc_copy_ranges(g->ctx, csrc, 1, L.copies.data(), (uint32_t)L.copies.size(),
                                   g->carry_pool, g->s_comp),
               "stream carry");
    }
    // A long chunk's host bytes may lie inside the old carry (c_host points
    // into it: a chunk of exactly max bytes that ended a batch's unit is
    // the next batch's carry, whole): the old carries stay with the batch
    // until its host id jobs are done (stage B runs after them)
    for (const auto &c : L.carries) {
        Unit &u = B->units[c.first];
        StreamSt &st = *u.st;
        std::vector<uint8_t> h(u.len - c.second);
        if (!h.empty()) unit_gather(u, c.second, h.size(), h.data());
        B->gathers.push_back(std::move(st.hcarry));
        st.hcarry = std::move(h);
        st.base = u.base + c.second;
        st.carry_len = u.len - c.second;
    }
    std::lock_guard<std::mutex> lk(g->mu);
    for (Unit &u : B->units)
        if (u.st && u.final && u.st->cslot >= 0) {
            g->free_cslots.push_back(u.st->cslot);
            u.st->cslot = -1;
            B->gathers.push_back(std::move(u.st->hcarry));
            u.st->hcarry = std::vector<uint8_t>();
            g->closing_streams--;
        }
    g->cv_slot.notify_all();
    return true;
}

// 5c. The short chunks' refs (longest first) up, and their ids on s_ids
// after the compute stream's work so far.
bool a_device_ids(Ing *g, Batch *B, PSlot &P) {
    std::sort(B->short_idx.begin(), B->short_idx.end(),
              [&](uint32_t a, uint32_t b) { return B->c_len[a] > B->c_len[b]; });
    const uint64_t ns = B->short_idx.size(), grown = ns + ns / 4 + 64;  // the refs' headroom: a quarter
    if (!P.h_refs.ensure(g, 2 * ns, 2 * grown, "refs (host)") ||
        !P.d_refs.ensure(g, 2 * ns, 2 * grown, "refs") ||
        !P.d_dig.ensure(g, 32 * ns, 32 * grown, "digests"))
        return false;
    for (uint64_t j = 0; j < ns; j++) {
        P.h_refs[2 * j] = B->c_off[B->short_idx[j]];
        P.h_refs[2 * j + 1] = B->c_len[B->short_idx[j]];
    }
    ING_HIP(g, hipEventRecord(g->ev_comp, g->s_comp));
    ING_HIP(g, hipStreamWaitEvent(P.s_ids, g->ev_comp, 0));
    if (ns) {
        ING_HIP(g, hipMemcpyAsync(P.d_refs, P.h_refs, ns * 16, hipMemcpyHostToDevice, P.s_ids));
        ING_ST(g, rcdc_sha256_chunks(g->ctx, P.arena, (const rcdc_chunk_ref *)P.d_refs.p,
                                     (uint32_t)ns, P.d_dig, P.s_ids),
               "chunk ids");
    }
    ING_HIP(g, hipEventRecord(P.ev_ids, P.s_ids));
    return true;
}

// 5d. Long ids: groups of similar lengths (longest first), `ways` per call on
// the SHA extensions or 16 per multi-buffer call (sha_policy).  From here the
// input slot is freed once its H2D and these jobs are done.
void a_host_ids(Ing *g, Batch *bp, std::vector<uint32_t> &long_idx) {
    InSlot *in = bp->in;
    std::sort(long_idx.begin(), long_idx.end(),
              [&](uint32_t a, uint32_t b) { return bp->c_len[a] > bp->c_len[b]; });
    const bool mb = sha_policy().mb;
    const size_t per = mb ? 16 : (size_t)sha_policy().ways;
    for (size_t a = 0; a < long_idx.size(); a += per) {
        std::vector<uint32_t> grp(long_idx.begin() + a,
                                  long_idx.begin() + std::min(a + per, long_idx.size()));
        bp->long_jobs++;
        in->host_jobs++;
        post(g, [g, bp, in, grp, mb] {
            std::vector<const uint8_t *> ptrs;
            std::vector<uint64_t> ls;
            std::vector<uint8_t> dig(32 * grp.size());
            for (uint32_t k : grp) {
                ptrs.push_back(bp->c_host[k]);
                ls.push_back(bp->c_len[k]);
            }
            hash_group(ptrs.data(), ls.data(), (uint32_t)grp.size(), dig.data(), mb);
            for (size_t i = 0; i < grp.size(); i++)
                memcpy(bp->ids.data() + 32ull * grp[i], dig.data() + 32 * i, 32);
            in->host_jobs--;
            bp->long_jobs--;
            std::lock_guard<std::mutex> lk(g->mu);
            g->cv_slot.notify_all();
        }, true);
    }
    std::lock_guard<std::mutex> lk(g->mu);
    in->h2d_pending = true;
    in->state = kSubmitted;
}

// 6a. Every chunk: zstd (version 2), sealed into the staging area once its
// previous batch has been packed.  src_len: the bytes sealed per chunk (its
// frame, or the chunk as it is).
bool a_seal(Ing *g, Batch *B, PSlot &P, std::vector<uint64_t> &src_len) {
    const uint64_t nchunks = B->c_off.size();
    std::vector<uint64_t> src_off(nchunks);
    src_len.assign(nchunks, 0);
    const uint8_t *src = P.arena;
    B->ulen.assign(nchunks, 0);
    if (g->compress && nchunks) {
        uint64_t fo = 0;
        std::vector<rcdc_zstd_ref> zr(nchunks);
        for (uint64_t k = 0; k < nchunks; k++) {
            zr[k].in_off = B->c_off[k];
            zr[k].len = B->c_len[k];
            zr[k].out_off = fo;
            src_off[k] = fo;
            fo = round_up(fo + rcdc_zstd_bound(B->c_len[k]) + 48, 16);
        }
        if (!g->frames.ensure(g, fo + 64, grow8(fo + 64), "frames")) return false;
        ING_ST(g, rcdc_zstd_compress(g->ctx, g->level, P.arena, zr.data(), (uint32_t)nchunks,
                                     g->frames, src_len.data(), g->s_comp),
               "zstd");
        src = g->frames;
        for (uint64_t k = 0; k < nchunks; k++) B->ulen[k] = B->c_len[k];
        mark(g, B->index, now_s());
    } else {
        for (uint64_t k = 0; k < nchunks; k++) {
            src_off[k] = B->c_off[k];
            src_len[k] = B->c_len[k];
        }
    }
    B->seal_off.resize(nchunks);
    B->seal_len.resize(nchunks);
    std::vector<rcdc_aead_ref> ar(nchunks);
    uint64_t so = 0;
    for (uint64_t k = 0; k < nchunks; k++) {
        ar[k].in_off = src_off[k];
        ar[k].len = src_len[k];
        ar[k].out_off = so;
        B->seal_off[k] = so;
        B->seal_len[k] = src_len[k] + 32;
        so = round_up(so + src_len[k] + 64, 16);
    }
    if (nchunks) {
        std::vector<uint8_t> nonces(16 * nchunks);
        random_bytes(nonces.data(), nonces.size());
        for (uint64_t k = 0; k < nchunks; k++) memcpy(ar[k].nonce, nonces.data() + 16 * k, 16);
    }
    if (!P.staging.ensure(g, so + 64, grow8(so + 64), "staging")) return false;
    // the staging area's previous batch has been packed (stage B, s_back)
    ING_HIP(g, hipStreamWaitEvent(g->s_comp, P.ev_retired, 0));
    if (nchunks)
        ING_ST(g, rcdc_aead_seal(g->ctx, g->cfg.key, src, ar.data(), (uint32_t)nchunks, P.staging,
                                 g->s_comp),
               "seal");
    return true;
}

// 6b. verify_data (decrypt.rs:508-529): open (MAC) into the frames buffer,
// decode, compare with the chunk in place.
bool a_verify(Ing *g, Batch *B, PSlot &P, const std::vector<uint64_t> &src_len) {
    const uint64_t nchunks = B->c_off.size();
    std::vector<rcdc_aead_ref> orf(nchunks);
    std::vector<rcdc_zstd_check_ref> cr(nchunks);
    uint64_t po = 0;
    for (uint64_t k = 0; k < nchunks; k++) {
        orf[k].in_off = B->seal_off[k];
        orf[k].len = B->seal_len[k];
        orf[k].out_off = po;
        cr[k].frame_off = po;
        cr[k].frame_len = src_len[k];
        cr[k].data_off = B->c_off[k];
        cr[k].data_len = B->c_len[k];
        po = round_up(po + src_len[k] + 16, 16);
    }
    if (!g->compress && !g->frames.ensure(g, po + 64, grow8(po + 64), "frames")) return false;
    std::vector<uint32_t> stat(nchunks, 0);
    ING_ST(g, rcdc_aead_open(g->ctx, g->cfg.key, P.staging, orf.data(), (uint32_t)nchunks,
                             g->frames, stat.data(), g->s_comp),
           "verify open");
    for (uint64_t k = 0; k < nchunks; k++)
        if (stat[k]) {
            set_err(g, RCDC_ERR_VERIFICATION, "Verifying data failed (MAC)");
            return false;
        }
    ING_ST(g, rcdc_zstd_check(g->ctx, g->frames, P.arena, cr.data(), (uint32_t)nchunks,
                              g->compress ? 0u : RCDC_CHECK_STORED, stat.data(), g->s_comp),
           "verify check");
    for (uint64_t k = 0; k < nchunks; k++)
        if (stat[k]) {
            set_err(g, RCDC_ERR_VERIFICATION,
                    "Verifying compressed data failed (extra_verify, decrypt.rs:516-526)");
            return false;
        }
    return true;
}

// 7. Stats: bytes and files new in this batch (a stream counts at its end).
void a_stats(Ing *g, Batch *B) {
    uint64_t bytes = 0, nfiles = 0;
    for (const Unit &u : B->units) {
        bytes += u.fresh;
        nfiles += !u.st || (u.final && !u.aborted);
    }
    std::lock_guard<std::mutex> lk(g->mu);
    g->st.bytes_in += bytes;
    g->st.files += nfiles;
    g->st.chunks += B->c_off.size();
    g->st.batches++;
}

bool stage_a(Ing *g, Batch *B) {
    PSlot &P = g->ps[B->pslot];
    uint64_t arena_len = 0;
    std::vector<uint64_t> cuts, counts, src_len;
    std::vector<uint32_t> long_idx;
    if (!a_wait_h2d(g, B)) return false;                                // 1
    if (!a_gather_units(g, B, P, &arena_len)) return false;             // 2
    if (!a_chunk(g, B, P, arena_len, cuts, counts)) return false;       // 3
    const steps::CutLists L = a_cut_lists(g, B, cuts, counts);          // 4
    a_split_ids(g, B, long_idx);                                        // 5
    if (!a_move_carries(g, B, P, L)) return false;
    if (!a_device_ids(g, B, P)) return false;
    a_host_ids(g, B, long_idx);
    if (!a_seal(g, B, P, src_len)) return false;                  // 6
    if (g->verify && !B->c_off.empty() && !a_verify(g, B, P, src_len)) return false;
    ING_HIP(g, hipEventRecord(P.ev_sealed, g->s_comp));
    mark(g, B->index, now_s());
    a_stats(g, B);                                                      // 7
    return true;
}

// ---- stage B: dedup, per-file results, packs ------------------------------
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // stage B with no batch: close the open pack

// The stage B steps (stage_b below runs them in this order).

// 1. The batch's ids: the device's read back into place beside the host's.
bool b_read_ids(Ing *g, Batch *B, PSlot &P) {
    const uint64_t ns = B->short_idx.size();
    if (!ns) return true;
    std::vector<uint8_t> dig(ns * 32);
    // on the ids' own stream (not the legacy default stream's queue)
    ING_HIP(g, hipMemcpyAsync(dig.data(), P.d_dig, ns * 32, hipMemcpyDeviceToHost, P.s_ids));
    ING_HIP(g, hipEventRecord(P.ev_ids, P.s_ids));
    ING_HIP(g, wait_event(g, P.ev_ids));
    for (uint64_t j = 0; j < ns; j++)
        memcpy(B->ids.data() + 32ull * B->short_idx[j], dig.data() + 32 * j, 32);
    return true;
}

// 2. Packer::add (packer.rs:304-315): the first occurrence of an id the
// index does not have is added, in chunk order -- to B->blobs, after the open
// pack's blobs.  Returns the number added.
size_t b_dedup(Ing *g, Batch *B, std::vector<uint8_t> &is_new) {
    const uint64_t n = B->c_len.size();
    is_new.assign(n, 0);
    B->blobs = g->carry_blobs;
    B->blobs.reserve(B->blobs.size() + n);
    for (uint64_t k = 0; k < n; k++) {
        Id32 id;
        memcpy(id.b, B->ids.data() + 32 * k, 32);
        if (!g->idx->insert(id)) continue;
        is_new[k] = 1;
        rcdc_pack_blob b{};
        b.in_off = B->seal_off[k];
        b.len = (uint32_t)B->seal_len[k];
        b.uncompressed_len = (uint32_t)B->ulen[k];
        b.type = 0;
        b.pad = kSrcStaging;
        memcpy(b.id, id.b, 32);
        B->blobs.push_back(b);
    }
    return B->blobs.size() - g->carry_blobs.size();
}

// 3. Per-file results (the tree's content lists, file_archiver.rs:144-168):
// a whole file at once; a stream's chunks accumulate until its end.
void b_file_results(Ing *g, Batch *B, const std::vector<uint8_t> &is_new) {
    uint64_t k = 0;
    for (size_t i = 0; i < B->units.size(); i++) {
        const Unit &u = B->units[i];
        const uint32_t ne = B->ncuts[i];
        uint32_t nnew = 0;
        for (uint32_t j = 0; j < ne; j++) nnew += is_new[k + j];
        rcdc_ingest_file_result fr{};
        bool deliver_file = false;
        if (!u.st) {
            fr.tag = u.tag;
            fr.len = u.len;
            fr.nchunks = ne;
            fr.nnew = nnew;
            fr.cuts = B->cuts.data() + k;
            fr.ids = B->ids.data() + 32 * k;
            deliver_file = true;
        } else {
            StreamSt &st = *u.st;
            for (uint32_t j = 0; j < ne; j++) st.cuts.push_back(u.base + B->cuts[k + j]);
            st.ids.insert(st.ids.end(), B->ids.begin() + 32 * k, B->ids.begin() + 32 * (k + ne));
            st.nnew += nnew;
            if (u.final && !u.aborted) {
                fr.tag = st.tag;
                fr.len = u.base + u.len;  // the stream's length (its last cut)
                fr.nchunks = (uint32_t)st.cuts.size();
                fr.nnew = st.nnew;
                fr.cuts = st.cuts.data();
                fr.ids = st.ids.data();
                deliver_file = true;
            }
        }
        k += ne;
        if (deliver_file && g->file_cb) {
            std::lock_guard<std::mutex> lk(g->cb_mu);
            g->file_cb(g->user, &fr);
        }
        if (u.st && u.final) {
            std::vector<uint64_t>().swap(u.st->cuts);
            std::vector<uint8_t>().swap(u.st->ids);
        }
    }
}

// The sources of the pack build and of the open pack's copy: [kSrcStaging]
// the slot's staging area, [kSrcCarry] the current carry buffer (the carry
// for both when there is no batch).
void pack_sources(Ing *g, const Batch *B, const void *srcs[2]) {
    const bool has_slot = B->pslot != kNoSlot;
    const void *staging = g->ps[has_slot ? B->pslot : 0].staging;
    const void *cur_carry = g->carry[g->carry_cur];
    srcs[0] = has_slot ? staging : cur_carry;
    srcs[1] = cur_carry ? cur_carry : staging;
}

// 6a. The closed packs built in d_packs.
bool b_build_packs(Ing *g, Batch *B) {
    // the last pack build's D2H must be done with d_packs: once the pump
    // has enqueued its last piece, ev_out marks its end
    if (g->last_d2h)
        while (!g->last_d2h->issued.load() && !g->err)
            std::this_thread::sleep_for(std::chrono::microseconds(50));
    if (g->err) return false;
    if (g->d_packs.cap < B->total + 64) {
        // a regrow frees d_packs: every D2H piece reading it must have
        // run, not only been enqueued (hipFree waits for queued work, but
        // the pump enqueues pieces one by one)
        ING_HIP(g, wait_event(g, g->ev_out));
        if (!g->d_packs.ensure(g, B->total + 64, grow8(B->total + 64), "packs")) return false;
    }
    ING_HIP(g, hipStreamWaitEvent(g->s_back, g->ev_out, 0));
    const void *srcs[2];
    pack_sources(g, B, srcs);
    B->boffs.assign(std::max<size_t>(B->open_from, 1), 0);
    ING_ST(g, rcdc_pack_build_raw_multi(g->ctx, g->cfg.key, srcs, 2, B->blobs.data(),
                                        (uint32_t)B->open_from, B->packs.data(),
                                        (uint32_t)B->packs.size(), g->d_packs, B->total,
                                        B->boffs.data(), g->s_back),
           "pack build");
    return true;
}

// 6b. A free page-locked output slot, and the D2H to it queued for the
// feeder's pump, piece by piece, after the build (the first group's job
// orders the copy stream after it; the rest follow on that stream).
// The packs go back in groups of whole packs of ~256 MiB, each with its
// own end event: a group's pack ids start as soon as it has landed, not
// after the batch's whole D2H (~20 ms for a 2 GiB batch's ~1 GB of packs;
// the last batch's ids end the run).
bool b_queue_d2h(Ing *g, Batch *B, bool finalize) {
    OutSlot *out = nullptr;
    {
        std::unique_lock<std::mutex> lk(g->mu);
        for (;;) {
            for (auto &o : g->outs)
                if (!o->busy) {
                    out = o.get();
                    break;
                }
            if (out || g->err) break;
            g->cv_slot.wait_for(lk, std::chrono::milliseconds(2));
        }
        if (!out) return false;
        out->busy = true;
    }
    B->out = out;
    if (!out->host.ensure(g, B->total, B->total + B->total / 4, "out slot")) return false;
    Event after;
    ING_HIP(g, after.create());
    ING_HIP(g, hipEventRecord(after, g->s_back));
    // The last two batches' packs go back one pack per group: each pack's
    // id starts as soon as that pack has landed.  Their ids are the end of
    // the run, and in groups of ~256 MiB the last group's packs were
    // still being hashed ~43 ms after the last copy (r6i timeline, 16
    // files: landed 385 ms, last id 429 ms).
    bool tail_b;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        tail_b = finalize || (g->finishing && g->front_done && g->inflight.size() <= 1);
    }
    const uint64_t group_bytes = g->knobs.tail_single && tail_b ? 1 : g->knobs.d2h_group;
    for (const steps::D2HRange &r :
         steps::d2h_ranges(B->packs.data(), B->packs.size(), B->total, group_bytes)) {
        auto done = std::make_shared<D2HDone>();
        ING_HIP(g, done->fin.create());
        {
            std::lock_guard<std::mutex> lq(g->d2h_mu);
            g->d2h_q.push_back({out->host + r.lo, g->d_packs + r.lo, r.hi - r.lo, 0, nullptr,
                                r.first == 0 ? std::move(after) : Event(), done});
        }
        g->last_d2h = done;
        B->d2h.push_back({r, done});
    }
    g->cv_slot.notify_all();
    return true;
}

// 7. The still open pack: its blobs into the other carry buffer.  Its age
// runs from its first blob (a pack that starts in this batch is new; one
// carried on keeps its time).
bool b_carry_open_pack(Ing *g, Batch *B, bool carried, double tnow) {
    std::vector<rcdc_pack_blob> rest(B->blobs.begin() + B->open_from, B->blobs.end());
    if (!rest.empty()) {
        const int nx = g->carry_cur ^ 1;
        std::vector<rcdc_copy_ref> cr(rest.size());
        uint64_t o = 0;
        for (size_t i = 0; i < rest.size(); i++) {
            cr[i].in_off = rest[i].in_off;
            cr[i].out_off = o;
            cr[i].len = rest[i].len;
            cr[i].src = rest[i].pad;
            rest[i].in_off = o;
            rest[i].pad = kSrcCarry;
            o = round_up(o + rest[i].len, 16);
        }
        if (!g->carry[nx].ensure(g, o + 64, grow8(o + 64), "carry")) return false;
        const void *srcs[2];
        pack_sources(g, B, srcs);
        ING_ST(g, rcdc_copy_ranges(g->ctx, srcs, 2, cr.data(), (uint32_t)cr.size(), g->carry[nx],
                                   g->s_back),
               "carry");
        g->carry_cur = nx;
    }
    if (!rest.empty() && (B->open_from > 0 || !carried)) g->pack_t0 = tnow;
    g->carry_blobs = std::move(rest);
    return true;
}

// 8. The packs' jobs: one wait item per D2H group for the waiter, which
// hands the group's packs to the pool once they have landed.
void b_post_packs(Ing *g, Batch *B) {
    std::vector<std::shared_ptr<PackJob>> jobs;
    for (size_t j = 0; j < B->grp.size(); j++) {
        auto pj = std::make_shared<PackJob>();
        pj->out = B->out;
        pj->off = B->packs[j].out_off;
        pj->size = B->packs[j].size;
        pj->header_len = B->packs[j].header_len;
        pj->seq = g->next_seq++;
        pj->batch = B->index;
        for (uint32_t i = B->grp[j].first; i < B->grp[j].first + B->grp[j].second; i++) {
            rcdc_ingest_blob e{};
            memcpy(e.id, B->blobs[i].id, 32);
            e.offset = B->boffs[i];
            e.length = B->blobs[i].len;
            e.uncompressed_length = B->blobs[i].uncompressed_len;
            e.type = B->blobs[i].type;
            pj->blobs.push_back(e);
        }
        jobs.push_back(pj);
    }
    B->out->packs_left += (int)jobs.size();
    g->packs_pending += (int)jobs.size();
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->st.packs += jobs.size();
        g->st.pack_bytes += B->total;
    }
    {
        std::lock_guard<std::mutex> lk(g->wait_mu);
        for (auto &d : B->d2h)
            g->wait_q.push_back({d.second, B->index,
                                 std::vector<std::shared_ptr<PackJob>>(
                                     jobs.begin() + d.first.first, jobs.begin() + d.first.last)});
    }
    g->wait_cv.notify_one();
}

bool stage_b(Ing *g, Batch *B, bool finalize) {
    const bool has_slot = B->pslot != kNoSlot;
    PSlot &P = g->ps[has_slot ? B->pslot : 0];
    mark(g, B->index, now_s());
    if (has_slot) {                                                     // 1
        ING_HIP(g, wait_event(g, P.ev_ids));
        ING_HIP(g, hipStreamWaitEvent(g->s_back, P.ev_sealed, 0));
    }
    mark(g, B->index, now_s());
    if (!b_read_ids(g, B, P)) return false;
    std::vector<uint8_t> is_new;
    const size_t nnew = b_dedup(g, B, is_new);                          // 2
    b_file_results(g, B, is_new);                                       // 3
    // 4. should_save pack by pack over the open pack's blobs and the new
    // ones (steps::group_packs), and by age (MAX_AGE, packer.rs:63,668-670):
    // the open pack carried in from earlier batches is saved once its first
    // blob is pack_max_age old
    const double tnow = now_s();
    const bool carried = !g->carry_blobs.empty();
    const bool aged = carried && tnow - g->pack_t0 >= g->pack_max_age;
    B->grp = steps::group_packs(B->blobs.data(), B->blobs.size(), g->sizer, finalize, aged,
                                &B->open_from);
    // 5. the packs' places in the pack buffer, and their header nonces
    B->packs.assign(B->grp.size(), rcdc_pack{});
    B->total = steps::layout_packs(B->blobs.data(), B->grp, B->packs.data());
    std::vector<uint8_t> hn(16 * B->grp.size());
    random_bytes(hn.data(), hn.size());
    for (size_t j = 0; j < B->grp.size(); j++) memcpy(B->packs[j].header_nonce, hn.data() + 16 * j, 16);
    if (!B->grp.empty() && (!b_build_packs(g, B) || !b_queue_d2h(g, B, finalize))) return false;  // 6
    if (!b_carry_open_pack(g, B, carried, tnow)) return false;          // 7
    if (!B->grp.empty()) b_post_packs(g, B);                            // 8
    if (has_slot) ING_HIP(g, hipEventRecord(P.ev_retired, g->s_back));
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->st.new_blobs += nnew;
    }
    mark(g, B->index, now_s());
    return true;
}

// Stage B with no batch: the open pack is closed on its own (MAX_AGE with no
// batch coming, or Packer::finalize with nothing else left).
bool close_open_pack(Ing *g) {
    Batch empty;
    empty.pslot = kNoSlot;
    empty.index = g->nbatches;
    return stage_b(g, &empty, true);
}

// The input slot of a batch is free again once its H2D has landed and the
// host long-id jobs have read it.
void reap_inputs(Ing *g) {
    std::lock_guard<std::mutex> lk(g->mu);
    for (auto &s : g->in)
        if (s->state == kSubmitted && s->host_jobs == 0 &&
            (!s->h2d_pending || hipEventQuery(s->h2d) == hipSuccess)) {
            s->h2d_pending = false;
            s->reset(kFree);
            g->cv_slot.notify_all();
        }
}

// Front thread: the copies in (submit_ready) and stage A, in batch order.
void worker_main(Ing *g) {
    (void)hipSetDevice(g->device);
    for (;;) {
        std::unique_ptr<Batch> B;
        bool done = false;
        {
            std::unique_lock<std::mutex> lk(g->mu);
            if (g->err) {
                g->cv_done.notify_all();
                return;
            }
            if (!g->submitted.empty()) {
                B = std::move(g->submitted.front());
                g->submitted.pop_front();
            } else {
                // closed slots whose files are not all in wait in closed_q
                done = g->finishing && g->ready.empty() && g->open == nullptr &&
                       g->closed_q.empty() && g->submitting == 0;
            }
        }
        if (B) {
            if (!stage_a(g, B.get())) return;
            std::lock_guard<std::mutex> lk(g->mu);
            g->inflight.push_back(std::move(B));
            g->cv_slot.notify_all();
            continue;
        }
        std::unique_lock<std::mutex> lk(g->mu);
        if (done) {
            g->front_done = true;
            g->cv_slot.notify_all();
            return;
        }
        g->cv_slot.wait_for(lk, std::chrono::microseconds(200));
    }
}

// Back thread: stage B in batch order once a batch's ids are in, then the
// pipeline slot is free for the next batch; at the end, Packer::finalize.
void back_main(Ing *g) {
    (void)hipSetDevice(g->device);
    for (;;) {
        std::unique_ptr<Batch> B;
        bool last = false, all_done = false, fin_carry = false, aged = false;
        {
            std::unique_lock<std::mutex> lk(g->mu);
            for (;;) {
                if (g->err) {
                    g->cv_done.notify_all();
                    return;
                }
                if (!g->inflight.empty() && g->inflight.front()->long_jobs == 0) break;
                if (g->inflight.empty() && g->front_done) break;
                // MAX_AGE with no batch coming: the open pack is saved on its
                // own (a trickle backup leaves recent packs behind)
                if (g->inflight.empty() && !g->carry_blobs.empty() &&
                    now_s() - g->pack_t0 >= g->pack_max_age) {
                    aged = true;
                    break;
                }
                g->cv_slot.wait_for(lk, std::chrono::microseconds(200));
            }
            if (aged) {
            } else if (!g->inflight.empty()) {
                B = std::move(g->inflight.front());
                g->inflight.pop_front();
                last = g->front_done && g->inflight.empty();
            } else {
                all_done = true;
                fin_carry = !g->carry_blobs.empty();
            }
        }
        if (aged) {
            if (!close_open_pack(g)) return;
            continue;
        }
        if (B) {
            if (!stage_b(g, B.get(), last)) return;
            std::lock_guard<std::mutex> lk(g->mu);
            g->ps[B->pslot].busy = false;
            g->cv_slot.notify_all();
            continue;
        }
        if (all_done) {
            if (fin_carry && !close_open_pack(g)) return;  // Packer::finalize
            std::unique_lock<std::mutex> lk(g->mu);
            g->finished = true;
            g->cv_done.notify_all();
            return;
        }
    }
}

// Closed slots whose reservations are all in enter the pipeline (`ready`).
// A slot holding stream pieces enters only at the head of the close order:
// a stream's pieces are chunked in the order they were reserved, and its
// carry passes from batch to batch.  Others may pass a slot still waiting
// for a commit.  A slot left with nothing (every file cancelled) is free.
void promote_locked(Ing *g) {
    bool head = true;
    for (auto it = g->closed_q.begin(); it != g->closed_q.end();) {
        InSlot *s = *it;
        if (s->open_res == 0 && (head || !s->has_stream)) {
            it = g->closed_q.erase(it);
            bool empty = true;
            for (const FileEnt &f : s->files) empty &= f.cancelled;
            if (empty) {
                s->reset(kFree);
            } else {
                g->ready.push_back(s);
            }
            g->cv_slot.notify_all();
            continue;
        }
        head = false;
        ++it;
    }
}

void close_open_locked(Ing *g) {
    InSlot *s = g->open;
    if (!s) return;
    g->open = nullptr;
    s->close_seq = g->nclosed++;
    s->state = kClosed;
    g->closed_q.push_back(s);
    promote_locked(g);
    g->cv_slot.notify_all();
}

// Space for len bytes in the open slot (a new one when it does not fit).  A
// stream's piece goes right after the stream's previous piece when that is
// committed and the last thing in the slot (the two are then one range).
rcdc_status reserve_locked(Ing *g, std::unique_lock<std::mutex> &lk, uint64_t len,
                           const std::shared_ptr<StreamSt> &st, bool final, uint8_t **buf,
                           uint64_t *ticket) {
    for (;;) {
        if (g->err) return set_error(g->err, g->err_msg.c_str());
        if (g->finishing) return set_error(RCDC_ERR_INVALID_INPUT, "ingest already finishing");
        InSlot *s = g->open;
        // the first slot closes at a quarter: the device starts sooner
        const uint64_t cap_now = g->nclosed == 0 ? std::max(g->batch_cap / 4, len)
                                                 : (s ? s->host.cap : 0);
        uint64_t place = s ? s->used : 0;
        if (s && st && !s->files.empty()) {
            const FileEnt &b = s->files.back();
            if (b.st == st && b.done && !b.cancelled && s->used == round_up(b.off + b.res, 256))
                place = b.off + b.len;
        }
        if (s && place + len > cap_now) {
            close_open_locked(g);
            s = nullptr;
            place = 0;
        }
        if (!s) {
            for (auto &x : g->in)
                if (x->state == kFree) {
                    s = x.get();
                    break;
                }
            if (s) {
                s->reset(kOpen);
                g->open = s;
            }
        }
        if (s) {
            FileEnt f;
            f.off = place;
            f.res = len;
            f.st = st;
            f.final = final;
            s->files.push_back(f);
            s->used = round_up(place + len, 256);
            s->open_res++;
            s->has_stream |= st != nullptr;
            if (s->files.size() == 1) s->t_first = now_s();
            size_t idx = 0;
            for (; idx < g->in.size(); idx++)
                if (g->in[idx].get() == s) break;
            *ticket = ((uint64_t)idx << 32) | (uint64_t)(s->files.size() - 1);
            *buf = s->host + place;
            return RCDC_OK;
        }
        g->cv_slot.wait_for(lk, std::chrono::milliseconds(1));
        lk.unlock();
        reap_inputs(g);
        lk.lock();
    }
}

// Commit (or cancel) a reservation.
rcdc_status commit_locked(Ing *g, uint64_t ticket, uint64_t tag, uint64_t len, bool cancel) {
    const uint64_t si = ticket >> 32, fi = ticket & 0xFFFFFFFFull;
    if (si >= g->in.size() || fi >= g->in[si]->files.size() || g->in[si]->files[fi].done ||
        (g->in[si]->state != kOpen && g->in[si]->state != kClosed))
        return set_error(RCDC_ERR_INVALID_INPUT, "bad ticket");
    InSlot *s = g->in[si].get();
    FileEnt &f = s->files[fi];
    if (len > f.res) return set_error(RCDC_ERR_INVALID_INPUT, "commit longer than the reservation");
    if (!f.st) f.tag = tag;
    f.len = cancel ? 0 : len;
    f.done = true;
    f.cancelled = cancel;
    if (f.st) {
        f.st->fed += f.len;
        f.st->open_pieces--;
    }
    s->open_res--;
    if (s->state == kClosed && s->open_res == 0) promote_locked(g);
    return RCDC_OK;
}

std::shared_ptr<StreamSt> find_stream(Ing *g, uint64_t h) {
    auto it = g->streams.find(h);
    return it == g->streams.end() ? nullptr : it->second;
}

rcdc_status stream_end(Ing *g, uint64_t handle, bool abort) {
    if (!g) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::unique_lock<std::mutex> lk(g->mu);
    auto st = find_stream(g, handle);
    if (!st) return set_error(RCDC_ERR_INVALID_INPUT, "unknown stream");
    if (st->open_pieces)
        return set_error(RCDC_ERR_INVALID_INPUT, "stream has pieces not committed or cancelled");
    // a zero-byte final piece carries the end through the pipeline
    uint8_t *buf;
    uint64_t t;
    if (rcdc_status rs = reserve_locked(g, lk, 0, st, true, &buf, &t)) return rs;
    st->closed = true;
    st->aborted = abort;
    g->streams.erase(handle);
    g->closing_streams++;
    return commit_locked(g, t, 0, 0, false);
}

// Engine buffer sizes for a config (create and rcdc_ingest_footprint).
struct Sizes {
    uint64_t batch_cap, max_chunk, min_chunk;
    uint32_t depth, nin, nout, nthreads, max_streams;
    uint64_t out_slot, asm_base, asm_cap, arena, staging, refs_cap, frames, carry, carry_pool;
    uint64_t pinned() const { return nin * batch_cap + nout * out_slot + depth * refs_cap * 16; }
    uint64_t device() const {
        return depth * (arena + staging + refs_cap * 48) + 2 * frames + 2 * carry + carry_pool;
    }
};

Sizes engine_sizes(const rcdc_ctx *ctx, const rcdc_ingest_config *cfg, uint64_t pack_size) {
    Sizes z{};
    z.batch_cap = round_up(cfg->batch_bytes ? cfg->batch_bytes : (2ull << 30), 256);
    z.max_chunk = round_up(std::max<uint64_t>(ctx_max_size(ctx), 64), 256);
    z.min_chunk = std::max<uint64_t>(ctx_min_size(ctx), 4096);
    z.depth = cfg->depth ? cfg->depth : 4;
    z.nin = std::max(cfg->in_slots ? cfg->in_slots : 4u, 2u);
    z.nout = std::max(cfg->out_slots ? cfg->out_slots : 4u, 1u);
    z.nthreads = cfg->hash_threads ? cfg->hash_threads : 10;
    z.max_streams = cfg->max_streams ? cfg->max_streams : 16;
    z.out_slot = z.batch_cap + z.batch_cap / 16 + (64ull << 20);
    // a batch's stream units gathered: its pieces plus one carry per stream
    z.asm_base = round_up(z.batch_cap + 1024, 256);
    z.asm_cap = z.batch_cap + (uint64_t)z.max_streams * (z.max_chunk + 256) + 256;
    z.arena = z.asm_base + z.asm_cap + 1024;
    const uint64_t chunked = z.batch_cap + (uint64_t)z.max_streams * z.max_chunk;
    z.staging = chunked + chunked / 64 + (64ull << 20);
    z.frames = z.staging;
    z.refs_cap = chunked / z.min_chunk * 2 + 1024;
    z.carry = std::max<uint64_t>(pack_size * 2, 128ull << 20);
    z.carry_pool = (uint64_t)z.max_streams * z.max_chunk;
    return z;
}

// create's failures: nothing to free by hand (the engine's owners do it)
rcdc_status create_fail(hipError_t e, const char *what) {
    return set_error(RCDC_ERR_INTERNAL, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}
#define NEW_TRY(expr, what)                                         \
    do {                                                            \
        hipError_t e_ = (expr);                                     \
        if (e_ != hipSuccess) return create_fail(e_, what);         \
    } while (0)

// One pipeline slot's stream, events, buffers and plan (create).
rcdc_status build_pslot(Ing *g, PSlot &P, const Sizes &z) {
    // the chunk-id kernel runs for up to ~60 ms (a 2 MiB chunk's
    // SHA-256 chain on one lane): its stream gets the lowest priority, so
    // HIP puts it on a hardware queue of its own class -- a stream that
    // shared its queue waited behind it in order (r5o: each batch's
    // chunking started only when the previous batch's ids were done)
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    NEW_TRY(hipStreamCreateWithPriority(&P.s_ids.h, hipStreamNonBlocking, prio_lo), "stream");
    NEW_TRY(P.ev_ids.create(), "stream");
    NEW_TRY(P.ev_sealed.create(), "stream");
    NEW_TRY(P.ev_retired.create(), "stream");
    // device buffers sized for a full batch up front (a hipFree inside
    // the pipeline would synchronise the device): the slot's bytes, then
    // the assembly region for streams' gathered pieces and carries
    NEW_TRY(P.arena.alloc(g, z.arena, false), "arena");
    NEW_TRY(P.staging.alloc(g, z.staging, false), "staging");
    // the plan built once for a full-batch layout (allocations and
    // synchronous uploads here, not inside the pipeline); each batch then
    // re-lays it out on its compute stream, reusing the buffers
    // (256 streams: its per-stream arrays then hold any batch of up to
    // 256 files without a regrow; r5j logged five regrows per slot with
    // a one-stream layout, each a device-wide hipFree)
    constexpr uint32_t kPlanStreams = 256;
    std::vector<uint64_t> off0(kPlanStreams), len0(kPlanStreams);
    const uint64_t per = (g->batch_cap / kPlanStreams) & ~255ull;
    for (uint32_t i = 0; i < kPlanStreams; i++) {
        off0[i] = i * per;
        len0[i] = per;
    }
    rcdc_plan *pl = nullptr;
    if (rcdc_status ps = rcdc_plan_create(g->ctx, off0.data(), len0.data(), kPlanStreams,
                                          g->batch_cap + 256, &pl))
        return ps;
    P.plan.reset(pl);
    // ... and run once in that layout and in the one-stream layout (the
    // walk path's buffers at full size; the arena's bytes do not matter):
    // a plan's first run in a new layout allocated inside the pipeline,
    // and each allocation's hipFree waited for every queued copy and
    // kernel (r5u: 30-55 ms in each slot's first relayout)
    std::vector<uint64_t> wc(g->batch_cap / 4096 + kPlanStreams + 16), wn(kPlanStreams);
    for (uint32_t ns : {0u, 1u, 2u, 4u, 16u}) {  // as created, then walked layouts of 1-16 streams
        std::vector<uint64_t> o(ns), l(ns);
        const uint64_t each = (g->batch_cap / std::max(ns, 1u)) & ~255ull;
        for (uint32_t i = 0; i < ns; i++) {
            o[i] = i * each;
            l[i] = each;
        }
        if (rcdc_status ps = ns ? rcdc::plan_relayout(pl, o.data(), l.data(), ns,
                                                      g->batch_cap + 256, nullptr)
                                : RCDC_OK)
            return ps;
        if (rcdc_status ps = rcdc_plan_run(pl, P.arena, nullptr)) return ps;
        if (rcdc_status ps = rcdc_plan_results(pl, wc.data(), wc.size(), wn.data());
            ps && ps != RCDC_ERR_CAPACITY)
            return ps;
    }
    // short-chunk refs for a batch of minimum-size chunks
    NEW_TRY(P.h_refs.alloc(g, z.refs_cap * 2, true), "refs");
    NEW_TRY(P.d_refs.alloc(g, z.refs_cap * 2, false), "refs");
    NEW_TRY(P.d_dig.alloc(g, z.refs_cap * 32, false), "refs");
    return RCDC_OK;
}

// Every buffer, stream, event and plan of the engine, in this order (the
// order of the allocations is part of the engine's timing: keep it).
rcdc_status build_engine(Ing *g, const Sizes &z) {
    for (uint32_t i = 0; i < g->nin; i++) {
        g->in.push_back(std::make_unique<InSlot>());
        NEW_TRY(g->in.back()->host.alloc(g, g->batch_cap, true), "input slot");
        NEW_TRY(g->in.back()->h2d.create(), "event");
    }
    for (uint32_t i = 0; i < g->nout; i++) {
        g->outs.push_back(std::make_unique<OutSlot>());
        NEW_TRY(g->outs.back()->host.alloc(g, z.out_slot, true), "output slot");
    }
    // the open pack's carry buffers, sized for a default pack and its slack
    for (int c = 0; c < 2; c++) NEW_TRY(g->carry[c].alloc(g, z.carry, false), "carry");
    NEW_TRY(g->carry_pool.alloc(g, z.carry_pool, false), "stream carries");
    g->ps = std::vector<PSlot>(g->depth);
    for (auto &P : g->ps)
        if (rcdc_status st = build_pslot(g, P, z)) return st;
    NEW_TRY(g->frames.alloc(g, z.frames, false), "frames");
    NEW_TRY(g->d_packs.alloc(g, z.frames, false), "packs");
    NEW_TRY(hipStreamCreateWithFlags(&g->s_in.h, hipStreamNonBlocking), "streams");
    NEW_TRY(hipStreamCreateWithFlags(&g->s_comp.h, hipStreamNonBlocking), "streams");
    NEW_TRY(hipStreamCreateWithFlags(&g->s_out.h, hipStreamNonBlocking), "streams");
    NEW_TRY(hipStreamCreateWithFlags(&g->s_back.h, hipStreamNonBlocking), "streams");
    NEW_TRY(g->ev_comp.create(), "streams");
    NEW_TRY(g->ev_back.create(), "streams");
    NEW_TRY(g->ev_out.create(), "streams");
    NEW_TRY(hipEventRecord(g->ev_out, g->s_out), "event");
    return RCDC_OK;
}
#undef NEW_TRY

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

void rcdc_ingest_config_default(rcdc_ingest_config *c) {
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->zstd_level = 0;
    c->compress = 1;
    c->extra_verify = 1;
    c->pack_size = 32ull << 20;  // configfile.rs:211-231 (data packs)
    c->pack_grow_factor = 32;
    c->pack_size_limit = 0xFFFFFFFFull;
    c->batch_bytes = 2ull << 30;
    c->depth = 4;
    c->in_slots = 4;
    c->out_slots = 4;
    c->hash_threads = 10;
    c->max_streams = 16;
    c->long_chunk = 2ull << 20;
    c->pack_max_age_ms = 300000;  // packer.rs:63 MAX_AGE = 5 min
    c->slot_max_age_ms = 1000;
}

rcdc_status rcdc_ingest_footprint(const rcdc_ctx *ctx, const rcdc_ingest_config *cfg,
                                  uint64_t *pinned, uint64_t *device) {
    if (!ctx || !cfg) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    PackSizer ps{cfg->pack_size ? cfg->pack_size : (32ull << 20), cfg->pack_grow_factor,
                 cfg->pack_size_limit ? cfg->pack_size_limit : 0xFFFFFFFFull, cfg->pack_current_size};
    const Sizes z = engine_sizes(ctx, cfg, ps.pack_size());
    if (pinned) *pinned = z.pinned();
    if (device) *device = z.device();
    return RCDC_OK;
}

void rcdc_ingest_mem_live(uint64_t *pinned, uint64_t *device) {
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    if (pinned) *pinned = g_live_pinned;
    if (device) *device = g_live_dev;
}

rcdc_status rcdc_ingest_create(rcdc_ctx *ctx, const rcdc_ingest_config *cfg,
                               rcdc_ingest_pack_fn pack_cb, rcdc_ingest_file_fn file_cb,
                               void *user, rcdc_ingest **out) {
    if (!ctx || !cfg || !out) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    if (cfg->zstd_level < -131072 || cfg->zstd_level > 22)
        return set_error(RCDC_ERR_INVALID_INPUT, "zstd level out of range");
    auto g = std::make_unique<rcdc_ingest>();
    g->ctx = ctx;
    g->cfg = *cfg;
    g->pack_cb = pack_cb;
    g->file_cb = file_cb;
    g->user = user;
    g->device = ctx_device(ctx);
    g->level = cfg->zstd_level;
    g->compress = cfg->compress != 0;
    g->verify = cfg->extra_verify != 0;
    g->sizer.default_size = cfg->pack_size ? cfg->pack_size : (32ull << 20);
    g->sizer.grow = cfg->pack_grow_factor;
    g->sizer.limit = cfg->pack_size_limit ? cfg->pack_size_limit : 0xFFFFFFFFull;
    g->sizer.current = cfg->pack_current_size;
    const Sizes z = engine_sizes(ctx, cfg, g->sizer.pack_size());
    g->batch_cap = z.batch_cap;
    g->long_chunk = cfg->long_chunk ? cfg->long_chunk : (2ull << 20);
    g->depth = z.depth;
    g->nin = z.nin;
    g->nout = z.nout;
    g->nthreads = z.nthreads;
    g->max_chunk = z.max_chunk;
    g->asm_base = z.asm_base;
    g->asm_cap = z.asm_cap;
    g->pack_max_age = (cfg->pack_max_age_ms ? cfg->pack_max_age_ms : 300000) / 1e3;
    g->slot_max_age = (cfg->slot_max_age_ms ? cfg->slot_max_age_ms : 1000) / 1e3;
    g->own_idx = std::make_unique<rcdc_index>();
    g->idx = g->own_idx.get();
    for (uint32_t i = 0; i < z.max_streams; i++) g->free_cslots.push_back((int)(z.max_streams - 1 - i));
    Ing *gp = g.get();
    (void)hipSetDevice(g->device);
    if (rcdc_status st = build_engine(gp, z)) {
        // what was built so far goes with the engine, the device still current
        const std::string m = rcdc_last_error();
        g.reset();
        return set_error(st, m.c_str());
    }
    for (uint32_t i = 0; i < g->nthreads; i++) g->pool.emplace_back(pool_main, gp);
    g->waiter = std::thread(waiter_main, gp);
    g->worker = std::thread(worker_main, gp);
    g->feeder = std::thread(feeder_main, gp);
    g->back = std::thread(back_main, gp);
    *out = g.release();
    return RCDC_OK;
}

rcdc_status rcdc_ingest_add_index(rcdc_ingest *g, const uint8_t *ids, uint64_t n) {
    if (!g || (n && !ids)) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->nbatches) return set_error(RCDC_ERR_INVALID_INPUT, "index ids after the first batch");
    return rcdc_index_add(g->idx, ids, n);
}

rcdc_status rcdc_ingest_reserve(rcdc_ingest *g, uint64_t len, uint8_t **buf, uint64_t *ticket) {
    if (!g || !buf || !ticket) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    if (len > g->batch_cap)
        return set_error(RCDC_ERR_UNSUPPORTED,
                         "file larger than the ingest batch (batch_bytes): feed it as a stream "
                         "(rcdc_ingest_stream_open)");
    std::unique_lock<std::mutex> lk(g->mu);
    return reserve_locked(g, lk, len, nullptr, false, buf, ticket);
}

rcdc_status rcdc_ingest_commit(rcdc_ingest *g, uint64_t ticket, uint64_t tag, uint64_t len) {
    if (!g) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    return commit_locked(g, ticket, tag, len, false);
}

rcdc_status rcdc_ingest_cancel(rcdc_ingest *g, uint64_t ticket) {
    if (!g) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    return commit_locked(g, ticket, 0, 0, true);
}

rcdc_status rcdc_ingest_stream_open(rcdc_ingest *g, uint64_t tag, uint64_t size_hint,
                                    uint64_t *stream) {
    if (!g || !stream) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::unique_lock<std::mutex> lk(g->mu);
    for (;;) {
        if (g->err) return set_error(g->err, g->err_msg.c_str());
        if (g->finishing) return set_error(RCDC_ERR_INVALID_INPUT, "ingest already finishing");
        if (!g->free_cslots.empty()) break;
        if (!g->closing_streams)
            return set_error(RCDC_ERR_UNSUPPORTED, "max_streams streams are open");
        // streams that ended free their carry slots once their last batch
        // has been chunked: send the open slot on its way
        close_open_locked(g);
        g->cv_slot.wait_for(lk, std::chrono::milliseconds(1));
    }
    auto st = std::make_shared<StreamSt>();
    st->handle = g->next_stream++;
    st->tag = tag;
    st->hint = size_hint;
    st->cslot = g->free_cslots.back();
    g->free_cslots.pop_back();
    g->streams[st->handle] = st;
    *stream = st->handle;
    return RCDC_OK;
}

rcdc_status rcdc_ingest_stream_reserve(rcdc_ingest *g, uint64_t stream, uint64_t len,
                                       uint8_t **buf, uint64_t *ticket) {
    if (!g || !buf || !ticket) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    if (len > g->batch_cap)
        return set_error(RCDC_ERR_UNSUPPORTED, "piece larger than the ingest batch (batch_bytes)");
    std::unique_lock<std::mutex> lk(g->mu);
    auto st = find_stream(g, stream);
    if (!st) return set_error(RCDC_ERR_INVALID_INPUT, "unknown stream");
    st->open_pieces++;
    const rcdc_status rs = reserve_locked(g, lk, len, st, false, buf, ticket);
    if (rs) st->open_pieces--;
    return rs;
}

rcdc_status rcdc_ingest_stream_close(rcdc_ingest *g, uint64_t stream) {
    return stream_end(g, stream, false);
}

rcdc_status rcdc_ingest_stream_abort(rcdc_ingest *g, uint64_t stream) {
    return stream_end(g, stream, true);
}

rcdc_status rcdc_ingest_add(rcdc_ingest *g, uint64_t tag, const void *data, uint64_t len) {
    if (!g || (len && !data)) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    uint8_t *buf;
    uint64_t t;
    if (len <= g->batch_cap) {
        rcdc_status s = rcdc_ingest_reserve(g, len, &buf, &t);
        if (s) return s;
        memcpy(buf, data, len);
        return rcdc_ingest_commit(g, t, tag, len);
    }
    // larger than a batch: a stream of quarter-batch pieces
    uint64_t h;
    if (rcdc_status s = rcdc_ingest_stream_open(g, tag, len, &h)) return s;
    const uint64_t piece = std::max<uint64_t>(g->batch_cap / 4 & ~255ull, 256);
    for (uint64_t o = 0; o < len; o += piece) {
        const uint64_t n = std::min(piece, len - o);
        rcdc_status s = rcdc_ingest_stream_reserve(g, h, n, &buf, &t);
        if (s) {
            (void)rcdc_ingest_stream_abort(g, h);
            return s;
        }
        memcpy(buf, (const uint8_t *)data + o, n);
        if ((s = rcdc_ingest_commit(g, t, 0, n))) {
            const std::string m = rcdc_last_error();
            (void)rcdc_ingest_cancel(g, t);  // (a failed commit leaves the piece open)
            (void)rcdc_ingest_stream_abort(g, h);
            return set_error(s, m.c_str());
        }
    }
    return rcdc_ingest_stream_close(g, h);
}

rcdc_status rcdc_ingest_flush(rcdc_ingest *g) {
    if (!g) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    close_open_locked(g);
    return g->err ? set_error(g->err, g->err_msg.c_str()) : RCDC_OK;
}

rcdc_status rcdc_ingest_finish(rcdc_ingest *g, rcdc_ingest_stats *stats) {
    if (!g) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    {
        std::unique_lock<std::mutex> lk(g->mu);
        if (!g->streams.empty())
            return set_error(RCDC_ERR_INVALID_INPUT, "streams still open (close or abort them first)");
        close_open_locked(g);
        g->finishing = true;
        g->cv_slot.notify_all();
        g->cv_done.wait(lk, [&] { return g->finished || g->err; });
        g->cv_done.wait(lk, [&] { return g->packs_pending == 0 || g->err; });
        g->st.seconds = g->t_first ? now_s() - g->t_first : 0;
        if (stats) *stats = g->st;
        if (g->knobs.prof) {
            std::lock_guard<std::mutex> lk2(g->cb_mu);
            for (size_t b = 0; b < g->tl.size(); b++) {
                fprintf(stderr, "ingest batch %zu:", b);
                for (double t : g->tl[b]) fprintf(stderr, " %.1f", t * 1e3);
                if (b < g->tl_d2h.size() && g->tl_d2h[b] > 0)
                    fprintf(stderr, " | landed %.1f", g->tl_d2h[b] * 1e3);
                if (b < g->tl_ids.size() && g->tl_ids[b] > 0)
                    fprintf(stderr, " ids %.1f", g->tl_ids[b] * 1e3);
                fprintf(stderr, " ms\n");
            }
            fprintf(stderr, "ingest end %.1f ms\n", g->st.seconds * 1e3);
        }
        if (g->err) return set_error(g->err, g->err_msg.c_str());
    }
    return RCDC_OK;
}

void rcdc_ingest_destroy(rcdc_ingest *g) {
    if (!g) return;
    {
        std::unique_lock<std::mutex> lk(g->mu);
        if (!g->finished && !g->err) {  // abandoned: stop after what is queued
            g->err = RCDC_ERR_INTERNAL;
            g->err_msg = "destroyed";
        }
        g->cv_slot.notify_all();
    }
    if (g->worker.joinable()) g->worker.join();
    if (g->feeder.joinable()) g->feeder.join();
    if (g->back.joinable()) g->back.join();
    {
        std::unique_lock<std::mutex> lk(g->mu);
        g->cv_done.wait_for(lk, std::chrono::seconds(30), [&] { return g->packs_pending == 0; });
    }
    g->stop = true;
    g->wait_cv.notify_all();
    g->pool_cv.notify_all();
    if (g->waiter.joinable()) g->waiter.join();
    for (auto &t : g->pool)
        if (t.joinable()) t.join();
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    delete g;  // its plans, buffers, events and streams go here, the device current
}

rcdc_status rcdc_index_create(rcdc_index **out) {
    if (!out) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    *out = new rcdc_index();
    return RCDC_OK;
}

void rcdc_index_destroy(rcdc_index *idx) { delete idx; }

rcdc_status rcdc_index_add(rcdc_index *idx, const uint8_t *ids, uint64_t n) {
    if (!idx || (n && !ids)) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    for (uint64_t i = 0; i < n; i++) {
        Id32 id;
        memcpy(id.b, ids + 32 * i, 32);
        idx->insert(id);
    }
    return RCDC_OK;
}

uint64_t rcdc_index_size(const rcdc_index *idx) {
    return idx ? const_cast<rcdc_index *>(idx)->size() : 0;
}

rcdc_status rcdc_ingest_set_index(rcdc_ingest *g, rcdc_index *idx) {
    if (!g || !idx) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->nbatches) return set_error(RCDC_ERR_INVALID_INPUT, "index set after the first batch");
    if (g->idx == idx) return RCDC_OK;
    for (auto &sh : g->idx->sh) {
        std::lock_guard<std::mutex> l2(sh.mu);
        for (const Id32 &id : sh.set) idx->insert(id);
    }
    g->own_idx.reset();
    g->idx = idx;
    return RCDC_OK;
}

rcdc_status rcdc_sha256_host_one(const void *data, uint64_t len, uint8_t *digest) {
    if ((len && !data) || !digest) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    host_sha256_one((const uint8_t *)data, len, digest);
    return RCDC_OK;
}

rcdc_status rcdc_sha256_host_ni(const void *const *ptrs, const uint64_t *lens, uint32_t n,
                                uint32_t ways, uint8_t *digests) {
    if (n && (!ptrs || !lens || !digests)) return set_error(RCDC_ERR_INVALID_INPUT, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (!ptrs[i] && lens[i]) return set_error(RCDC_ERR_INVALID_INPUT, "null buffer");
    if (ways < 1 || ways > 4) return set_error(RCDC_ERR_INVALID_INPUT, "ways must be 1-4");
    host_sha256_ni_many(reinterpret_cast<const uint8_t *const *>(ptrs), lens, n, digests,
                        (int)ways);
    return RCDC_OK;
}

}  // extern "C"
