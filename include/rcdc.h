/*
 * rcdc.h -- C ABI of librcdc, the MI355X-native content-defined chunker that
 * replaces rustic_core's Rabin CDC hot path.
 *
 * Drop-in point (reference = rustic_core 0.12.0, /root/reference):
 *   crates/core/src/chunker.rs:21-58  ChunkIter::from_config(&ConfigFile, R, size_hint)
 *                                     + Iterator<Item = RusticResult<Vec<u8>>>
 *   crates/core/src/chunker/rabin.rs:82-191  RabinChunkIter::{new, next}
 * called from crates/core/src/archiver/file_archiver.rs:144-160
 * (FileArchiver::backup_reader), one iterator per file on pariter workers
 * (crates/core/src/archiver.rs:195).
 *
 * Contract: every function returns cut offsets (END offset of each chunk,
 * i.e. the prefix sums of the chunk lengths the reference iterator yields)
 * that are bit-identical to what rabin.rs ChunkIter::next produces on the
 * same bytes with the same (poly, min, avg, max).  A Rust `ChunkIter::Gpu`
 * variant slices its buffer at these offsets.
 *
 * Plain C types only (pointers + sizes); no HIP or torch types appear in a
 * signature.  Device pointers are passed as `const void *` / `uint64_t`.
 * All entry points are thread-safe for distinct contexts/streams/plans; one
 * context may be shared by any number of threads (a pool of per-call lanes,
 * see the host-stream section).  A stream or plan is used by one thread at
 * a time.
 */
#ifndef RCDC_H
#define RCDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCDC_ABI_VERSION 5u

/* Status codes map onto rustic_core ErrorKind (crates/core/src/error.rs:108-124). */
typedef enum {
    RCDC_OK = 0,
    RCDC_ERR_UNSUPPORTED = 1,   /* ErrorKind::Unsupported  (rabin.rs:22-40)           */
    RCDC_ERR_INVALID_INPUT = 2, /* ErrorKind::InvalidInput (configfile.rs:166-171)     */
    RCDC_ERR_INTERNAL = 3,      /* ErrorKind::Internal     (HIP runtime failures)      */
    RCDC_ERR_INPUT_OUTPUT = 4,  /* ErrorKind::InputOutput  (rabin.rs:131-138,174-180)  */
    RCDC_ERR_CAPACITY = 5,      /* caller's cut buffer too small; counts still valid   */
    RCDC_ERR_VERIFICATION = 6   /* ErrorKind::Verification (decrypt.rs:516-526)       */
} rcdc_status;

typedef struct rcdc_ctx rcdc_ctx;       /* one device + chunker parameters      */
typedef struct rcdc_stream rcdc_stream; /* one file fed in pieces               */
typedef struct rcdc_plan rcdc_plan;     /* a fixed batch layout in device memory */

typedef struct {
    const uint8_t *data; /* host pointer (rcdc_chunk_batch)                */
    uint64_t len;
} rcdc_buf;

/* ---- parameters -------------------------------------------------------- */

/* check_rabin_params -- replaces crates/core/src/chunker/rabin.rs:17-42.
 * avg must be a power of two, min <= avg <= max.  Additionally rejected with
 * RCDC_ERR_UNSUPPORTED: min < 4096 and max > 2^40.  Below 4096 the
 * reference's `min_size -= open_buf_len` (rabin.rs:124, up to 4095 bytes of
 * its 4 KiB read buffer, rabin.rs:12) underflows -- a panic under debug
 * assertions, a read-pattern-dependent wrap in release -- so no bit-exact
 * cut list exists for such parameters.                                     */
rcdc_status rcdc_check_params(uint64_t avg, uint64_t min, uint64_t max);

/* ConfigFile::poly -- replaces crates/core/src/repofile/configfile.rs:165-175
 * (u64::from_str_radix(hex, 16)); RCDC_ERR_INVALID_INPUT on a bad string.   */
rcdc_status rcdc_parse_poly(const char *hex, uint64_t *poly);

/* ---- context ------------------------------------------------------------ */

/* Replaces Rabin64::new_with_polynom(6, &poly) + RabinChunkIter::new
 * (crates/core/src/chunker.rs:29-38, rabin.rs:82-104).  Builds the Rabin64
 * out/mod tables once per context (the reference rebuilds them per file) and
 * uploads them to `device`.  deg(poly) must be in [9, 56].                  */
rcdc_status rcdc_ctx_create(uint64_t poly, uint64_t min, uint64_t avg_pow2,
                            uint64_t max, int device, rcdc_ctx **out);
void rcdc_ctx_destroy(rcdc_ctx *ctx);

/* Message of the last failing call on this thread ("" if none). */
const char *rcdc_last_error(void);

/* Upper bound on the number of chunks of an n-byte stream. */
uint64_t rcdc_max_cuts(const rcdc_ctx *ctx, uint64_t n);

/* ---- independent host streams (per-file parallel path, archiver.rs:195) - */

/* Host-buffer calls (rcdc_chunk_batch, rcdc_stream_feed) may come from many
 * threads at once on one context, as the reference runs one ChunkIter per
 * file on pariter workers (archiver.rs:195).  Each call takes one of the
 * context's lanes -- a HIP stream, two pinned staging slots and a device
 * arena of its own -- for its duration, so concurrent calls overlap instead
 * of serialising; at most RCDC_LANES (environment, default 16) lanes exist,
 * further callers wait for a free one.  The caller's pageable bytes go
 * through the staging slots in 16 MiB blocks, the copy of block k + 1
 * overlapping the DMA of block k.                                          */

/* Chunk n independent host buffers; only the cut offsets come back.  Cuts of
 * stream i are written consecutively to cuts[] in stream order;
 * cut_counts[i] receives the count.  If the total exceeds cuts_cap,
 * RCDC_ERR_CAPACITY is returned with every cut_counts[i] valid and cuts[]
 * untouched (call again with a larger buffer).                            */
rcdc_status rcdc_chunk_batch(rcdc_ctx *ctx, const rcdc_buf *bufs, uint32_t n,
                             uint64_t *cuts, uint64_t cuts_cap,
                             uint64_t *cut_counts);

/* ---- one file fed in pieces (the Read-driven iterator) ------------------ */

/* Replaces the read loop of rabin.rs:110-191: the caller feeds the file in
 * arbitrary pieces (any split gives the same cuts, like the reference's
 * read()-independence).  Cut offsets (absolute, from the start of the file)
 * become final as enough bytes arrive; each call hands out up to `cap` of
 * them (*n_cuts) and keeps the rest queued for the next call -- a call with
 * len = 0 only drains the queue, and rcdc_stream_queued() tells how many
 * wait.  A feed never fails for lack of cut space and never consumes input
 * twice.  is_final = 1 marks EOF (the reference's Ok(0)); the last cut is
 * then the file length.
 * Retention: the stream buffers bytes until rcdc_stream_batch_bytes(ctx)
 * (16 MiB, at least 2 max + 256; environment RCDC_STREAM_BATCH) would be
 * pending, then runs one device pass over the buffered tail plus the new
 * piece, straight from the caller's buffer; afterwards it keeps only the
 * tail after the last final cut (< max bytes).  So at most batch + max
 * bytes are held -- more than the reference's 4 KiB + one chunk, for one
 * device pass per 16 MiB instead of a byte loop per chunk.
 * On an HIP failure the bytes stay buffered and the status is returned;
 * the feed may be retried with len = 0 (same is_final).                    */
rcdc_status rcdc_stream_open(rcdc_ctx *ctx, rcdc_stream **out);
rcdc_status rcdc_stream_feed(rcdc_stream *st, const uint8_t *data,
                             uint64_t len, int is_final, uint64_t *cuts,
                             uint64_t cap, uint64_t *n_cuts);
uint64_t rcdc_stream_queued(const rcdc_stream *st);
uint64_t rcdc_stream_batch_bytes(const rcdc_ctx *ctx);
void rcdc_stream_close(rcdc_stream *st);

/* ---- device-resident batches (the measured hot path) ------------------- */

/* A plan fixes a batch layout: n streams at byte offsets offs[i] (any
 * alignment) with lengths lens[i] inside a device arena of arena_len bytes.
 * It owns the device work lists, per-segment summaries and the cut output.
 * Requires the arena base pointer passed to rcdc_plan_run to be 256-B
 * aligned (hipMalloc / torch allocations are).                             */
rcdc_status rcdc_plan_create(rcdc_ctx *ctx, const uint64_t *offs,
                             const uint64_t *lens, uint32_t n,
                             uint64_t arena_len, rcdc_plan **out);
void rcdc_plan_destroy(rcdc_plan *plan);

/* Enqueue scan + resolve on `hip_stream` (a hipStream_t, or 0 for the
 * context's own stream) over the device arena `d_arena`.  Asynchronous. */
rcdc_status rcdc_plan_run(rcdc_plan *plan, const void *d_arena,
                          void *hip_stream);

/* Complete the last run on the host side: wait for it and, for any long
 * stream whose walk-path fixup overflowed its slots (never seen outside
 * forced tests), re-chunk it on the scan path and write its cuts -- and, if
 * the run was hashed, its digests -- back into the device buffers.  Until
 * this returns the device arena of the run must stay unchanged; after it,
 * the device views below are complete.  rcdc_plan_results and
 * rcdc_plan_digests call it.                                                */
rcdc_status rcdc_plan_finish(rcdc_plan *plan);

/* Finish the last run and copy the results to the host: same layout and
 * capacity rule as rcdc_chunk_batch.                                      */
rcdc_status rcdc_plan_results(rcdc_plan *plan, uint64_t *cuts,
                              uint64_t cuts_cap, uint64_t *cut_counts);

/* Device-side view of the results: stream i's cuts are
 * d_cuts[cut_base[i] .. cut_base[i] + d_counts[i]).  Complete after
 * rcdc_plan_finish; before it, a stream whose walk needs host completion
 * reads d_counts[i] == UINT64_MAX (and its digests are not written).
 * Ordering: a serial run's last kernel is ordered before later work on the
 * run's stream (for hip_stream = 0, before later work on the legacy default
 * stream too).  A pipelined run (rcdc_plan_set_pipeline) ends on a stream
 * of the plan's own and is NOT ordered before the caller's later work on any
 * stream: call rcdc_plan_finish (or synchronise the device) before reading
 * these buffers from device code.                                          */
rcdc_status rcdc_plan_device_results(rcdc_plan *plan, uint64_t *d_cuts,
                                     uint64_t *d_counts,
                                     const uint64_t **cut_base);

/* Crossing window of stream `stream` of the last run, for stitching one
 * stream sliced over GPUs (each rank runs a plan over its slice
 * plus a max + 64 byte halo).  Writes 3 + k words to the device buffer d_out
 * (8-B aligned), asynchronously on hip_stream (0: the context's stream),
 * ordered after the run: [0] the stream's cut count n, [1] j = the index of
 * its first cut >= bound (n if none), [2] that cut (UINT64_MAX if none),
 * [3 + t] cut t for t < k (UINT64_MAX for t >= n).  Cuts are relative to the
 * stream's first byte.  n == UINT64_MAX: the stream needs rcdc_plan_finish
 * (never seen outside forced tests); the caller then reads the host list.   */
rcdc_status rcdc_plan_window(rcdc_plan *plan, uint32_t stream, uint64_t bound, uint32_t k,
                             uint64_t *d_out, void *hip_stream);

/* Pipelined runs: with enable = 1, run k's hashing kernels (scan, walk) go
 * to hashing stream k % 2 of the plan's own (after the caller's earlier
 * work) and its chain kernels (resolve; walk check / fixup / assemble) to a
 * third stream, so run k's chain overlaps run k + 1's hashing; every
 * per-run buffer the chain reads alternates between two sets, and run
 * k + 2's hashing waits for run k's chain.  rcdc_plan_results /
 * rcdc_plan_hash wait for the last chain; a caller that reuses the arena
 * must synchronise the device (or call rcdc_plan_results) first.  The plan
 * then uses three streams: HIP maps a process's streams onto
 * GPU_MAX_HW_QUEUES hardware queues (4 by default), and kernels whose
 * streams share a queue run in order, so a caller that adds streams of its
 * own around a pipelined plan can serialise its chain with the next walk
 * (bench.py runs pipelined plans on the default stream).  enable = 0
 * restores serial runs.  enable = 2: pipelined, and the next run is the
 * last of the sequence: its chain kernels run on every CU instead of beside
 * a next walk (a pipeline flush; one-shot, later runs are narrow again).    */
rcdc_status rcdc_plan_set_pipeline(rcdc_plan *plan, int enable);

/* Scan-kernel geometry chosen by the plan (for profiling / roofline). */
typedef struct {
    uint64_t scanned_bytes;   /* bytes the scan kernel must hash         */
    uint64_t segments;        /* per-lane segments                       */
    uint32_t segment_bytes;   /* S                                        */
    uint32_t work_items;      /* 64-segment wave work items               */
    uint32_t scan_blocks;     /* workgroups of the scan launch            */
    uint32_t walk_pieces;     /* pieces of long streams on the walk path  */
    uint32_t walk_seg_bytes;  /* S of the walk kernel's 64-lane rounds    */
    uint32_t pad;
} rcdc_plan_info;
rcdc_status rcdc_plan_get_info(const rcdc_plan *plan, rcdc_plan_info *info);

/* Kernel timing (HIP events recorded on the launch stream around the scan
 * and the resolve kernel while enabled).  enable = P >= 1 starts a fresh
 * accumulation and times every P-th run from the next one on (P = 1: every
 * run; a larger P samples the runs and keeps the events' own inter-kernel
 * gaps out of most of them); 0 stops recording.  rcdc_plan_kernel_times
 * waits for the timed runs and returns their count and summed device times. */
rcdc_status rcdc_plan_set_timing(rcdc_plan *plan, int enable);
rcdc_status rcdc_plan_kernel_times(rcdc_plan *plan, uint64_t *runs,
                                   double *scan_ms_total,
                                   double *resolve_ms_total);

/* Work counters of the walk path (long streams) of the last run, after it
 * completes: stats[0] 64-lane hashing rounds of rcdc_walk_kernel, [1] its
 * min-zone evaluations (64 windows of 64 bytes), [2] chunks it emitted, [3]
 * 1024-lane rounds of the fixup kernel (1024 x (512 + 64) bytes each), [4]
 * fixup zones, [5] cuts the fixups walked, [6] 64-lane rounds of the
 * boundary check kernel over bytes no walker searched, [7] its zone
 * evaluations, [8] the bytes the walk kernel's rounds hashed (64 x (S + 64)
 * per round; the last round of a search with a known end -- a piece's stop,
 * a chunk's max, EOF -- hashes only the 64-byte units it needs), [9] the
 * same for the check kernel's rounds.  With the environment variable
 * RCDC_WALK_TRACE=1 at plan creation, `trace` (if not NULL) receives 4
 * words per walk piece: wall clock (100 MHz) at the piece's start and end,
 * rounds, chunks; then 4 words per piece boundary (rows of piece 0 unused)
 * from the check kernel: start, end, gap rounds, hop entries -- at most
 * trace_cap words (2 x walk_pieces x 4 in all).  All zero for plans without
 * walked streams.                                                          */
#define RCDC_WALK_STATS 10
rcdc_status rcdc_plan_walk_stats(rcdc_plan *plan, uint64_t *stats, uint64_t *trace,
                                 uint64_t trace_cap);

/* ---- FixedSize chunker (crates/core/src/chunker/fixed_size.rs:41-70) ---- */
/* Cuts every `size` bytes, last chunk short; returns the count.           */
uint64_t rcdc_fixed_cuts(uint64_t n, uint64_t size, uint64_t *cuts,
                         uint64_t cap);

/* ---- SHA-256 blob ids: crypto/hasher.rs:17-19 `hash(&chunk)`, called per
 * chunk by FileArchiver::backup_reader (archiver/file_archiver.rs:151) ---- */

/* One chunk of a device arena: bytes [off, off + len). */
typedef struct {
    uint64_t off;
    uint64_t len;
} rcdc_chunk_ref;

/* SHA-256 of n chunks of a device arena.  d_refs (16-B aligned) and
 * d_digests (32 bytes per chunk, 4-B aligned) are device pointers.
 * Asynchronous on hip_stream (0: the context's stream).                    */
rcdc_status rcdc_sha256_chunks(rcdc_ctx *ctx, const void *d_arena,
                               const rcdc_chunk_ref *d_refs, uint32_t n,
                               uint8_t *d_digests, void *hip_stream);

/* SHA-256 of n buffers in host memory (pack ids: blob/packer.rs:832-834
 * `hash_reader` of each finished pack file), on the calling thread: 16
 * messages side by side in the lanes of AVX-512 registers, a lane taking the
 * next message when its own ends.  digests: 32 bytes per buffer.
 * RCDC_ERR_UNSUPPORTED on a CPU without AVX-512F/BW (no digest written).   */
rcdc_status rcdc_sha256_host(const void *const *ptrs, const uint64_t *lens, uint32_t n,
                             uint8_t *digests);

/* Page-locked host memory for read buffers.  Host-buffer calls
 * (rcdc_stream_feed, rcdc_chunk_batch) whose pieces all lie in such memory
 * copy them to the device by DMA straight from the caller's buffer, with no
 * staging copy.  The reference reads into a Vec (rabin.rs:110-191); this is
 * the buffer a caller's read loop would fill instead.  rcdc_host_free(NULL)
 * is a no-op.                                                              */
rcdc_status rcdc_host_alloc(uint64_t bytes, void **out);
void rcdc_host_free(void *p);

/* Fused blob ids of a plan: after rcdc_plan_run over d_arena (the same
 * pointer), enqueue the SHA-256 of every chunk it found, on the device
 * cut list (no host round trip).  Asynchronous.                           */
rcdc_status rcdc_plan_hash(rcdc_plan *plan, const void *d_arena,
                           void *hip_stream);

/* rcdc_plan_hash for up to 8 plans of one context in a single launch (plan
 * j over d_arenas[j], its last run's arena), so their chunks share the
 * longest-chunk latency floor instead of queueing per stream.            */
rcdc_status rcdc_plan_hash_many(rcdc_plan *const *plans, uint32_t n,
                                const void *const *d_arenas, void *hip_stream);

/* Synchronise and copy the digests to the host: 32 bytes per chunk, in the
 * order of rcdc_plan_results' cuts (whose counts it also writes).          */
rcdc_status rcdc_plan_digests(rcdc_plan *plan, uint8_t *digests,
                              uint64_t cap_chunks, uint64_t *cut_counts);

/* Device view: slot-indexed like rcdc_plan_device_results' d_cuts. */
rcdc_status rcdc_plan_device_digests(rcdc_plan *plan, uint64_t *d_digests);

/* ---- blob encryption: crypto/aespoly1305.rs:88-135 `Key::encrypt_data` /
 * `decrypt_data` (aes256ctr_poly1305aes 0.2.1, the restic format), applied
 * by the packer to every new blob (blob/packer.rs:268-270,
 * backend/decrypt.rs:566-572) -- here to chunks already in HBM. ---------- */

/* One blob.  seal: data [in_off, in_off + len) of d_in becomes
 * nonce || AES-256-CTR ciphertext || Poly1305-AES tag (len + 32 bytes) at
 * out_off of d_out.  open: the sealed blob [in_off, in_off + len) (len >= 32)
 * becomes its len - 32 plaintext bytes at out_off.  Offsets may have any
 * alignment (16-byte aligned outputs store fastest; allow 4 readable bytes
 * after each input).  The nonce is the caller's (rustic draws it at random,
 * :120-121). */
typedef struct {
    uint64_t in_off;
    uint64_t len;
    uint64_t out_off;
    uint8_t nonce[16]; /* seal only; open reads it from the blob */
} rcdc_aead_ref;

/* key: 64 bytes, AES-256 key || Poly1305-AES k || r (aespoly1305.rs:15-24).
 * refs is a HOST array.  Asynchronous on hip_stream (0: the context's
 * stream); calls on one context take turns (the second waits for the
 * first's kernels).                                                         */
rcdc_status rcdc_aead_seal(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                           const rcdc_aead_ref *refs, uint32_t n, void *d_out,
                           void *hip_stream);
/* status[i] (host array): 0 = MAC ok, 1 = MAC mismatch or shorter than
 * nonce + tag (ErrorKind::Cryptography, aespoly1305.rs:97-108; the plaintext
 * written is then not to be used), 2 = shorter than 16 bytes (:89-94).
 * Synchronous.                                                              */
rcdc_status rcdc_aead_open(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                           const rcdc_aead_ref *refs, uint32_t n, void *d_out,
                           uint32_t *status, void *hip_stream);

/* ---- pack files: blob/packer.rs:615-655 (add_raw), :693-735 (save,
 * write_header) and repofile/packfile.rs (HeaderEntry, PackHeaderRef) -- the
 * packer's byte work for blobs in HBM: each pack is its blobs sealed back to
 * back, then the sealed pack header, then its length (u32 LE). ---------- */

typedef struct {
    uint64_t in_off;           /* the blob's bytes in d_in (as stored: the raw blob, or the
                                  zstd frame of a compressed one)                         */
    uint32_t len;              /* bytes at in_off                                          */
    uint32_t uncompressed_len; /* 0: stored as is (HeaderEntry Data / Tree); else the raw
                                  length of a compressed blob (CompData / CompTree)       */
    uint32_t type;             /* BlobType: 0 data, 1 tree                                 */
    uint32_t pad;
    uint8_t id[32];            /* blob id                                                  */
    uint8_t nonce[16];
} rcdc_pack_blob;              /* 72 B */

typedef struct {
    uint64_t out_off;          /* where the pack file starts in d_out                      */
    uint32_t blob0, nblobs;    /* its blobs, in pack order: blobs[blob0 .. blob0 + nblobs) */
    uint8_t header_nonce[16];
    uint64_t size;             /* out: pack file bytes                                     */
    uint32_t header_len;       /* out: sealed header bytes (the trailing u32)              */
    uint32_t pad;
} rcdc_pack;                   /* 48 B */

/* Build npacks pack files in d_out (out_len bytes).  blobs and packs are HOST
 * arrays; blob_offsets (optional, host, nblobs) receives each blob's offset
 * in its pack (IndexBlob location.offset; its length is len + 32).  Grouping
 * blobs into packs (PackSizer, packer.rs:65-200) and the pack id (SHA-256
 * of the file, packer.rs:833) stay with the caller.  Asynchronous on
 * hip_stream; the outputs of `packs` are set on return.                     */
rcdc_status rcdc_pack_build(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                            const rcdc_pack_blob *blobs, uint32_t nblobs, rcdc_pack *packs,
                            uint32_t npacks, void *d_out, uint64_t out_len,
                            uint32_t *blob_offsets, void *hip_stream);

/* The same with blobs sealed already (packer.rs:615-655 add_raw: the packer
 * appends encrypted data): blobs[i].len is the sealed length (>= 32, nonce +
 * ciphertext + tag) of the bytes at in_off, copied into the pack as they are
 * (nonce ignored); only the headers are sealed here.                        */
rcdc_status rcdc_pack_build_raw(rcdc_ctx *ctx, const uint8_t *key, const void *d_in,
                                const rcdc_pack_blob *blobs, uint32_t nblobs, rcdc_pack *packs,
                                uint32_t npacks, void *d_out, uint64_t out_len,
                                uint32_t *blob_offsets, void *hip_stream);

/* rcdc_pack_build_raw over blobs that lie in several device buffers (sealed
 * in different passes, or carried over from an earlier call while their pack
 * was still open, packer.rs:659-671): blob i's bytes are at
 * d_ins[blobs[i].pad] + in_off; pad >= n_ins is InvalidInput.              */
rcdc_status rcdc_pack_build_raw_multi(rcdc_ctx *ctx, const uint8_t *key,
                                      const void *const *d_ins, uint32_t n_ins,
                                      const rcdc_pack_blob *blobs, uint32_t nblobs,
                                      rcdc_pack *packs, uint32_t npacks, void *d_out,
                                      uint64_t out_len, uint32_t *blob_offsets,
                                      void *hip_stream);

/* Device byte ranges gathered into one buffer: bytes [in_off, in_off + len)
 * of d_ins[src] go to out_off of d_out (any alignment).  refs is a HOST
 * array.  Returns once the copy has run (it is ordered on hip_stream).  Used
 * to keep an open pack's sealed blobs alive across ingest calls.           */
typedef struct {
    uint64_t in_off;
    uint64_t out_off;
    uint64_t len;
    uint32_t src;
    uint32_t pad;
} rcdc_copy_ref; /* 32 B */
rcdc_status rcdc_copy_ranges(rcdc_ctx *ctx, const void *const *d_ins, uint32_t n_ins,
                             const rcdc_copy_ref *refs, uint32_t n, void *d_out,
                             void *hip_stream);

/* ---- restore: decoded blobs to their file positions (commands/restore.rs
 * restore_contents, :630-668) -- what follows rcdc_aead_open /
 * rcdc_zstd_decompress there.  Blob i, bytes [in_off, in_off + len) of
 * d_ins[src], is copied to each of its destinations dests[dest0 .. dest0 +
 * ndests): bytes [out_off, out_off + len) of d_outs[dst].  Any alignment on
 * either side; a long blob is split over many workgroups (tiles of 64 KiB).
 * The blob, dest, pointer and length arrays and `zero` are HOST arrays;
 * d_ins[] / d_outs[] hold device pointers, in_lens[] / out_lens[] the sizes
 * of those buffers.
 *
 * zero (nblobs bytes, may be NULL): zero[i] = 1 when every byte of blob i is
 * 0 (SparseRestore::ByContent's `data.iter().all(|&b| b == 0)`; an empty
 * blob gives 1), else 0.  With RCDC_PLACE_SKIP_ZERO an all-zero blob is not
 * written (`if !is_sparse { write_at }`): its destination bytes keep what
 * they held.  With flags 0 and zero NULL the test is left out.
 *
 * InvalidInput, checked before anything is launched or written: src >=
 * n_ins, dst >= n_outs, dest0 + ndests > ndests_total, in_off + len >
 * in_lens[src], out_off + len > out_lens[dst], unknown flag bits, a null
 * array with a non-zero count, a null context.  Nothing outside a destination
 * range is stored; loads touch only the 16-byte-aligned granules that hold
 * source bytes.  Destination ranges that overlap each other or a source range
 * are the caller's error and are not checked (a buffer may be both a source
 * and a destination as long as the ranges are disjoint).
 *
 * Ordered on hip_stream; returns once the work has run and `zero` is filled.
 * Calls on one context take turns.  nblobs == 0 launches nothing.          */
typedef struct {
    uint64_t in_off;   /* the blob: bytes [in_off, in_off + len) of d_ins[src]      */
    uint64_t len;
    uint32_t src;      /* < n_ins                                                   */
    uint32_t dest0;    /* its destinations: dests[dest0 .. dest0 + ndests)          */
    uint32_t ndests;   /* 0 is allowed: only the zero test                          */
    uint32_t pad;
} rcdc_place_blob;     /* 32 B */
typedef struct {
    uint64_t out_off;  /* the blob goes to [out_off, out_off + len) of d_outs[dst]  */
    uint32_t dst;      /* < n_outs                                                  */
    uint32_t pad;
} rcdc_place_dest;     /* 16 B */
#define RCDC_PLACE_SKIP_ZERO 1u
rcdc_status rcdc_place_blobs(rcdc_ctx *ctx, const void *const *d_ins, const uint64_t *in_lens,
                             uint32_t n_ins, const rcdc_place_blob *blobs, uint32_t nblobs,
                             const rcdc_place_dest *dests, uint32_t ndests_total,
                             void *const *d_outs, const uint64_t *out_lens, uint32_t n_outs,
                             uint32_t flags, uint8_t *zero, void *hip_stream);

/* ---- blob compression: backend/decrypt.rs:478-506 (`encode_all(data,
 * level)` before `Key::encrypt_data` when the repository is version 2,
 * configfile.rs:177-186), applied by the packer's process_data
 * (blob/packer.rs:268-270) -- here to chunks already in HBM.  Each blob
 * becomes one zstd frame (RFC 8878) that any zstd decoder reads back (rustic's
 * decode_all, decrypt.rs:71-95); the bytes are this library's own, not
 * libzstd's (no zstd version promises another's output).               ---- */

/* One blob: bytes [in_off, in_off + len) of d_in become a frame at out_off of
 * d_out, at most rcdc_zstd_bound(len) bytes.  Any alignment. */
typedef struct {
    uint64_t in_off;
    uint64_t len;      /* < 2^32 (decrypt.rs:479-487: the length is a u32) */
    uint64_t out_off;
} rcdc_zstd_ref;

/* Worst-case frame size of a len-byte blob (header + stored blocks):
 * len + 3 per 128 KiB block + 9, + 10 above 2^27 bytes (those frames carry a
 * window descriptor: rustic's decode_all refuses windows above 2^27 + 1, and
 * a single-segment frame's window is its content size). */
uint64_t rcdc_zstd_bound(uint64_t len);

/* Compress n blobs (refs is a HOST array).  level: zstd's range
 * [-131072, 22] (0 = zstd's default, level 3: rustic's choice for version 2);
 * out-of-range -> InvalidInput.  The level picks the parse: <= 1 keys
 * positions on 6 bytes (6-byte minimum match, fastest), 2-3 on 4 bytes,
 * >= 4 also doubles the hash table to 2^12 positions (better ratio on
 * structured data, half the waves per CU).  On return (synchronous)
 * out_lens[i] (host) holds blob i's frame length.  Calls on one context take
 * turns.  The context keeps its scratch after the first call: up to 4 GiB of
 * per-block slots (batches of more than 32768 blocks run in windows) and
 * 1 GiB of per-wave sequence buffers, freed by rcdc_ctx_destroy.  A/B
 * overrides (process environment): RCDC_ZSTD_HLOG (11 / 12), RCDC_ZSTD_KEY
 * (4 / 6).                                                                  */
rcdc_status rcdc_zstd_compress(rcdc_ctx *ctx, int level, const void *d_in,
                               const rcdc_zstd_ref *refs, uint32_t n, void *d_out,
                               uint64_t *out_lens, void *hip_stream);

/* ---- frame check: backend/decrypt.rs:508-529 (`very_data`, on by default:
 * extra_verify, repofile/configfile.rs:198): after compressing a blob the
 * packer decodes it again and compares it with the input.  Here every frame
 * is decoded on the device and compared with its blob in place. ---------- */

/* Frame [frame_off, frame_off + frame_len) of d_frames is expected to decode
 * to [data_off, data_off + data_len) of d_data (allow 4 readable bytes after
 * each range). */
typedef struct {
    uint64_t frame_off;
    uint64_t frame_len;
    uint64_t data_off;
    uint64_t data_len;
} rcdc_zstd_check_ref;

/* Decode n frames (refs is a HOST array) and compare them with their blobs:
 * status[i] (host) = 0 the frame decodes to exactly the blob (RFC 8878: any
 * block and literal type, 1 or 4 Huffman streams, predefined / RLE / FSE /
 * repeat sequence tables, repeat offsets, matches into earlier blocks),
 * 1 it decodes to other bytes or another length (ErrorKind::Verification,
 * decrypt.rs:516-526), 2 malformed or not readable here (a dictionary, a
 * skippable frame, bytes after the frame).  A frame checksum is verified
 * (the low 32 bits of XXH64 of the blob, once the content compared equal);
 * a wrong one is status 2.
 * Malformed means what decode_all's decoder refuses on the path it would
 * take: one pass when the declared content size fits its first 8 KiB
 * read, otherwise the streaming stage machine (a window above 2^27 + 1
 * bytes is refused there, empty blocks of any type are skipped, every
 * block's size field and regenerated bytes are bounded by
 * min(window, 128 KiB) and every match offset by the window; the window of
 * a single-segment frame is its content size).  On either path a
 * compressed block has at least 3 bytes.  Where libzstd 1.4.8 is laxer
 * than RFC 8878 (reserved mode bits, bits left in a sequences bitstream,
 * a repeat offset resolving to 0) the RFC holds: status 2.
 * flags bit 0 (RCDC_CHECK_STORED): the "frames" are stored bytes (blobs of an
 * uncompressed repository), compared as they are.  Synchronous.  Calls on one context take turns; the context keeps a
 * 128 KiB literal scratch per resident wave (256 MiB on 256 CUs).          */
rcdc_status rcdc_zstd_check(rcdc_ctx *ctx, const void *d_frames, const void *d_data,
                            const rcdc_zstd_check_ref *refs, uint32_t n, uint32_t flags,
                            uint32_t *status, void *hip_stream);
#define RCDC_CHECK_STORED 1u

/* ---- zstd frames decompressed on the device: the read direction
 * (read_encrypted_from_partial, decrypt.rs:71-97; check_pack,
 * check.rs:718-814).  Additive entry points of ABI 5. ---------------------- */

/* Frame [frame_off, frame_off + frame_len) of d_frames decodes into
 * [out_off, out_off + out_cap) of d_out. */
typedef struct {
    uint64_t frame_off;
    uint64_t frame_len;
    uint64_t out_off;
    uint64_t out_cap;
} rcdc_zstd_dec_ref;  /* 32 B */

/* decode_all (decrypt.rs:78) for n frames in HBM.  refs, out_lens, status: HOST arrays.
 * status[i]: 0 decoded, out_lens[i] bytes written at out_off; 1 valid so far but the
 * output does not fit out_cap; 2 malformed or not readable here -- exactly the rules
 * of rcdc_zstd_check's status 2 (a frame that is malformed anywhere is 2, also when
 * its output would not fit).  Nothing outside [out_off, out_off + out_cap) is
 * ever written; on a non-zero status the bytes inside are unspecified.  Any alignment
 * (allow 4 readable bytes after the frames and the output).  flags: 0.
 * Synchronous; calls on one context take turns.  The context keeps a workspace of
 * the frames' literals and 8 bytes per sequence, at most 4 GiB at a time
 * (RCDC_ZDX_WS_MAX, bytes, overrides; frames that need more run in groups).
 * RCDC_ZDX_BLOCKS=0 decodes every frame's entropy in order (A/B). */
rcdc_status rcdc_zstd_decompress(rcdc_ctx *ctx, const void *d_frames, const rcdc_zstd_dec_ref *refs,
                                 uint32_t n, uint32_t flags, void *d_out,
                                 uint64_t *out_lens, uint32_t *status, void *hip_stream);

/* Host only (frame in host memory, no device): declared content size (UINT64_MAX if the
 * header has none), an upper bound of the decoded size from the block headers
 * (128 KiB per compressed block, exact for raw/RLE), and the block count, of the
 * first frame in [frame, frame + len).  RCDC_ERR_INVALID_INPUT for what the header
 * walk refuses: another magic, the reserved bit, a dictionary, a reserved block
 * type, a header or block past the end. */
rcdc_status rcdc_zstd_frame_info(const uint8_t *frame, uint64_t len, uint64_t *content_size,
                                 uint64_t *out_bound, uint32_t *nblocks);

/* Counters of the context's last rcdc_zstd_decompress call: [0] frames, [1] compressed
 * blocks decoded by the parallel pass, [2] compressed blocks decoded by the in-order
 * entropy pass, [3] treeless blocks resolved from an earlier block in the parallel
 * pass, [4] workspace groups, [5] peak workspace bytes; [6], [7] zero, or with
 * RCDC_ZDX_TIME=1 the microseconds of the entropy kernels and of the copy kernel
 * (HIP events, a synchronisation per group: for measuring). */
rcdc_status rcdc_zstd_decompress_stats(rcdc_ctx *ctx, uint64_t out[8]);

/* The FSE coding tables the kernels use (predefined distributions, RFC 8878
 * 3.1.1.3.2.2), copied to out (rcdc_zstd_tables_size() bytes): for tests. */
void rcdc_zstd_tables(void *out);
uint64_t rcdc_zstd_tables_size(void);

/* ---- the backup data path, host memory to host memory (ABI 4, 5) -------
 * FileArchiver::backup_reader (archiver/file_archiver.rs:144-160) for many
 * files: chunk, `hash(&chunk)`, `index.has_data`, Packer::add -- zstd at the
 * repository's level, Key::encrypt_data, extra_verify (backend/decrypt.rs:
 * 478-529) -- PackSizer / should_save (blob/packer.rs:65-200, 659-671), the
 * sealed header (:693-735) and the pack id, SHA-256 of the pack file
 * (hash_reader, :826-836).  One engine per backup (per device): the packer
 * stays open across files and batches, and rcdc_ingest_finish closes the
 * last pack (Packer::finalize, :385-398).
 *
 * Files enter page-locked input slots.  Two ways in:
 *  - a file of known size: rcdc_ingest_reserve hands out space for it (the
 *    node's size; at most batch_bytes), the caller reads the file into it
 *    (the Read of rabin.rs:110-191) and rcdc_ingest_commit hands it over
 *    (fewer bytes than reserved are fine);
 *  - any Read, of any or unknown length (a file larger than a batch, stdin,
 *    a child's stdout: commands/backup.rs:336-346): rcdc_ingest_stream_open,
 *    then pieces -- rcdc_ingest_stream_reserve + rcdc_ingest_commit, each
 *    piece any size up to batch_bytes, the stream's bytes in reservation
 *    order -- then rcdc_ingest_stream_close (EOF).  The size is only a hint
 *    (chunker.rs:22-47, size_hint): cuts never depend on how the bytes were
 *    split into pieces or batches.  The engine carries each stream's open
 *    chunk (at most max bytes) from batch to batch on the device, as
 *    rcdc_stream_feed does for the chunk-only path.
 * Reserve / commit may be called from many threads (archiver.rs:195).  A
 * reservation whose read fails is dropped with rcdc_ingest_cancel (the
 * reference logs and skips the file, archiver.rs:197-203); a stream whose
 * read fails is ended with rcdc_ingest_stream_abort (the chunks it completed
 * before the error stay packed, as the reference's Packer::add calls did).
 * A slot that fills (or whose first file is slot_max_age_ms old) becomes a
 * device batch: H2D, chunking, the short chunks' ids on the device, the long
 * ones' on host threads, zstd + seal + verify of every chunk, then (once the
 * ids are in) dedup in chunk order, packs, D2H and the pack ids on host
 * threads.  Results come back through callbacks: per file (or stream) its
 * cut offsets and chunk ids in file order (the tree's content list), per
 * pack the pack file in host memory (valid during the call), its id and its
 * index entries.  Callbacks run on the engine's threads, one at a time.
 *
 * Memory (rcdc_ingest_footprint gives the exact figures for a config):
 * page-locked in_slots x batch_bytes + out_slots x (batch_bytes + 1/16 +
 * 64 MiB) -- 16.75 GiB at the defaults (4 + 4 slots of 2 GiB) -- and on
 * the device depth x (2 x batch_bytes + max_streams x max + a sealed-blob
 * staging area of ~batch_bytes) plus two batch-sized compression / pack
 * buffers: ~30 GiB at the defaults, about a tenth of an MI355X's HBM.      */
typedef struct rcdc_ingest rcdc_ingest;

typedef struct {
    uint8_t key[64];            /* aespoly1305 Key: AES-256 || Poly1305-AES k || r     */
    int32_t zstd_level;         /* repository version 2: zstd level (0 = zstd's 3)     */
    uint32_t compress;          /* 1: version 2 compression; 0: stored blobs           */
    uint32_t extra_verify;      /* 1: decrypt, decode and compare every blob (default) */
    uint32_t hash_threads;      /* host SHA-256 threads (default 10)                   */
    uint64_t pack_size;         /* PackSizer (configfile.rs:211-231): default 32 MiB,  */
    uint64_t pack_grow_factor;  /*   grow factor 32,                                    */
    uint64_t pack_size_limit;   /*   limit u32::MAX,                                    */
    uint64_t pack_current_size; /*   the repository's data pack bytes so far           */
    uint64_t batch_bytes;       /* input slot / device batch bytes (default 2 GiB)     */
    uint32_t depth;             /* batches in flight on the device (default 4)         */
    uint32_t in_slots;          /* page-locked input slots (default 4)                 */
    uint32_t out_slots;         /* page-locked pack buffers (default 4)                */
    uint32_t max_streams;       /* streams open at once (default 16; each holds a
                                   device carry of max bytes)                          */
    uint64_t long_chunk;        /* chunks above this get their id on the host (2 MiB) */
    uint32_t pack_max_age_ms;   /* should_save's MAX_AGE (packer.rs:63,668-670): an open
                                   pack this old is saved (default 300000 = 5 min)      */
    uint32_t slot_max_age_ms;   /* an open input slot whose first file is this old is
                                   submitted unfilled (default 1000)                   */
} rcdc_ingest_config;

typedef struct {
    uint8_t id[32];
    uint32_t offset;              /* in the pack (IndexBlob location)              */
    uint32_t length;              /* sealed bytes                                  */
    uint32_t uncompressed_length; /* 0: stored as is                               */
    uint32_t type;                /* BlobType: 0 data                              */
} rcdc_ingest_blob;               /* 48 B */

typedef struct {
    const uint8_t *data;          /* the pack file (valid during the callback)     */
    uint64_t size;
    uint64_t seq;                 /* packer order                                  */
    uint8_t id[32];               /* SHA-256 of the pack file                      */
    uint32_t nblobs, header_len;
    const rcdc_ingest_blob *blobs;
} rcdc_ingest_pack;

typedef struct {
    uint64_t tag;                 /* the caller's (rcdc_ingest_commit / _stream_open) */
    uint64_t len;
    uint32_t nchunks, nnew;       /* chunks; those the packer added                */
    const uint64_t *cuts;         /* end offset of each chunk in the file          */
    const uint8_t *ids;           /* 32 B per chunk                                */
} rcdc_ingest_file_result;

typedef struct {
    uint64_t bytes_in, files, chunks, new_blobs, packs, pack_bytes, batches;
    double seconds;               /* first batch submitted .. last pack delivered  */
} rcdc_ingest_stats;

typedef void (*rcdc_ingest_pack_fn)(void *user, const rcdc_ingest_pack *pack);
typedef void (*rcdc_ingest_file_fn)(void *user, const rcdc_ingest_file_result *file);

void rcdc_ingest_config_default(rcdc_ingest_config *cfg);
/* Bytes rcdc_ingest_create allocates for cfg on ctx: page-locked host memory
 * and device memory (the engine's own buffers; the context's scratch and the
 * plans' work lists come on top).                                          */
rcdc_status rcdc_ingest_footprint(const rcdc_ctx *ctx, const rcdc_ingest_config *cfg,
                                  uint64_t *pinned_bytes, uint64_t *device_bytes);
/* Allocates the slots (page-locked and device memory for a full batch
 * each) and starts the engine's threads.  On failure nothing stays
 * allocated.                                                               */
rcdc_status rcdc_ingest_create(rcdc_ctx *ctx, const rcdc_ingest_config *cfg,
                               rcdc_ingest_pack_fn pack_cb, rcdc_ingest_file_fn file_cb,
                               void *user, rcdc_ingest **out);
/* Ids the repository's index already has (Indexer::has): before the first file. */
rcdc_status rcdc_ingest_add_index(rcdc_ingest *ing, const uint8_t *ids, uint64_t n);
/* Space for one file of len bytes (<= batch_bytes); waits for a free slot. */
rcdc_status rcdc_ingest_reserve(rcdc_ingest *ing, uint64_t len, uint8_t **buf, uint64_t *ticket);
/* The file's (or piece's) bytes are in place: its first len bytes (<= the
 * reservation).  tag: the file's (ignored for a stream piece). */
rcdc_status rcdc_ingest_commit(rcdc_ingest *ing, uint64_t ticket, uint64_t tag, uint64_t len);
/* Drop a reservation that will not be committed (its read failed): no
 * result for it, and rcdc_ingest_finish does not wait for it.  For a stream
 * piece: the piece is empty (end the stream with rcdc_ingest_stream_abort). */
rcdc_status rcdc_ingest_cancel(rcdc_ingest *ing, uint64_t ticket);
/* reserve + memcpy + commit of a file already in memory (a file larger than
 * batch_bytes goes in as a stream of pieces). */
rcdc_status rcdc_ingest_add(rcdc_ingest *ing, uint64_t tag, const void *data, uint64_t len);

/* One file (any Read) fed in pieces: ChunkIter::from_config(cfg, reader,
 * size_hint) (chunker.rs:22-47) + its iterator (rabin.rs:110-191).  size_hint
 * is only a hint (0: unknown).  Waits while max_streams streams are closing;
 * RCDC_ERR_UNSUPPORTED if max_streams are open.  *stream: the handle.      */
rcdc_status rcdc_ingest_stream_open(rcdc_ingest *ing, uint64_t tag, uint64_t size_hint,
                                    uint64_t *stream);
/* Space for the stream's next len bytes (<= batch_bytes); commit it with
 * rcdc_ingest_commit(ticket, 0, n).  Consecutive pieces of one stream that
 * land in the same slot are laid out back to back. */
rcdc_status rcdc_ingest_stream_reserve(rcdc_ingest *ing, uint64_t stream, uint64_t len,
                                       uint8_t **buf, uint64_t *ticket);
/* EOF (Ok(0), rabin.rs:164-166): the stream's last chunk ends at its last
 * byte, and its file result (all cuts and ids, in order) follows.  Every
 * piece must be committed or cancelled first.  The handle is then invalid. */
rcdc_status rcdc_ingest_stream_close(rcdc_ingest *ing, uint64_t stream);
/* The stream's read failed: the chunk in progress is dropped, no file
 * result is delivered; chunks it completed before stay packed.  The handle
 * is then invalid. */
rcdc_status rcdc_ingest_stream_abort(rcdc_ingest *ing, uint64_t stream);

/* Submit the partly filled slot now. */
rcdc_status rcdc_ingest_flush(rcdc_ingest *ing);
/* No more files: process everything, close the last pack, wait for every
 * callback; stats (optional) receives the totals.  A verification failure
 * is RCDC_ERR_VERIFICATION.  Every stream must be closed or aborted.       */
rcdc_status rcdc_ingest_finish(rcdc_ingest *ing, rcdc_ingest_stats *stats);
void rcdc_ingest_destroy(rcdc_ingest *ing);

/* ---- one dedup set for several engines (multi-device ingest) ------------
 * The reference has ONE Packer per backup, so a blob is stored once however
 * many file workers found it (archiver.rs:195, blob/packer.rs:304-315, the
 * index check of file_archiver.rs:153).  N engines -- one per GPU, fed by a
 * file router -- keep that property by sharing one id set: an engine packs
 * a chunk only if its insert into the set is the first.  The set is
 * thread-safe (sharded locks).                                             */
typedef struct rcdc_index rcdc_index;
rcdc_status rcdc_index_create(rcdc_index **out);
void rcdc_index_destroy(rcdc_index *idx);       /* after every engine using it */
/* Ids the repository already has (Indexer::has). */
rcdc_status rcdc_index_add(rcdc_index *idx, const uint8_t *ids, uint64_t n);
uint64_t rcdc_index_size(const rcdc_index *idx);
/* Dedup against idx (not the engine's own set) from now on; before the
 * engine's first batch.  Ids already given to rcdc_ingest_add_index move
 * into idx.                                                                */
rcdc_status rcdc_ingest_set_index(rcdc_ingest *ing, rcdc_index *idx);

/* ---- the blob index in device memory (index/binarysorted.rs) -------------
 * ReadIndex::has / get_id (index/binarysorted.rs:230-261) for batches of ids
 * that are already in HBM, and the packer's dedup rule (packer.rs:304-315).
 * The reference sorts 48-byte SortedEntry records and binary-searches them;
 * here the entries stay in the order added and an open-addressing table
 * finds them.  (rcdc_index above is the host dedup set of the ingest engine,
 * a different object.)
 *
 * Entries are numbered in the order added: an add of n ids gets the numbers
 * [size, size + n).  locs == NULL makes id-only entries (pack =
 * RCDC_DINDEX_NO_PACK, the other fields 0).  pack is the caller's own pack
 * number (SortedEntry::pack_idx); uncompressed_length 0 stands for None.
 *
 * One id may be added any number of times, in one call or across calls.
 * rcdc_dindex_lookup gives, per queried id, the LOWEST-numbered entry that
 * carries it, that entry's loc, and count = how many entries carry it; a
 * miss gives entry = RCDC_DINDEX_MISS, count = 0 and a zeroed loc.  (The
 * reference's binary_search leaves the choice among duplicates open; here it
 * is fixed, and it does not depend on the order in which lanes and
 * workgroups reach the table, nor on when the table grew.)
 *
 * rcdc_dindex_first_new is the packer's rule for one batch: d_new[i] = 1
 * exactly when d_select[i] != 0 (a NULL d_select selects every i), id i is
 * not in the index, and no j < i with d_select[j] != 0 has the same id;
 * otherwise d_new[i] = 0.  The index is not changed: the batch's own
 * duplicates are resolved in scratch memory that the index owns and grows
 * (blobs are indexed only once they are packed).
 *
 * Table contract: slots is a power of two, at least twice the entries; the
 * home slot of an id is the little-endian uint64 of its bytes 0..8, masked
 * with slots - 1 (SHA-256 output needs no further mixing); collisions go to
 * the next slot, wrapping.  A slot is one 64-bit word: the entry number in
 * the high half, the little-endian uint32 of id bytes 8..12 in the low half.
 * Ids crafted to collide are still answered correctly, only more slowly.
 *
 * Ordering: rcdc_dindex_add returns once the entries are in (it first waits
 * for the lookups queued on this index).  lookup and first_new enqueue on
 * hip_stream (0: the legacy default stream) and are ordered on it; their
 * outputs are valid once that stream reaches them.  Calls on one index take
 * turns.  n == 0 launches nothing.
 *
 * RCDC_ERR_INVALID_INPUT before anything is launched or touched: a null
 * index (or context / out pointer at create), a null array with n > 0
 * (d_select and locs may be null), unknown flag bits, size + n >= 2^32 - 1
 * (first_new: n >= 2^32 - 1).
 *
 * Memory: 48 bytes per entry (32 id + 16 loc, the reference's 48) in arrays
 * that grow by doubling, plus 12 bytes per slot (8 slot + 4 count) with
 * 2 to 4 slots per entry: 72 to 96 bytes per entry held, up to twice that
 * reserved right after a growth.                                           */
typedef struct rcdc_dindex rcdc_dindex;
#define RCDC_DINDEX_MISS    0xFFFFFFFFu   /* hit.entry on a miss               */
#define RCDC_DINDEX_NO_PACK 0xFFFFFFFFu   /* loc.pack of an id-only entry      */
#define RCDC_DINDEX_DEVICE_PTRS 1u        /* add: ids/locs are device pointers */
typedef struct {
    uint32_t pack, offset, length, uncompressed_length;
} rcdc_dindex_loc; /* 16 B */
typedef struct {
    uint32_t entry, count;
    rcdc_dindex_loc loc;
} rcdc_dindex_hit; /* 24 B */

/* reserve_entries: entries the arrays and the table are sized for up front. */
rcdc_status rcdc_dindex_create(rcdc_ctx *ctx, uint64_t reserve_entries, rcdc_dindex **out);
void rcdc_dindex_destroy(rcdc_dindex *dx);
uint64_t rcdc_dindex_size(const rcdc_dindex *dx); /* entries added (0 for NULL) */
uint64_t rcdc_dindex_keys(const rcdc_dindex *dx); /* distinct ids  (0 for NULL) */
/* ids: n x 32 bytes; locs: n records or NULL; host pointers unless flags has
 * RCDC_DINDEX_DEVICE_PTRS (then both are read on hip_stream).              */
rcdc_status rcdc_dindex_add(rcdc_dindex *dx, const void *ids, const rcdc_dindex_loc *locs,
                            uint64_t n, uint32_t flags, void *hip_stream);
/* d_ids: n x 32 bytes, d_hits: n records (4-byte aligned), both on the device. */
rcdc_status rcdc_dindex_lookup(rcdc_dindex *dx, const void *d_ids, uint64_t n,
                               rcdc_dindex_hit *d_hits, void *hip_stream);
/* d_select: n bytes or NULL; d_new: n bytes; all on the device. */
rcdc_status rcdc_dindex_first_new(rcdc_dindex *dx, const void *d_ids, uint64_t n,
                                  const uint8_t *d_select, uint8_t *d_new, void *hip_stream);

/* ---- index files parsed on the device (repofile/indexfile.rs) -------------
 * What every command does first (stream_all::<IndexFile> into IndexCollector,
 * index/binarysorted.rs:127-163), for index files whose decoded JSON text is
 * already in HBM: n_files refs (off, len) into one arena d_json of json_len
 * bytes.  The output is what IndexCollector's Extend<IndexPack> keeps, as
 * device arrays that go straight to rcdc_dindex_add with
 * RCDC_DINDEX_DEVICE_PTRS.
 *
 * The device parses a strict grammar G and nothing else.  A file outside G
 * is no error: its status is RCDC_IXPARSE_NOT_PARSED, it adds nothing to any
 * output, the numbering of the other files does not depend on it, and the
 * caller parses it on the host.  G (no backslash anywhere; whitespace is
 * space, \t, \n, \r, between any two tokens and around the root; trailing
 * bytes other than whitespace are outside G):
 *   root  {"supersedes": null | [id, ...], "packs": [pack, ...],
 *          "packs_to_delete": [pack, ...]}       packs required
 *   pack  {"id": id, "blobs": [blob, ...], "time": null | string,
 *          "size": null | int}                   id and blobs required
 *   blob  {"id": id, "type": "data" | "tree", "offset": int, "length": int,
 *          "uncompressed_length": null | int != 0}   the first four required
 *   id    a string of exactly 64 hex digits, either case
 *   int   decimal digits, no sign / fraction / exponent / leading zero,
 *         at most 2^32 - 1
 *   string (time)  bytes 0x20..0x7E without '"' and '\'
 * Keys come in any order, each at most once; any other key is outside G.
 *
 * Output, exactly the collector's rule: packs in file order, then in the
 * order of "packs" ("packs_to_delete" is validated and counted only).  A
 * pack goes to the type of its first blob (an empty pack to data, type 0),
 * gets the next pack number of that type counted from pack_base[type], and
 * all its blobs become entries of that type in order: d_ids[type] gets
 * 32 bytes per entry, d_locs[type] one {pack number, offset, length,
 * uncompressed_length or 0}.  d_ids[t] == NULL: entries of type t are
 * counted, not written; d_locs[t] == NULL: only the ids are written.
 * files (host, n_files records) gets the status and the counts per file,
 * packs (host) one record per collected pack in order: id, type, number and
 * pack_size() (size if present, else sum(length + 37 or 41) + 36,
 * indexfile.rs:108-112).
 *
 * Bound (rcdc_index_parse_bound): the smallest blob object of G,
 *   {"id":"<64>","type":"data","offset":0,"length":0}
 * has 109 bytes and every blob but the last of an array is followed by a
 * comma, so len bytes hold at most (len + 1) / 110 entries; the smallest
 * pack object, {"id":"<64>","blobs":[]}, has 84 bytes, so at most
 * (len + 1) / 85 packs.  cap_entries (the capacity of each of d_ids[t] and
 * d_locs[t], in entries) and cap_packs must be at least the sum of the
 * bounds over the batch's files.
 *
 * refs, files, packs, pack_base and result are host memory; the work is
 * queued on hip_stream and the call returns once it has drained.
 * RCDC_ERR_INVALID_INPUT before anything is launched: a null context, a
 * null array with n_files > 0 (d_ids / d_locs entries may be null), a ref
 * outside the arena, capacities below the bound, a bound of 2^32 - 1
 * entries or more.  n_files == 0 launches nothing.
 *
 * RCDC_IXPARSE_TILE: the structural pass works on tiles of this many bytes,
 * counted from the 16-byte boundary at or before each file's first byte.   */
#define RCDC_IXPARSE_TILE       4096u
#define RCDC_IXPARSE_OK         0u
#define RCDC_IXPARSE_NOT_PARSED 1u
typedef struct {
    uint64_t off, len;
} rcdc_ixparse_ref; /* 16 B */
typedef struct {
    uint32_t status;          /* RCDC_IXPARSE_OK / RCDC_IXPARSE_NOT_PARSED */
    uint32_t packs[2];        /* collected packs per type                   */
    uint32_t packs_to_delete; /* pack objects in "packs_to_delete"          */
    uint32_t entries[2];      /* entries per type                           */
} rcdc_ixparse_file; /* 24 B */
typedef struct {
    uint8_t id[32];
    uint32_t type, number;
    uint64_t size; /* IndexPack::pack_size() */
} rcdc_ixparse_pack; /* 48 B */
typedef struct {
    uint64_t packs[2], entries[2];
    uint64_t files_not_parsed;
} rcdc_ixparse_result; /* 40 B */

void rcdc_index_parse_bound(uint64_t len, uint64_t *max_entries, uint64_t *max_packs);
uint32_t rcdc_index_parse_tile(void); /* == RCDC_IXPARSE_TILE */
rcdc_status rcdc_index_parse(rcdc_ctx *ctx, const void *d_json, uint64_t json_len,
                             const rcdc_ixparse_ref *refs, uint32_t n_files,
                             const uint32_t pack_base[2], void *const d_ids[2],
                             rcdc_dindex_loc *const d_locs[2], uint64_t cap_entries,
                             rcdc_ixparse_file *files, rcdc_ixparse_pack *packs,
                             uint64_t cap_packs, rcdc_ixparse_result *result, void *hip_stream);

/* ---- index files written on the device (repofile/indexfile.rs) ------------
 * The reverse of rcdc_index_parse: for a batch of index files whose blobs are
 * entries in HBM, the bytes serde_json::to_vec(&IndexFile) writes, into one
 * device arena.  No byte of the text and no entry reaches the host; only the
 * per-file (off, len) and the total come back.
 *
 * Text, byte for byte (no whitespace anywhere, integers in plain decimal,
 * ids as 64 lower-case hex digits):
 *   root  {  then "supersedes":[id,...],  only when the file has a supersedes
 *         list (an empty one writes []), then "packs":[pack,...], then
 *         ,"packs_to_delete":[pack,...] only when that list is not empty, }
 *   pack  {"id":id,"blobs":[blob,...]  then ,"time":"<text>" when it has a
 *         time, then ,"size":<int> when it has a size, }
 *   blob  {"id":id,"type":"data"|"tree","offset":<int>,"length":<int>,
 *         "uncompressed_length":<int>|null}
 *         the last key is always there; an uncompressed length of 0 writes
 *         null; every blob of a pack carries the pack's type.
 *
 * Entries (device), by strides in bytes exactly as rcdc_prune_set_entries
 * takes them: entry e has its id at d_ids + e * id_stride and its uint32
 * offset, length and uncompressed length at d_offset + e * offset_stride,
 * d_len + e * len_stride, d_ulen + e * ulen_stride.  The integer arrays and
 * their strides must be 4-byte aligned; so the d_ids[t] / d_locs[t] of
 * rcdc_index_parse pass as they are.  n_entries is the arrays' length.
 *
 * packs, files, supersedes (n_supersedes x 32 bytes) and times (time_bytes
 * of text) are host memory; the call uploads them.  A pack record names its
 * entries [first, first + count); ranges may lie anywhere in the arrays and
 * one range may be written by several records.  A file record names its
 * pack records [pack_first, pack_first + pack_count), of which the last
 * n_delete are its packs_to_delete, and its supersedes ids [sup_first,
 * sup_first + sup_count) when has_supersedes is set.  A time is the bytes
 * times[time_off .. time_off + time_len): at most RCDC_IXWRITE_MAX_TIME of
 * them, each in 0x20..0x7E and neither '"' nor '\' (the string of
 * rcdc_index_parse's grammar, so what is written parses back there).
 *
 * Output: file i lies at d_out + out[i].off, out[i].len bytes, the offsets
 * 16-byte aligned and in file order (out[0].off == 0, out[i + 1].off ==
 * out[i].off + out[i].len rounded up to 16); *total is the end of the last
 * file.  out and total are host memory.  Every byte of a file is written
 * exactly once; no other byte of d_out is written, neither the gap up to the
 * next 16-byte boundary nor anything behind the last file.
 *
 * Bound (rcdc_index_write_bound): the largest blob object,
 *   {"id":"<64>","type":"data","offset":4294967295,"length":4294967295,
 *    "uncompressed_length":4294967295}
 * has 130 + 3 * 10 = 160 bytes, 161 with its comma.  The largest pack object
 * without its blobs and its time text is {"id":"<64>","blobs":[] (82 + 1),
 * ,"time":"" (10), ,"size":4294967295 (18), } (1) and a comma: 113 bytes.
 * A supersedes id is 66 bytes and a comma.  The root's own text is at most
 * {"supersedes":[], (17) "packs":[ (9) ],"packs_to_delete":[ (21) ]} (2):
 * 49 bytes, and the padding to the next file is at most 15.  So
 *   161 n_entries + 113 n_packs + time_bytes + 67 n_supersedes + 64 n_files
 * always suffices, the counts being those WRITTEN: the sum of count over
 * the pack records of all files, the sum of pack_count, of the time_len of
 * those packs, and of sup_count.  cap_out must be at least that.
 *
 * Stages, the parser's in reverse: a size pass, one lane per written entry;
 * device scans of the entry sizes, then of the pack sizes, then of the file
 * lengths into aligned offsets; an emit pass in which one wave owns a span
 * of RCDC_IXWRITE_SPAN bytes of d_out (counted from d_out, which must be
 * 16-byte aligned), its lanes format the objects that touch the span into
 * LDS at their places, and the span leaves with 16-byte stores; only a
 * file's last, ragged 16 bytes go byte by byte.
 *
 * The work is queued on hip_stream and the call returns once it has drained.
 * RCDC_ERR_INVALID_INPUT before anything is launched or written: a null
 * context, a null array with a non-zero count, out or total null, a range
 * past its array, unaligned integer arrays or strides, an unaligned d_out,
 * a type above 1, a flag other than the two below, a time outside the
 * string above, n_delete above pack_count, 2^32 - 1 written entries or pack
 * records or more, cap_out below the bound.  n_files == 0 launches nothing
 * and gives *total = 0.                                                      */
#define RCDC_IXWRITE_SPAN     8192u
#define RCDC_IXWRITE_MAX_TIME 64u
#define RCDC_IXWRITE_HAS_TIME 1u
#define RCDC_IXWRITE_HAS_SIZE 2u
typedef struct {
    uint8_t id[32];
    uint64_t first;      /* its entries are [first, first + count)        */
    uint32_t count;
    uint32_t type;       /* 0 data, 1 tree: the type every blob is given  */
    uint32_t flags;      /* RCDC_IXWRITE_HAS_TIME | RCDC_IXWRITE_HAS_SIZE */
    uint32_t size;
    uint32_t time_off, time_len; /* into times                            */
} rcdc_ixwrite_pack; /* 64 B */
typedef struct {
    uint64_t pack_first;
    uint32_t pack_count; /* pack records, packs_to_delete included        */
    uint32_t n_delete;   /* the last n_delete of them are packs_to_delete */
    uint64_t sup_first;
    uint32_t sup_count;
    uint32_t has_supersedes;
} rcdc_ixwrite_file; /* 32 B */
typedef struct {
    uint64_t off, len;
} rcdc_ixwrite_out; /* 16 B */

uint64_t rcdc_index_write_bound(uint64_t n_entries, uint64_t n_packs, uint64_t n_files,
                                uint64_t n_supersedes, uint64_t time_bytes);
uint32_t rcdc_index_write_span(void); /* == RCDC_IXWRITE_SPAN */
rcdc_status rcdc_index_write(rcdc_ctx *ctx, const void *d_ids, uint64_t id_stride,
                             const void *d_offset, uint64_t offset_stride, const void *d_len,
                             uint64_t len_stride, const void *d_ulen, uint64_t ulen_stride,
                             uint64_t n_entries, const rcdc_ixwrite_pack *packs, uint64_t n_packs,
                             const rcdc_ixwrite_file *files, uint32_t n_files,
                             const uint8_t *supersedes, uint64_t n_supersedes, const char *times,
                             uint64_t time_bytes, void *d_out, uint64_t cap_out,
                             rcdc_ixwrite_out *out, uint64_t *total, void *hip_stream);

/* ---- prune's plan on the device (commands/prune.rs) -------------------------
 * The per-blob part of PrunePlan::from_prune_options for index entries that
 * are in HBM: count_used_blobs (prune.rs:770-784), the sequential marking of
 * PackInfo::from_pack (:1495-1568) over all packs, its sums per pack, and the
 * pick of the blobs a repack keeps (:1092-1095, :1320-1321).  Thresholds, the
 * candidate sort and every decision per pack stay with the caller.
 *
 * rcdc_prune_create takes the m used ids (m x 32 bytes on the device) and
 * builds an rcdc_dindex of ids without locations over them; the USED NUMBER
 * of an id is its row.  The ids must be distinct (the reference holds them
 * in a map): a repeated id is RCDC_ERR_INVALID_INPUT.  The ids are copied.
 *
 * rcdc_prune_set_entries gives the entries: entry e has its 32 id bytes at
 * d_ids + e * id_stride, its length (uint32) at d_len + e * len_stride and
 * its uncompressed length (uint32, 0 for none) at d_ulen + e * ulen_stride;
 * strides are in bytes, so the d_ids / d_locs arrays of rcdc_index_parse
 * pass as they are (id_stride 32; &d_locs->length and
 * &d_locs->uncompressed_length with stride 16).  Lengths must be 4-byte
 * aligned.  The arrays are read, never copied to the host, and must stay
 * valid and unchanged while the handle uses them (until the next
 * set_entries or destroy).  ranges[p] = {first entry, count} is pack p, p
 * being its place in PROCESSING ORDER (prune.rs:835-842: marked packs, then
 * unmarked ones).  Ranges may lie anywhere in the arrays and must not
 * overlap; an entry outside every range does not exist for the plan.  The
 * call looks every entry id up in the used table (the join) and is ordered
 * on hip_stream.
 *
 * rcdc_prune_mark writes
 *   d_counts[j], j < m: min(entries in ranges that carry used id j, 255);
 *   d_used[e],  e < n: 1 where PackInfo::from_pack counts entry e as used,
 *                      else 0 (0 outside every range);
 *   packs[p] (host):   the PackInfo sums of pack p and whether every blob
 *                      of it has an uncompressed length (1 for an empty pack);
 *   result (host):     used ids with count 0 and the lowest such j
 *                      (RCDC_PRUNE_NONE if none), the rounds the marking
 *                      took, the entries of ids with two or more entries,
 *                      and the device time of the marking and of the sums.
 * The marking is exactly the sequential rule, on every input.  Its parallel
 * form: an id with one entry makes its pack needed at once.  For an id with
 * k >= 2 entries, sorted by processing position (rocPRIM radix sort over
 * these entries only), the first min(k, 255) are live; the pack of the last
 * live entry is needed unless an earlier pack with a live entry is; a pack
 * is not needed once every id whose last live entry it holds was taken by
 * an earlier needed pack.  One ROUND is one launch over the ids with k >= 2
 * in which each walks on through its live entries as far as the packs'
 * states are decided.  The lowest undecided pack is decided in every round,
 * so n_packs rounds are the most; the host reads one counter (ids not yet
 * settled) between rounds and gives RCDC_ERR_INTERNAL past n_packs + 1.
 * No kernel waits for a value that another lane is yet to write; pack
 * states, per-id taken words and per-pack minima are agent-scope atomics.
 * The call returns when its outputs are written (it waits for hip_stream).
 *
 * rcdc_prune_keep: kinds[p] (host) is 0, RCDC_PRUNE_KEEP (the pack is Keep
 * or Recover) or RCDC_PRUNE_REPACK; file_rank[p] (host) is the place of
 * pack p in FILE ORDER, a permutation of 0..n_packs-1.  d_keep[e] = 1 where
 * entry e is in a REPACK pack, its id is a used id, no KEEP pack holds that
 * id, and e is the first entry of the id among the REPACK packs in file
 * order; else 0.  Two passes over the entries: an atomic or of a block flag
 * and an atomic min of the file-order position per used id, then the
 * compare.  Ordered on hip_stream; d_keep is valid once it gets there.
 *
 * RCDC_ERR_INVALID_INPUT before anything is launched or written: a null
 * handle, a null array with a non-zero count, n or m >= 2^32 - 1, a range
 * past n, overlapping ranges, a pack of 65 536 entries or more (the
 * reference's u16 counts), an unaligned length array or stride, a kind above
 * 2, a file_rank that is no permutation, mark or keep before set_entries.
 *
 * Memory: 28 bytes per entry (24 the join's hit, 4 the pack number), 28 per
 * entry of an id with two or more entries while mark runs, 16 per used id
 * beside the table, 32 per pack.                                           */
typedef struct rcdc_prune rcdc_prune;
#define RCDC_PRUNE_NONE   0xFFFFFFFFu
#define RCDC_PRUNE_KEEP   1u
#define RCDC_PRUNE_REPACK 2u
#define RCDC_PRUNE_MAX_PACK_ENTRIES 65535u
typedef struct {
    uint64_t first;
    uint32_t count, pad;
} rcdc_prune_range; /* 16 B */
typedef struct {
    uint64_t used_size, unused_size;
    uint32_t used_blobs, unused_blobs;
    uint32_t compressed, pad;
} rcdc_prune_pack; /* 32 B */
typedef struct {
    uint64_t missing;        /* used ids with count 0          */
    uint64_t first_missing;  /* lowest such row, or RCDC_PRUNE_NONE */
    uint64_t dup_entries;    /* entries of ids with >= 2 entries */
    uint32_t rounds, pad;
    float mark_ms, sums_ms;  /* device time, HIP events        */
} rcdc_prune_result; /* 40 B */

rcdc_status rcdc_prune_create(rcdc_ctx *ctx, const void *d_used_ids, uint64_t m,
                              void *hip_stream, rcdc_prune **out);
void rcdc_prune_destroy(rcdc_prune *pr);
rcdc_status rcdc_prune_set_entries(rcdc_prune *pr, const void *d_ids, uint64_t id_stride,
                                   const void *d_len, uint64_t len_stride, const void *d_ulen,
                                   uint64_t ulen_stride, uint64_t n,
                                   const rcdc_prune_range *ranges, uint64_t n_packs,
                                   void *hip_stream);
rcdc_status rcdc_prune_mark(rcdc_prune *pr, uint8_t *d_counts, uint8_t *d_used,
                            rcdc_prune_pack *packs, rcdc_prune_result *result,
                            void *hip_stream);
rcdc_status rcdc_prune_keep(rcdc_prune *pr, const uint8_t *kinds, const uint32_t *file_rank,
                            uint8_t *d_keep, void *hip_stream);

/* ---- tree blobs parsed on the device (blob/tree.rs, backend/node.rs) --------
 * What find_used_blobs (commands/prune.rs:1582-1632) and TreeStreamerOnce
 * (blob/tree.rs:618-800) read out of Tree { nodes: Vec<Node> }, for a batch
 * of decoded tree blobs in HBM: n_blobs refs (off, len) into one arena d_text
 * of text_len bytes, at any alignment.  No id and no byte of the text reaches
 * the host.
 *
 * The device parses a strict grammar G_T and nothing else.  A blob outside
 * G_T is no error: its status is RCDC_TRPARSE_NOT_PARSED, it adds nothing to
 * any output, the numbering of the other blobs does not depend on it, and the
 * caller parses it on the host.  G_T (whitespace as in rcdc_index_parse's G:
 * space, \t, \n, \r between any two tokens and around the root; trailing
 * bytes other than whitespace are outside G_T):
 *   root  {"nodes": null | [node, ...]}   that key, once, and no other
 *   node  an object; each key at most once, in any order, from this set:
 *           name                                     string, required
 *           type                                     required; "file", "dir",
 *               "symlink", "dev", "chardev", "fifo" or "socket", literally
 *           mode, uid, gid                           null | int <= 2^32 - 1
 *           mtime, atime, ctime, user, group         null | string
 *           inode, device_id, size, links, device    int <= 2^64 - 1
 *           linktarget                               string; required when
 *                                                    type is "symlink"
 *           linktarget_raw                           null | string
 *           content                                  null | [id, ...]
 *           subtree                                  null | id
 *           extended_attributes   [{"name": string, "value": null | string},
 *                                  ...]  both keys at most once, name required
 *         a "dir" node without a non-null subtree is outside G_T (the
 *         reference unwraps it in find_used_blobs and reports it in
 *         check_trees: that decision stays with the host path)
 *   id      a string of exactly 64 hex digits, either case, no escapes
 *   int     decimal digits, no sign / fraction / exponent / leading zero
 *   string  a JSON string: no raw byte below 0x20; the escapes \" \\ \/ \b \f
 *           \n \r \t \uXXXX, \uD800-\uDFFF excluded (serde's surrogate pairs
 *           are not modelled); the raw bytes are well-formed UTF-8 (no
 *           overlong form, no surrogate, at most U+10FFFF)
 *   key     written literally: a key with a backslash is outside G_T
 * Nesting is the grammar's own, 5 deep; anything deeper is outside G_T.  At
 * a tile boundary of the structural pass a run of more than RCDC_TRPARSE_TILE
 * backslashes before the boundary is outside G_T (the pass looks back over
 * one tile at most to learn whether the tile's first byte is escaped).
 *
 * Where G_T is wider than the reference, and the whole list: mtime, atime and
 * ctime (RusticTime), linktarget_raw and an attribute's value (base64) are
 * checked as strings only; "device" is taken with every type.  A blob that
 * is OK here and fails there fails in one of these texts, which carry no id.
 *
 * Output.  d_data_ids: the content ids of every node whose type is "file",
 * 32 bytes each, in the order blob, node, array (the content of other types
 * is validated and dropped, as find_used_blobs' match does).  d_tree_ids:
 * the non-null subtree of every node of any type, in blob and node order
 * (TreeStreamerOnce::next follows every node.subtree), and d_tree_is_dir one
 * byte per such id: 1 where the node's type is "dir" (find_used_blobs
 * inserts only those).  d_data_ids == NULL or d_tree_ids == NULL: those ids
 * are counted, not written; d_tree_is_dir may be NULL on its own.  blobs
 * (host, n_blobs records): status, the counts, and where the blob's ids
 * start in each array.  result (host): the totals.
 *
 * Bound (rcdc_tree_parse_bound).  A content id is 66 bytes and every one but
 * the last of an array is followed by a comma, so len bytes hold at most
 * (len + 1) / 67 of them.  The smallest node with a subtree,
 *   {"name":"","type":"dir","subtree":"<64>"}
 * has 101 bytes ("dir" and "dev" are the shortest types), 102 with its
 * comma: at most (len + 1) / 102 subtree ids.  The smallest node,
 *   {"name":"","type":"dev"}
 * has 24 bytes ("dir" needs a subtree), 25 with its comma: at most
 * (len + 1) / 25 nodes.  cap_data_ids and cap_tree_ids (in ids; each checked
 * only where its array is given) must be at least the sum of the bounds over
 * the batch's blobs.
 *
 * refs, blobs and result are host memory; the work is queued on hip_stream
 * and the call returns once it has drained.  RCDC_ERR_INVALID_INPUT before
 * anything is launched: a null context, a null array with n_blobs > 0
 * (d_data_ids, d_tree_ids and d_tree_is_dir may be null), a ref outside the
 * arena, capacities below the bound, an id array that is not 16-byte
 * aligned, a batch of 2^32 - 1 bytes or more.  n_blobs == 0 launches nothing.
 *
 * RCDC_TRPARSE_TILE: the structural pass works on tiles of this many bytes,
 * counted from the 16-byte boundary at or before each blob's first byte.   */
#define RCDC_TRPARSE_TILE       4096u
#define RCDC_TRPARSE_OK         0u
#define RCDC_TRPARSE_NOT_PARSED 1u
typedef struct {
    uint64_t off, len;
} rcdc_trparse_ref; /* 16 B */
typedef struct {
    uint32_t status;     /* RCDC_TRPARSE_OK / RCDC_TRPARSE_NOT_PARSED */
    uint32_t nodes;
    uint32_t data_ids, tree_ids;
    uint64_t data_start; /* its first id in d_data_ids                  */
    uint64_t tree_start; /* its first id in d_tree_ids / d_tree_is_dir  */
} rcdc_trparse_blob; /* 32 B */
typedef struct {
    uint64_t data_ids, tree_ids, nodes;
    uint64_t blobs_not_parsed;
} rcdc_trparse_result; /* 32 B */

void rcdc_tree_parse_bound(uint64_t len, uint64_t *max_data_ids, uint64_t *max_tree_ids,
                           uint64_t *max_nodes);
uint32_t rcdc_tree_parse_tile(void); /* == RCDC_TRPARSE_TILE */
rcdc_status rcdc_tree_parse(rcdc_ctx *ctx, const void *d_text, uint64_t text_len,
                            const rcdc_trparse_ref *refs, uint32_t n_blobs, void *d_data_ids,
                            uint64_t cap_data_ids, void *d_tree_ids, uint8_t *d_tree_is_dir,
                            uint64_t cap_tree_ids, rcdc_trparse_blob *blobs,
                            rcdc_trparse_result *result, void *hip_stream);

/* ---- node records of tree blobs (commands/check.rs:627-700) ------------------
 * rcdc_tree_nodes is rcdc_tree_parse -- the same kernels, the same three id
 * outputs with the same meaning -- plus one fixed-size record per node: what
 * check_trees judges of a node, and what ls, find and diff read of a tree.
 *
 * Grammar G_N.  G_T with one rule dropped: a "dir" node whose subtree is
 * absent or null is inside G_N (check reports it as NoSubTree; it adds no
 * entry to d_tree_ids).  Everything else is G_T's, every place where G_T is
 * wider or narrower than the reference included.
 *
 * d_nodes: one rcdc_trnode per node of every OK blob, in blob and node order;
 * a NOT_PARSED blob adds none and the numbering of the others does not depend
 * on it.  The record:
 *   name_off, name_len  the raw name: the arena offset of the first byte
 *                       after its opening quote and the bytes up to its
 *                       closing quote, escapes unresolved
 *   blob                the index of the node's blob in refs
 *   data_start          the count of d_data_ids entries before this node (the
 *                       node's first content id where its type is "file";
 *                       the content of other types is not in d_data_ids)
 *   n_content           ids in "content" where it is an array, else 0
 *   tree_index          the count of d_tree_ids entries before this node: the
 *                       node's own entry where RCDC_TRNODE_SUBTREE is set
 *   type                the index in file, dir, symlink, dev, chardev, fifo,
 *                       socket
 *   flags               RCDC_TRNODE_CONTENT: "content" is an array (of
 *                       n_content ids, 0 for []); clear: absent or null.
 *                       RCDC_TRNODE_SUBTREE: "subtree" is an id; clear: absent
 *                       or null.  RCDC_TRNODE_NAME_ESC: the raw name holds a
 *                       backslash.
 * blobs: rcdc_trparse_blob's fields and node_start, the blob's first record.
 *
 * Bound: rcdc_tree_nodes_bound is rcdc_tree_parse_bound; the smallest node of
 * G_N has 24 bytes as that of G_T has, so cap_nodes (in records) must be at
 * least the sum of (len + 1) / 25 over the batch.  Refused before anything is
 * launched: what rcdc_tree_parse refuses, a null d_nodes with n_blobs > 0,
 * cap_nodes below the bound, a d_nodes that is not 16-byte aligned.          */
#define RCDC_TRNODE_CONTENT  1u
#define RCDC_TRNODE_SUBTREE  2u
#define RCDC_TRNODE_NAME_ESC 4u
typedef struct {
    uint64_t name_off;
    uint32_t name_len;
    uint32_t blob;
    uint32_t data_start;
    uint32_t n_content;
    uint32_t tree_index;
    uint8_t type;
    uint8_t flags; /* RCDC_TRNODE_* */
    uint16_t pad;
} rcdc_trnode; /* 32 B */
typedef struct {
    uint32_t status;     /* RCDC_TRPARSE_OK / RCDC_TRPARSE_NOT_PARSED */
    uint32_t nodes;
    uint32_t data_ids, tree_ids;
    uint64_t data_start, tree_start;
    uint64_t node_start; /* its first record in d_nodes */
} rcdc_trnodes_blob; /* 40 B */

void rcdc_tree_nodes_bound(uint64_t len, uint64_t *max_data_ids, uint64_t *max_tree_ids,
                           uint64_t *max_nodes);
rcdc_status rcdc_tree_nodes(rcdc_ctx *ctx, const void *d_text, uint64_t text_len,
                            const rcdc_trparse_ref *refs, uint32_t n_blobs, void *d_data_ids,
                            uint64_t cap_data_ids, void *d_tree_ids, uint8_t *d_tree_is_dir,
                            uint64_t cap_tree_ids, rcdc_trnode *d_nodes, uint64_t cap_nodes,
                            rcdc_trnodes_blob *blobs, rcdc_trparse_result *result,
                            void *hip_stream);

/* Raw names gathered: for each of the n node indices in d_index (device,
 * uint32, any order, repeats allowed) the name_len raw bytes of that record's
 * name are copied from the arena into d_names, back to back in list order.
 * d_offsets (device, n + 1 uint64, 8-byte aligned): where each name starts
 * and, last, the total, from a device scan of the lengths.  An index that is
 * not below n_nodes or a span outside the arena counts as an empty name.
 * *total (host) is the sum of the lengths; where it exceeds cap_names (or
 * d_names is NULL) the offsets are written and nothing is copied: the caller
 * comes again with room.  Nothing is unescaped.  Refused before anything is
 * launched: a null context or total, null arrays with n > 0, a misaligned
 * d_index or d_offsets.                                                     */
rcdc_status rcdc_tree_names(rcdc_ctx *ctx, const void *d_text, uint64_t text_len,
                            const rcdc_trnode *d_nodes, uint64_t n_nodes,
                            const uint32_t *d_index, uint64_t n, uint64_t *d_offsets,
                            void *d_names, uint64_t cap_names, uint64_t *total,
                            void *hip_stream);

/* A level of check_trees judged on the device (commands/check.rs:627-700).
 * In HBM: the node records of a level (rcdc_tree_nodes, of one call or of
 * several renumbered into one), d_data_ids with the hit records of a lookup
 * of them in the data index, d_tree_ids / d_tree_is_dir with the hit records
 * of a lookup in the tree index (the hits of subtrees of nodes that are no
 * "dir" and of all-zero ids are there and ignored).
 *
 * Findings, in the order check_trees emits them: nodes in order; a "file"
 * whose content is absent or null gives FILE_HAS_NO_CONTENT; one with content
 * gives, for each id i in order, FILE_BLOB_HAS_NULL_ID (the id is all zero)
 * and then FILE_BLOB_NOT_IN_INDEX (hit.count == 0 or hit.loc.pack ==
 * RCDC_DINDEX_NO_PACK; an all-zero id is looked up like any other), blob_num
 * = i; a "dir" gives NO_SUBTREE (no subtree), NULL_SUBTREE (an all-zero id)
 * or SUBTREE_MISSING_IN_INDEX, or nothing; other types give nothing.  One
 * lane per id and one per node count, two scans place, the same lanes emit: a
 * finding stands at (id findings before it) + (node findings before it).
 * *n_findings (host) is their number; where it exceeds cap_findings none is
 * written and the caller comes again with room.
 *
 * Pack marks: d_data_marks[hit.loc.pack] = 1 for every content id of a
 * "file" that is in the index, d_tree_marks likewise for every dir subtree
 * that is not all zero and is in the index; n_*_packs are the arrays'
 * lengths, a pack number past them is not marked.
 *
 * Refused before anything is launched: a null context or n_findings, a null
 * array whose count is not 0, cap_findings > 0 with null d_findings, arrays
 * not aligned (16 bytes for records and ids, 4 for hits), 2^32 - 1 or more
 * nodes or ids.                                                              */
#define RCDC_CKTREE_FILE_HAS_NO_CONTENT       0u
#define RCDC_CKTREE_FILE_BLOB_HAS_NULL_ID     1u
#define RCDC_CKTREE_FILE_BLOB_NOT_IN_INDEX    2u
#define RCDC_CKTREE_NO_SUBTREE                3u
#define RCDC_CKTREE_NULL_SUBTREE              4u
#define RCDC_CKTREE_SUBTREE_MISSING_IN_INDEX  5u
typedef struct {
    uint32_t node;     /* index of the node record */
    uint32_t kind;     /* RCDC_CKTREE_*            */
    uint32_t blob_num; /* the id's place in "content"; 0 for a node finding */
    uint32_t pad;
} rcdc_cktree_finding; /* 16 B */
rcdc_status rcdc_check_trees_level(rcdc_ctx *ctx, const rcdc_trnode *d_nodes, uint64_t n_nodes,
                                   const void *d_data_ids, const rcdc_dindex_hit *d_data_hits,
                                   uint64_t n_data_ids, const void *d_tree_ids,
                                   const uint8_t *d_tree_is_dir,
                                   const rcdc_dindex_hit *d_tree_hits, uint64_t n_tree_ids,
                                   uint8_t *d_data_marks, uint64_t n_data_packs,
                                   uint8_t *d_tree_marks, uint64_t n_tree_packs,
                                   rcdc_cktree_finding *d_findings, uint64_t cap_findings,
                                   uint64_t *n_findings, void *hip_stream);

/* ---- the verdict of `repair snapshots` (commands/repair/snapshots.rs,
 * blob/tree/modify.rs) ---------------------------------------------------------
 * Every distinct tree id of the walk has a slot: its entry number in an
 * id-only rcdc_dindex, which rcdc_dindex_lookup returns as hit.entry.  A tree
 * is damaged where the repair rule rewrites it for a reason of its own: a
 * "file" node with a content id the data index lacks (hit.count == 0 or
 * hit.loc.pack == RCDC_DINDEX_NO_PACK; an all-zero id is looked up like any
 * other), or a "dir" node without a subtree.  It is changed where it is
 * damaged or a tree under one of its "dir" nodes is changed.
 *
 * rcdc_repair_trees_level, one call per batch of rcdc_tree_nodes.  In HBM:
 * the node records; the hit records of d_data_ids in the data index; the hit
 * records of d_tree_ids in the id-only set of the walk, looked up after the
 * subtrees of this batch's "dir" nodes are in it; d_tree_is_dir; d_blob_slot,
 * the slot of each blob of the batch.  It writes d_damaged[slot] = 1 (plain
 * byte stores; nothing else of d_damaged is touched) for the blob of every
 * damaged node, and one edge per entry of d_tree_ids at the entry's place:
 * (slot of the node's blob, hit.entry of the subtree) for the subtree of a
 * "dir" node, (RCDC_REPAIR_NO_EDGE, RCDC_REPAIR_NO_EDGE) for that of any other
 * type, for a subtree the set lacks and for a blob or subtree slot not below
 * n_slots.  *result (host): the content ids of "file" nodes that the index
 * lacks, the damaged nodes, the "file" nodes whose content is absent or null
 * and the lowest index of such a node (RCDC_REPAIR_NO_NODE where there is
 * none); the reference panics on such a node, so the caller refuses the run.
 * A lane per id finds its node by a search over data_start, a lane per node
 * does the rest; no lane loops over a node's ids.
 *
 * rcdc_repair_spread.  d_changed becomes the least fixed point of
 * changed[p] |= changed[c] over the n_edges edges (p, c), starting from
 * d_damaged (the two may be the same array): rounds of one kernel, a lane per
 * edge, until a round sets nothing.  Edges with an end not below n_slots (so
 * RCDC_REPAIR_NO_EDGE) are skipped.  It ends on any edge list, cycles
 * included, after at most n_slots + 1 rounds.  *rounds (host): the rounds up
 * to and including the first that set nothing (0 without edges or slots);
 * RCDC_REPAIR_SPREAD_ROUNDS rounds are launched between two reads of their
 * "set something" words.
 *
 * Refused before anything is launched: a null context, result or rounds, a
 * null array whose count is not 0, arrays not aligned (16 bytes for records, 8
 * for edges, 4 for hits and slots), 2^32 - 1 or more of anything counted.     */
#define RCDC_REPAIR_NO_EDGE 0xFFFFFFFFu
#define RCDC_REPAIR_NO_NODE 0xFFFFFFFFFFFFFFFFull
#define RCDC_REPAIR_SPREAD_ROUNDS 8u
typedef struct {
    uint32_t parent, child; /* slots */
} rcdc_repair_edge; /* 8 B */
typedef struct {
    uint64_t missing_ids;
    uint64_t damaged_nodes;
    uint64_t files_without_content;
    uint64_t first_without_content; /* a node index, or RCDC_REPAIR_NO_NODE */
} rcdc_repair_level_result; /* 32 B */
rcdc_status rcdc_repair_trees_level(rcdc_ctx *ctx, const rcdc_trnode *d_nodes, uint64_t n_nodes,
                                    const rcdc_dindex_hit *d_data_hits, uint64_t n_data_ids,
                                    const uint8_t *d_tree_is_dir,
                                    const rcdc_dindex_hit *d_tree_hits, uint64_t n_tree_ids,
                                    const uint32_t *d_blob_slot, uint64_t n_blobs,
                                    uint8_t *d_damaged, uint64_t n_slots,
                                    rcdc_repair_edge *d_edges, rcdc_repair_level_result *result,
                                    void *hip_stream);
rcdc_status rcdc_repair_spread(rcdc_ctx *ctx, const rcdc_repair_edge *d_edges, uint64_t n_edges,
                               const uint8_t *d_damaged, uint8_t *d_changed, uint64_t n_slots,
                               uint64_t *rounds, void *hip_stream);
uint32_t rcdc_repair_spread_rounds_per_launch(void); /* RCDC_REPAIR_SPREAD_ROUNDS */

/* ---- pack headers parsed on the device (repofile/packfile.rs) --------------
 * What PackHeader::from_binary (packfile.rs:88-242) reads out of the table at
 * the end of a pack, for a batch of opened (plaintext) headers in HBM:
 * n_headers refs (off, len) into one arena d_plain of plain_len bytes, at any
 * alignment.  The output is what IndexCollector keeps of the packs, in the
 * layout of rcdc_index_parse, so it goes the same way to rcdc_dindex_add and
 * rcdc_index_write as device pointers; no entry and no id reaches the host.
 *
 * The format.  Entries follow each other from byte 0; integers are little
 * endian:
 *   type byte 0 (data), 1 (tree)   37 bytes: u32 length, id[32]
 *   type byte 2 (data), 3 (tree)   41 bytes: u32 length,
 *                                  u32 uncompressed_length, id[32]
 * The blob type is type & 1, the offset of an entry the sum of the lengths
 * before it, and an uncompressed length of 0 in a 41-byte entry is kept as 0
 * (NonZeroU32::new gives None).
 *
 * Status per header:
 *   RCDC_PKHDR_OK
 *   RCDC_PKHDR_BAD_TYPE   a type byte above 3 at an entry start (checked
 *                         before the entry's size)
 *   RCDC_PKHDR_CUT_SHORT  the last entry has fewer bytes than its size
 *   RCDC_PKHDR_OVERFLOW   neither of those, and the running offset after some
 *                         entry, the last included, exceeds 2^32 - 1 (the
 *                         reference's offset += length is a u32 add)
 * A header whose status is not OK is no error of the call: it adds nothing
 * to any output and the numbering of the other headers does not depend on
 * it; of its record only status, err_entry and err_pos (BAD_TYPE and
 * CUT_SHORT: the offending entry's index and its byte position in the
 * header) are set, the rest is 0.  len == 0 is OK: an empty pack, type data.
 *
 * Output, the collector's rule as in rcdc_index_parse: a header goes to the
 * type of its first entry (an empty one to data), gets the next pack number
 * of that type counted from pack_base[type] (only OK headers count), and all
 * its entries become entries of that type in order: d_ids[type] gets
 * 32 bytes per entry, d_locs[type] one {pack number, offset, length,
 * uncompressed_length or 0}.  d_ids[t] == NULL: entries of type t are
 * counted, not written; d_locs[t] == NULL: only the ids are written.
 * headers (host, n_headers records): status, type and number, the first
 * entry in the type's arrays and the count, how many of the entries are data
 * and how many tree (a header with both is mixed: its entries are written
 * under the first one's type all the same, and the caller decides),
 * PackHeaderRef::size() = 32 + the entries' bytes and
 * PackHeaderRef::pack_size() = 36 + sum(length + entry bytes)
 * (packfile.rs:355-372).  result (host): the totals.
 *
 * Bound (rcdc_pack_header_parse_bound): an entry has at least 37 bytes, so
 * len bytes hold at most len / 37.  cap_entries (the capacity of each of
 * d_ids[t] and d_locs[t], in entries) must be at least the sum of the bounds
 * over the batch's headers.
 *
 * refs, headers, pack_base and result are host memory; the work is queued on
 * hip_stream and the call returns once it has drained.
 * RCDC_ERR_INVALID_INPUT before anything is launched: a null context, a null
 * array with n_headers > 0 (d_ids / d_locs entries may be null), a ref
 * outside the arena, a capacity below the bound, an entry array that is not
 * 16-byte aligned, a bound of 2^32 - 1 entries or more.  n_headers == 0
 * launches nothing.
 *
 * RCDC_PKHDR_TILE: the passes work on tiles of this many bytes, counted from
 * the 16-byte boundary at or before each header's first byte.               */
#define RCDC_PKHDR_TILE      2048u
#define RCDC_PKHDR_OK        0u
#define RCDC_PKHDR_BAD_TYPE  1u
#define RCDC_PKHDR_CUT_SHORT 2u
#define RCDC_PKHDR_OVERFLOW  3u
typedef struct {
    uint64_t off, len;
} rcdc_pkhdr_ref; /* 16 B */
typedef struct {
    uint32_t status;     /* RCDC_PKHDR_*                                   */
    uint32_t type;       /* of its first entry; 0 for an empty header      */
    uint32_t number;     /* its pack number in that type                   */
    uint32_t count;      /* entries                                        */
    uint64_t first;      /* its first entry in d_ids[type] / d_locs[type]  */
    uint32_t data, tree; /* entries of each blob type: both != 0 is mixed  */
    uint64_t size;       /* PackHeaderRef::size()                          */
    uint64_t pack_size;  /* PackHeaderRef::pack_size()                     */
    uint64_t err_pos;    /* BAD_TYPE / CUT_SHORT: the entry's first byte   */
    uint32_t err_entry;  /* and its index                                  */
    uint32_t pad;
} rcdc_pkhdr_header; /* 64 B */
typedef struct {
    uint64_t packs[2], entries[2];
    uint64_t headers_not_parsed;
} rcdc_pkhdr_result; /* 40 B */

uint64_t rcdc_pack_header_parse_bound(uint64_t len); /* len / 37 */
uint32_t rcdc_pack_header_parse_tile(void);          /* == RCDC_PKHDR_TILE */
rcdc_status rcdc_pack_header_parse(rcdc_ctx *ctx, const void *d_plain, uint64_t plain_len,
                                   const rcdc_pkhdr_ref *refs, uint32_t n_headers,
                                   const uint32_t pack_base[2], void *const d_ids[2],
                                   rcdc_dindex_loc *const d_locs[2], uint64_t cap_entries,
                                   rcdc_pkhdr_header *headers, rcdc_pkhdr_result *result,
                                   void *hip_stream);

/* ---- check's index pass and header compare on the device (commands/check.rs) -
 * What check_packs does per pack with the blobs an index lists for it
 * (check.rs:484-507) and what check_pack compares with the pack's own header
 * (check.rs:779-786), for a batch of packs whose index entries are in HBM.
 *
 * Entries (device), by strides in bytes exactly as rcdc_prune_set_entries
 * takes them: entry e has its 32 id bytes at d_ids + e * id_stride and its
 * offset, length and uncompressed length (uint32 each, 0 for none) at
 * d_off + e * off_stride, d_len + e * len_stride, d_ulen + e * ulen_stride,
 * so the d_ids / d_locs arrays of rcdc_index_parse and of
 * rcdc_pack_header_parse pass as they are (&d_locs->offset, ->length,
 * ->uncompressed_length with stride 16; such records on a 16-byte boundary
 * are read with one 16-byte load each, ids with stride 32 on a 16-byte
 * boundary with two).  d_types: one byte per entry (0 data, 1 tree), or NULL:
 * every entry has its pack's type, which is then the header's where a header
 * is given and data otherwise.  ranges[p] = {first entry, count} is pack p;
 * ranges may lie anywhere in the arrays and must not overlap; count is any
 * uint32 (check has no 65 535 cap).  The arrays are read, never copied to the
 * host.
 *
 * The header side, optional (hdrs == NULL: none): d_hdr_ids[t] / d_hdr_locs[t]
 * are the outputs of rcdc_pack_header_parse, hdr_entries[t] the entries
 * written to each, and hdrs[p] = {type, count, first} is taken from the
 * rcdc_pkhdr_header record of pack p's header: its entries are the rows
 * [first, first + count) of type's arrays and all have that type (a mixed
 * header is the caller's).  type == RCDC_CKPACK_NO_HEADER: nothing to compare
 * for this pack.
 *
 * The rule per pack.  Its type is its first entry's IN INPUT ORDER
 * (blob_type() is read before the sort; an empty pack is data).  Its entries
 * are put in the order of (offset, length, uncompressed_length) -- IndexBlob's
 * cmp is BlobLocation's derived order; id and type take no part in it.
 * Entries with equal locations keep their input order: the reference's
 * sort_unstable leaves that open, so in an index that lists two blobs at one
 * place, and only there, which blob_id a finding names may differ from the
 * reference's.  Then with expected = 0, per entry in that order: a TYPE
 * finding where its type is not the pack's, an OFFSET finding where its
 * offset is not expected, and expected += length as a wrapping uint32 add
 * (what a release build of the reference does; a debug build panics there).
 *
 * A pack whose entries are already non-decreasing needs no sort and is taken
 * at any count.  One out of order is sorted in LDS up to
 * RCDC_CKPACK_SORT_MAX entries.  Above that its status is RCDC_CKPACK_HOST:
 * it adds nothing to any output (of its record only status and type are set),
 * the numbering of the other packs' findings does not depend on it, and the
 * caller applies the rule on the host.
 *
 * Output.  packs (host, n_packs records): status, type, the two finding
 * counts, the end offset (expected after the last entry), header_len = 32 +
 * sum(41 with an uncompressed length, else 37), which is
 * PackHeaderRef::from_index_pack(..).size() as u64, the header verdict
 * (NOT_COMPARED, EQUAL, DIFFERS), the first sorted position at which the two
 * sides differ (the shorter count when one side is a prefix of the other;
 * 0 unless DIFFERS) and where the pack's findings start.  EQUAL holds exactly
 * when the counts agree and at every sorted position the id (all 32 bytes),
 * offset, length, uncompressed length (0 and none the same) and the entry's
 * type and the header's agree.  d_findings (device, cap_findings records, may
 * be NULL with cap_findings 0): {pack, entry (its index in the arrays), kind,
 * got, expected} -- TYPE: the entry's and the pack's type, OFFSET: the
 * entry's and the expected offset -- in the reference's order: pack, sorted
 * position, TYPE before OFFSET.  Counted, scanned, then written: the order
 * does not depend on timing.  Records past cap_findings are not written; the
 * counts and result->findings are right all the same.  d_order (device, n
 * uint32, or NULL): d_order[first + k] is the entry at sorted position k of
 * the pack that starts at first; rows outside every OK pack are not written.
 *
 * One launch over the packs (judge and count, a workgroup per pack), then
 * sort and emit, each over a scanned list of the packs it has work for (those
 * out of order; those with findings, a header or the order to write) with a
 * grid that does not grow with the packs, and one scan of the counts.  No
 * kernel waits for a value another lane has yet to write.  ranges, hdrs, hdr_entries, packs and result are
 * host memory; the work is queued on hip_stream and the call returns once it
 * has drained.  Calls on one context take turns.
 *
 * RCDC_ERR_INVALID_INPUT before anything is launched: a null context or
 * result, a null array with a non-zero count (d_types, d_findings, d_order
 * and hdrs may be null), n >= 2^32 - 1, a stride smaller than its element,
 * offset / length arrays or strides that are not 4-byte aligned, a range past
 * n, overlapping ranges, a header type above 1 that is not the marker, a
 * header range past hdr_entries, a header array that is not 16-byte aligned.
 * n_packs == 0 launches nothing.                                           */
#define RCDC_CKPACK_SORT_MAX     4096u  /* 16 B of key and index each: 64 KiB of LDS */
#define RCDC_CKPACK_OK           0u
#define RCDC_CKPACK_HOST         1u
#define RCDC_CKPACK_NOT_COMPARED 0u
#define RCDC_CKPACK_EQUAL        1u
#define RCDC_CKPACK_DIFFERS      2u
#define RCDC_CKPACK_TYPE         0u     /* finding kinds */
#define RCDC_CKPACK_OFFSET       1u
#define RCDC_CKPACK_NO_HEADER    0xFFFFFFFFu
typedef struct {
    uint32_t type;  /* 0, 1 or RCDC_CKPACK_NO_HEADER */
    uint32_t count;
    uint64_t first; /* in d_hdr_ids[type] / d_hdr_locs[type] */
} rcdc_ckpack_hdr; /* 16 B */
typedef struct {
    uint32_t status;          /* RCDC_CKPACK_OK / _HOST            */
    uint32_t type;            /* of the first entry in input order */
    uint32_t type_findings, offset_findings;
    uint32_t end_offset;
    uint32_t header_verdict;  /* NOT_COMPARED / EQUAL / DIFFERS    */
    uint32_t header_diff;     /* first differing sorted position   */
    uint32_t sorted;          /* 1: the entries were in order      */
    uint64_t header_len;
    uint64_t first_finding;   /* in d_findings                     */
} rcdc_ckpack_pack; /* 48 B */
typedef struct {
    uint32_t pack, entry, kind, got, expected;
} rcdc_ckpack_finding; /* 20 B */
typedef struct {
    uint64_t findings;    /* of all OK packs, written or not */
    uint64_t packs_host;  /* packs with status HOST          */
    uint64_t packs_sorted_on_device;
} rcdc_ckpack_result; /* 24 B */

uint32_t rcdc_check_packs_sort_max(void); /* == RCDC_CKPACK_SORT_MAX */
rcdc_status rcdc_check_packs(rcdc_ctx *ctx, const void *d_ids, uint64_t id_stride,
                             const void *d_off, uint64_t off_stride, const void *d_len,
                             uint64_t len_stride, const void *d_ulen, uint64_t ulen_stride,
                             const uint8_t *d_types, uint64_t n,
                             const rcdc_prune_range *ranges, uint64_t n_packs,
                             const void *const d_hdr_ids[2],
                             const rcdc_dindex_loc *const d_hdr_locs[2],
                             const uint64_t hdr_entries[2], const rcdc_ckpack_hdr *hdrs,
                             rcdc_ckpack_pack *packs, rcdc_ckpack_finding *d_findings,
                             uint64_t cap_findings, uint32_t *d_order,
                             rcdc_ckpack_result *result, void *hip_stream);

/* Page-locked and device bytes currently held by all ingest engines of the
 * process (their own buffers, as rcdc_ingest_footprint counts them).        */
void rcdc_ingest_mem_live(uint64_t *pinned_bytes, uint64_t *device_bytes);

/* SHA-256 of one host buffer on the calling thread (SHA extensions when the
 * CPU has them): a pack id (packer.rs:832-834) where latency matters.      */
rcdc_status rcdc_sha256_host_one(const void *data, uint64_t len, uint8_t *digest);
/* SHA-256 of n host buffers on the calling thread, up to `ways` (1-4) of
 * them interleaved on the SHA extensions (one message's rounds are one
 * dependency chain; independent chains fill the unit's idle cycles): more
 * bytes per second per core than rcdc_sha256_host_one at about the same
 * latency per buffer.  Without SHA extensions: one buffer at a time.       */
rcdc_status rcdc_sha256_host_ni(const void *const *ptrs, const uint64_t *lens, uint32_t n,
                                uint32_t ways, uint8_t *digests);

/* ABI version of the loaded library (== RCDC_ABI_VERSION). */
uint32_t rcdc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RCDC_H */
