// rcdc_launch.h -- the launch and sizing functions of the kernel units, as
// the host units (rcdc_runtime.cpp, the family units, rcdc_ingest.cpp) call them.  Every
// defining .hip file includes this header too, so a signature that drifts is
// a compile error in the defining unit, not a link error.
#pragma once
#include <hip/hip_runtime.h>

#include "rcdc_internal.h"

namespace rcdc {

// ---- rcdc_scan.hip
int scan_threads(int code);
hipError_t launch_scan(int code, const uint8_t *arena, const ScanItem *items, uint32_t nitems,
                       const uint64_t *gtab, const ScanParams &prm, uint4 *sums,
                       uint64_t *item_masks, uint32_t blocks, hipStream_t stream);
hipError_t launch_plan_set_len(StreamDesc *sds, ScanItem *items, uint32_t nitems, uint64_t n,
                               uint64_t nseg, hipStream_t stream);

// ---- rcdc_resolve.hip
hipError_t launch_window(const uint64_t *cuts, const uint64_t *counts, uint32_t stream,
                         uint64_t base, uint64_t bound, uint32_t k, uint64_t *out,
                         hipStream_t hs);
hipError_t launch_resolve(const uint8_t *arena, const StreamDesc *sds, const ResolveUnit *units,
                          uint32_t nunits, const StitchDesc *stitches, uint32_t nstitch,
                          const uint64_t *gtab, const ResolveParams &prm, const uint4 *sums,
                          const uint64_t *item_masks, uint64_t *cuts, uint64_t *counts,
                          uint64_t *piece_cuts, uint64_t *piece_counts, uint64_t *stats,
                          hipStream_t stream);

// ---- rcdc_walk.hip
hipError_t launch_walk_order(const uint8_t *arena, const StreamDesc *sds, const WalkUnit *units,
                             const WalkParams &prm, hipStream_t stream);
hipError_t launch_walk(const uint8_t *arena, const StreamDesc *sds, const WalkUnit *units,
                       const WalkParams &prm, const uint64_t *gtab, uint64_t *piece_cuts,
                       uint64_t *pstatus, uint32_t *ctr, uint32_t blocks, hipStream_t stream,
                       bool ordered);
hipError_t launch_walk_chain(const uint8_t *arena, const StreamDesc *sds, const WalkUnit *units,
                             const uint32_t *stream_unit0, uint32_t nstreams,
                             const WalkParams &prm, const uint64_t *gtab,
                             const uint64_t *piece_cuts, const uint64_t *pstatus, BoundRes *bres,
                             uint32_t *ctr, uint32_t *fixlist, uint64_t *fix_cuts,
                             FixRes *fixres, uint64_t *cuts, uint64_t *counts,
                             uint32_t fix_blocks, uint32_t chk_cap, hipStream_t stream,
                             bool wide);

// ---- rcdc_sha256.hip
hipError_t launch_sha256_list(const uint8_t *arena, const ulonglong2 *refs, uint32_t n,
                              uint32_t *digests, hipStream_t stream);
hipError_t launch_sha256_plan(const uint8_t *arena, const StreamDesc *sds, uint32_t nstreams,
                              const uint64_t *cuts, const uint64_t *counts, uint64_t nslots,
                              uint64_t max_len, uint32_t *bwork, uint32_t *order,
                              uint32_t *digests, hipStream_t stream);
hipError_t launch_sha256_multi(uint32_t n, const uint8_t *const *arenas,
                               const StreamDesc *const *sds, const uint32_t *nstreams,
                               const uint64_t *const *cuts, const uint64_t *const *counts,
                               const uint64_t *nslots, uint64_t max_len, uint32_t *const *bwork,
                               uint32_t *const *order, uint32_t *const *digests,
                               hipStream_t stream);

// ---- rcdc_aead.hip
hipError_t launch_aead(bool open, const uint8_t *in, uint8_t *out, const AeadBlob *blobs,
                       uint32_t nblobs, const AeadUnit *units, uint32_t nunits,
                       const uint32_t *unit0, const AeadKeyDev *key, uint32_t *partials,
                       uint32_t *status, uint32_t cus, hipStream_t stream);

// ---- rcdc_zstd.hip
void zstd_prof_dump();
uint64_t zstd_far_words(int level, uint64_t nblk);
uint32_t zstd_block_grid(uint32_t cus, int level);
hipError_t launch_zstd(const uint8_t *in, uint8_t *out, const ZstdBlob *blobs, uint32_t nblobs,
                       const ZstdBlk *blks, uint32_t nblk, const ZstdTables *tabs, uint8_t *slots,
                       uint64_t *seqbuf, uint32_t grid, uint2 *res, uint64_t *bpos,
                       uint64_t *out_lens, uint32_t *queue, uint32_t *far, int level,
                       hipStream_t stream);

// ---- rcdc_zstd_dec.hip
uint64_t zstd_check_scratch_bytes(uint32_t grid);
void zstd_check_prof_dump();
uint64_t zstd_blkdesc_bytes();
uint32_t zstd_check_waves_per_cu();
hipError_t launch_zstd_check(const uint8_t *frames, const uint8_t *data, const void *refs,
                             const uint32_t *order, uint32_t n, bool stored, uint8_t *scratch,
                             uint32_t grid,
                             uint32_t *status, uint32_t *ctr, hipStream_t stream);
hipError_t launch_zstd_check_blocks(const uint8_t *frames, const uint8_t *data, const void *refs,
                                    const uint64_t *blk0, uint32_t n, void *blks, uint64_t nblk,
                                    uint8_t *scratch, uint32_t grid, uint32_t *status,
                                    uint32_t *ctr, hipStream_t stream);
hipError_t launch_stream_copy(void *dst, const void *src, uint64_t len, uint32_t blocks,
                              hipStream_t stream);
hipError_t launch_copy_ranges(uint8_t *out, const void *units, uint32_t n, uint32_t cus,
                              hipStream_t stream);

// ---- rcdc_zstd_dx.hip
uint32_t zdx_waves_per_cu();
hipError_t launch_zdx_blocks(const uint8_t *frames, const void *refs, uint32_t n, bool write,
                             bool all_in_order, const ZdxPlace *place, const ZdxLayout &lay,
                             uint8_t *ws, ZdxFrame *frm, hipStream_t stream);
hipError_t launch_zdx_entropy(const uint8_t *frames, const ZdxFrame *frm, const ZdxLayout &lay,
                              uint8_t *ws, uint64_t nblk, uint32_t grid, uint32_t *ctr,
                              hipStream_t stream);
hipError_t launch_zdx_inorder(const uint8_t *frames, const ZdxFrame *frm, const ZdxPlace *place,
                              const uint32_t *list, uint32_t nlist, const ZdxLayout &lay, uint8_t *ws,
                              uint32_t grid, uint32_t *ctr, hipStream_t stream);
hipError_t launch_zdx_copy(const uint8_t *frames, const void *refs, const ZdxFrame *frm,
                           const ZdxPlace *place, const uint32_t *order, uint32_t nlist,
                           const ZdxLayout &lay, uint8_t *ws, uint8_t *d_out, uint64_t *out_lens,
                           uint32_t *status, uint32_t grid, uint32_t *ctr, hipStream_t stream);

}  // namespace rcdc
