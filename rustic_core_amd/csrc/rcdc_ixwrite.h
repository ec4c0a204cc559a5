// rcdc_index_write: what the host half (rcdc_ixwrite.cpp) and the kernels
// (rcdc_ixwrite.hip) share.  Included by those two units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rcdc.h"

namespace rcdc {

constexpr uint32_t kIxwSpan = RCDC_IXWRITE_SPAN;  // bytes of d_out per wave of the emit pass
constexpr uint32_t kIxwChunks = kIxwSpan / 16;    // 16-byte stores per span
constexpr uint32_t kIxwBlock = 256;               // the per-entry and per-pack passes

// the text's fixed parts (rcdc.h)
constexpr uint32_t kIxwBlobFixed = 130;  // a blob object without its three values
constexpr uint32_t kIxwBlobMax = 161;    // with 3 x 10 digits and its comma
constexpr uint32_t kIxwPackHead = 82;    // {"id":"<64>","blobs":[
constexpr uint32_t kIxwPackMax = 113;    // head, comma, ,"time":"", ,"size":<10>, ]}
constexpr uint32_t kIxwSupId = 67;       // "<64>" and a comma
constexpr uint32_t kIxwRootMax = 49;
constexpr uint32_t kIxwMid = 21;         // ],"packs_to_delete":[

// IxwPack::flags
constexpr uint32_t kIxwTime = RCDC_IXWRITE_HAS_TIME, kIxwSize = RCDC_IXWRITE_HAS_SIZE;
constexpr uint32_t kIxwTree = 4;    // its blobs are "tree"
constexpr uint32_t kIxwComma = 8;   // not the first of its array: a comma leads it
constexpr uint32_t kIxwDelete = 16; // in "packs_to_delete"

// A written pack.  The host lays these out in output order: file by file, a
// file's packs, then its packs_to_delete.
struct IxwPack {
    uint32_t id[8];
    uint64_t first;
    uint32_t count, flags, size, time_off, time_len, file;
};  // 64 B
struct IxwFile {
    uint32_t pack_a, pack_b;  // its written packs
    uint32_t n_delete, has_sup, sup_first, sup_count;
    uint32_t head_len;        // { ["supersedes":[...],] "packs":[
    uint32_t mid_len;         // kIxwMid when n_delete, else 0
};  // 32 B

struct IxwArgs {
    // entries (device, strided)
    const uint8_t *ids, *off, *len, *ulen;
    uint64_t id_stride, off_stride, len_stride, ulen_stride;
    // device copies of the host's tables
    const IxwPack *packs;
    const uint32_t *wfirst;  // n_packs + 1: written entries before pack p
    const IxwFile *files;
    const uint8_t *sup;      // 32 B per id
    const uint8_t *times;
    uint32_t n_packs, n_files, n_written, n_spans;
    // scratch
    uint32_t *sizes;   // n_written + 1: bytes of entry w, its comma included; then 0
    uint64_t *epos;    // n_written + 1: the exclusive scan of sizes
    uint64_t *psize;   // n_packs + 1: bytes of pack p, its comma included; then 0
    uint64_t *ppos;    // n_packs + 1: the exclusive scan of psize
    uint64_t *pabs;    // n_packs: where pack p begins in d_out (at its comma)
    uint64_t *ebase;   // n_packs: entry w of pack p begins at ebase[p] + epos[w]
    void *scan_tmp;
    size_t scan_tmp_bytes;
    // outputs (device)
    rcdc_ixwrite_out *fout;  // n_files
    uint64_t *total;
    uint8_t *out;
};

// temporary storage the two scans need for up to n elements
hipError_t ix_write_scan_bytes(uint64_t n, size_t *bytes);
hipError_t launch_ix_write(const IxwArgs &a, hipStream_t st);

}  // namespace rcdc
