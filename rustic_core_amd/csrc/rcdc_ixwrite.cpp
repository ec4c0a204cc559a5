// rcdc_index_write (include/rcdc.h): the host half -- argument checks, the
// written packs laid out in output order with their entry prefix, scratch
// memory and the order of the launches.  The kernels are in
// rcdc_ixwrite.hip.
//
// Everything is checked before the first HIP call, and the capacity against
// the bound, so no kernel can write past d_out.  The call stops the stream
// once, at the end, to hand the per-file (off, len) and the total to the
// caller.  Scratch lives for one call.

#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>
#include <vector>

#include "rcdc_host.h"
#include "rcdc_ixwrite.h"

using namespace rcdc;

namespace {

// The device memory of one call: one allocation, carved up.  (One
// allocation because hipFree waits for the device each time.)
struct CarvedScratch {
    uint8_t *base = nullptr;
    uint64_t used = 0;
    std::vector<std::pair<void **, uint64_t>> parts;
    ~CarvedScratch() {
        if (base) (void)hipFree(base);
    }
    template <class T>
    void want(T **out, uint64_t n) {
        parts.emplace_back((void **)out, used);
        used += ((n ? n : 1) * sizeof(T) + 255u) & ~255ull;
    }
    hipError_t alloc() {
        const hipError_t e = hipMalloc((void **)&base, used);
        if (e == hipSuccess)
            for (auto &p : parts) *p.first = base + p.second;
        return e;
    }
};

constexpr uint64_t kMaxCount = 0xFFFFFFFFull;  // written entries and packs stay below it
constexpr uint64_t kMaxSup = 1ull << 24;       // supersedes ids of one file

}  // namespace

extern "C" {

uint64_t rcdc_index_write_bound(uint64_t n_entries, uint64_t n_packs, uint64_t n_files,
                                uint64_t n_supersedes, uint64_t time_bytes) {
    return (uint64_t)kIxwBlobMax * n_entries + (uint64_t)kIxwPackMax * n_packs + time_bytes +
           (uint64_t)kIxwSupId * n_supersedes + (kIxwRootMax + 15ull) * n_files;
}

uint32_t rcdc_index_write_span(void) { return RCDC_IXWRITE_SPAN; }

rcdc_status rcdc_index_write(rcdc_ctx *ctx, const void *d_ids, uint64_t id_stride,
                             const void *d_offset, uint64_t offset_stride, const void *d_len,
                             uint64_t len_stride, const void *d_ulen, uint64_t ulen_stride,
                             uint64_t n_entries, const rcdc_ixwrite_pack *packs, uint64_t n_packs,
                             const rcdc_ixwrite_file *files, uint32_t n_files,
                             const uint8_t *supersedes, uint64_t n_supersedes, const char *times,
                             uint64_t time_bytes, void *d_out, uint64_t cap_out,
                             rcdc_ixwrite_out *out, uint64_t *total, void *hip_stream) {
    if (!ctx) return invalid("rcdc_index_write: ctx is NULL");
    if (!total) return invalid("rcdc_index_write: total is NULL");
    if ((n_files && (!files || !out)) || (n_packs && !packs) || (n_supersedes && !supersedes) ||
        (time_bytes && !times) || (n_entries && (!d_ids || !d_offset || !d_len || !d_ulen)) ||
        (cap_out && !d_out))
        return invalid("rcdc_index_write: null array");
    if ((((uintptr_t)d_offset | (uintptr_t)d_len | (uintptr_t)d_ulen) & 3u) ||
        ((offset_stride | len_stride | ulen_stride) & 3u))
        return invalid("rcdc_index_write: the integer arrays and their strides must be 4-byte aligned");
    if ((uintptr_t)d_out & 15u) return invalid("rcdc_index_write: d_out must be 16-byte aligned");

    // the written packs in output order, each file's root text, the counts
    std::vector<IxwPack> wp;
    std::vector<uint32_t> wfirst;
    std::vector<IxwFile> wf(n_files);
    uint64_t written = 0, sups = 0, tbytes = 0;
    for (uint32_t f = 0; f < n_files; f++) {
        const rcdc_ixwrite_file &fl = files[f];
        if (fl.pack_first > n_packs || fl.pack_count > n_packs - fl.pack_first)
            return invalid("rcdc_index_write: a file's packs lie outside the pack records");
        if (fl.n_delete > fl.pack_count)
            return invalid("rcdc_index_write: n_delete above pack_count");
        if (fl.has_supersedes > 1u) return invalid("rcdc_index_write: has_supersedes above 1");
        const uint64_t ns = fl.has_supersedes ? fl.sup_count : 0;
        if (ns && (fl.sup_first > n_supersedes || ns > n_supersedes - fl.sup_first))
            return invalid("rcdc_index_write: a file's supersedes lie outside the ids");
        if (ns > kMaxSup || fl.sup_first + ns >= kMaxCount)
            return invalid("rcdc_index_write: too many supersedes ids");
        if (wp.size() + fl.pack_count >= kMaxCount)
            return invalid("rcdc_index_write: the batch writes 2^32 - 1 pack records or more");
        IxwFile &w = wf[f];
        w.pack_a = (uint32_t)wp.size();
        w.n_delete = fl.n_delete;
        w.has_sup = fl.has_supersedes;
        w.sup_first = (uint32_t)fl.sup_first;
        w.sup_count = (uint32_t)ns;
        w.head_len = 1u + (fl.has_supersedes ? 14u + (ns ? (uint32_t)ns * kIxwSupId - 1u : 0u) + 2u : 0u) + 9u;
        w.mid_len = fl.n_delete ? kIxwMid : 0u;
        sups += ns;
        for (uint32_t k = 0; k < fl.pack_count; k++) {
            const rcdc_ixwrite_pack &pk = packs[fl.pack_first + k];
            if (pk.type > 1u) return invalid("rcdc_index_write: a pack's type is above 1");
            if (pk.flags & ~(RCDC_IXWRITE_HAS_TIME | RCDC_IXWRITE_HAS_SIZE))
                return invalid("rcdc_index_write: unknown pack flags");
            if (pk.first > n_entries || pk.count > n_entries - pk.first)
                return invalid("rcdc_index_write: a pack's entries lie outside the arrays");
            IxwPack d = {};
            memcpy(d.id, pk.id, 32);
            d.first = pk.first;
            d.count = pk.count;
            d.size = pk.size;
            d.file = f;
            const bool del = k >= fl.pack_count - fl.n_delete;
            const bool lead = del ? k > fl.pack_count - fl.n_delete : k > 0;
            d.flags = pk.flags | (pk.type ? kIxwTree : 0u) | (lead ? kIxwComma : 0u) |
                      (del ? kIxwDelete : 0u);
            if (pk.flags & RCDC_IXWRITE_HAS_TIME) {
                if (pk.time_len > RCDC_IXWRITE_MAX_TIME)
                    return invalid("rcdc_index_write: a time is longer than RCDC_IXWRITE_MAX_TIME");
                if (pk.time_off > time_bytes || pk.time_len > time_bytes - pk.time_off)
                    return invalid("rcdc_index_write: a time lies outside the text arena");
                for (uint32_t i = 0; i < pk.time_len; i++) {
                    const unsigned char c = (unsigned char)times[pk.time_off + i];
                    if (c < 0x20 || c > 0x7E || c == '"' || c == '\\')
                        return invalid("rcdc_index_write: a time holds a byte outside 0x20..0x7E, "
                                       "a quote or a backslash");
                }
                d.time_off = pk.time_off;
                d.time_len = pk.time_len;
                tbytes += pk.time_len;
            }
            wfirst.push_back((uint32_t)written);
            written += pk.count;
            if (written >= kMaxCount)
                return invalid("rcdc_index_write: the batch writes 2^32 - 1 entries or more");
            wp.push_back(d);
        }
        w.pack_b = (uint32_t)wp.size();
    }
    wfirst.push_back((uint32_t)written);
    const uint64_t bound = rcdc_index_write_bound(written, wp.size(), n_files, sups, tbytes);
    if (cap_out < bound) return invalid("rcdc_index_write: cap_out below rcdc_index_write_bound");
    *total = 0;
    if (n_files == 0) return RCDC_OK;

    DeviceGuard g(ctx_device(ctx));
    hipStream_t st = (hipStream_t)hip_stream;
    CarvedScratch sc;
    IxwArgs a = {};
    a.ids = static_cast<const uint8_t *>(d_ids);
    a.off = static_cast<const uint8_t *>(d_offset);
    a.len = static_cast<const uint8_t *>(d_len);
    a.ulen = static_cast<const uint8_t *>(d_ulen);
    a.id_stride = id_stride;
    a.off_stride = offset_stride;
    a.len_stride = len_stride;
    a.ulen_stride = ulen_stride;
    a.n_packs = (uint32_t)wp.size();
    a.n_files = n_files;
    a.n_written = (uint32_t)written;
    a.n_spans = (uint32_t)((bound + kIxwSpan - 1) / kIxwSpan);
    a.out = static_cast<uint8_t *>(d_out);
    IxwPack *d_packs = nullptr;
    uint32_t *d_wfirst = nullptr;
    IxwFile *d_files = nullptr;
    uint8_t *d_sup = nullptr, *d_times = nullptr, *d_tmp = nullptr;
    HIP_TRY(ix_write_scan_bytes(std::max<uint64_t>(written, wp.size()) + 1, &a.scan_tmp_bytes));
    sc.want(&d_packs, wp.size());
    sc.want(&d_wfirst, wfirst.size());
    sc.want(&d_files, n_files);
    sc.want(&d_sup, n_supersedes * 32);
    sc.want(&d_times, time_bytes);
    sc.want(&d_tmp, a.scan_tmp_bytes);
    sc.want(&a.sizes, written + 1);
    sc.want(&a.epos, written + 1);
    sc.want(&a.psize, wp.size() + 1);
    sc.want(&a.ppos, wp.size() + 1);
    sc.want(&a.pabs, wp.size());
    sc.want(&a.ebase, wp.size());
    sc.want(&a.fout, n_files);
    sc.want(&a.total, 1);
    HIP_TRY(sc.alloc());
    const auto up = [st](void *dst, const void *src, uint64_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    HIP_TRY(up(d_packs, wp.data(), wp.size() * sizeof(IxwPack)));
    HIP_TRY(up(d_wfirst, wfirst.data(), wfirst.size() * sizeof(uint32_t)));
    HIP_TRY(up(d_files, wf.data(), wf.size() * sizeof(IxwFile)));
    HIP_TRY(up(d_sup, supersedes, n_supersedes * 32));
    HIP_TRY(up(d_times, times, time_bytes));
    a.packs = d_packs;
    a.wfirst = d_wfirst;
    a.files = d_files;
    a.sup = d_sup;
    a.times = d_times;
    a.scan_tmp = d_tmp;
    HIP_TRY(launch_ix_write(a, st));
    HIP_TRY(hipMemcpyAsync(out, a.fout, n_files * sizeof *out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(total, a.total, sizeof *total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (*total > bound)
        return set_error(RCDC_ERR_INTERNAL, "rcdc_index_write: more text than the bound allows");
    return RCDC_OK;
}

}  // extern "C"
