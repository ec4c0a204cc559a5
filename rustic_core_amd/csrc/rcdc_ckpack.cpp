// rcdc_check_packs (include/rcdc.h): the host half -- argument checks, the
// device copies of the ranges and header records, scratch memory (the
// context's CkpackState) and the launch.  The kernels are in rcdc_ckpack.hip.
//
// Nothing is sized from a device count, so the call stops the stream once, at
// the end, to hand the per-pack records and the totals to the caller.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "rcdc_ckpack.h"
#include "rcdc_ctx.h"

using namespace rcdc;

extern "C" {

uint32_t rcdc_check_packs_sort_max(void) { return RCDC_CKPACK_SORT_MAX; }

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
                             rcdc_ckpack_result *result, void *hip_stream) {
    if (!valid_ctx(ctx)) return invalid("rcdc_check_packs: ctx is NULL");
    if (!result) return invalid("rcdc_check_packs: result is NULL");
    if (n && (!d_ids || !d_off || !d_len || !d_ulen))
        return invalid("rcdc_check_packs: null array");
    if (n_packs && (!ranges || !packs)) return invalid("rcdc_check_packs: null array");
    if (cap_findings && !d_findings) return invalid("rcdc_check_packs: d_findings is NULL");
    if (n >= 0xFFFFFFFFull) return invalid("rcdc_check_packs: 2^32 - 1 entries or more");
    if (n_packs > 0x7FFFFFFFull) return invalid("rcdc_check_packs: more than 2^31 - 1 packs");
    if (n && (id_stride < 32 || off_stride < 4 || len_stride < 4 || ulen_stride < 4))
        return invalid("rcdc_check_packs: a stride is smaller than its element");
    if (n && (((uintptr_t)d_off | off_stride | (uintptr_t)d_len | len_stride | (uintptr_t)d_ulen |
               ulen_stride) & 3u))
        return invalid("rcdc_check_packs: offsets and lengths must be 4-byte aligned");
    // ranges: inside the entries, not overlapping
    std::vector<std::pair<uint64_t, uint64_t>> sorted;
    sorted.reserve(n_packs);
    std::vector<uint32_t> prefix(n_packs);
    uint64_t total = 0;
    for (uint64_t p = 0; p < n_packs; ++p) {
        const rcdc_prune_range &r = ranges[p];
        if (r.first > n || r.count > n - r.first)
            return invalid("rcdc_check_packs: a range past the entries");
        if (r.count) sorted.emplace_back(r.first, r.first + r.count);
        prefix[p] = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
        total += r.count;
    }
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < sorted.size(); ++i)
        if (sorted[i].first < sorted[i - 1].second)
            return invalid("rcdc_check_packs: overlapping ranges");
    // no overlap: total <= n < 2^32 - 1, so no prefix was clamped
    if (hdrs) {
        if (n_packs && (!d_hdr_ids || !d_hdr_locs || !hdr_entries))
            return invalid("rcdc_check_packs: null header arrays");
        for (uint64_t p = 0; p < n_packs; ++p) {
            const rcdc_ckpack_hdr &h = hdrs[p];
            if (h.type == RCDC_CKPACK_NO_HEADER) continue;
            if (h.type > 1) return invalid("rcdc_check_packs: a header type above 1");
            if (!h.count) continue;
            if (!d_hdr_ids[h.type] || !d_hdr_locs[h.type])
                return invalid("rcdc_check_packs: null header arrays");
            if (((uintptr_t)d_hdr_ids[h.type] | (uintptr_t)d_hdr_locs[h.type]) & 15u)
                return invalid("rcdc_check_packs: the header arrays must be 16-byte aligned");
            if (h.first > hdr_entries[h.type] || h.count > hdr_entries[h.type] - h.first)
                return invalid("rcdc_check_packs: a header range past its array");
        }
    }
    *result = rcdc_ckpack_result{};
    if (n_packs == 0) return RCDC_OK;

    CkpackState &S = ctx->ckpack;
    std::lock_guard<std::mutex> lk(S.mu);
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)hip_stream;
    rcdc_status rs;
    if ((rs = S.d_ranges.ensure(n_packs))) return rs;
    if ((rs = S.d_prefix.ensure(n_packs))) return rs;
    if ((rs = S.d_packs.ensure(n_packs))) return rs;
    if ((rs = S.d_order.ensure(std::max<uint64_t>(total, 1)))) return rs;
    if ((rs = S.d_totals.ensure(4))) return rs;
    if ((rs = S.d_list.ensure(n_packs))) return rs;
    if ((rs = S.d_list_n.ensure(2))) return rs;
    if (hdrs && (rs = S.d_hdrs.ensure(n_packs))) return rs;
    HIP_TRY(hipMemcpyAsync(S.d_ranges, ranges, n_packs * sizeof *ranges, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(S.d_prefix, prefix.data(), n_packs * 4, hipMemcpyHostToDevice, st));
    if (hdrs)
        HIP_TRY(hipMemcpyAsync(S.d_hdrs, hdrs, n_packs * sizeof *hdrs, hipMemcpyHostToDevice, st));

    CkArgs a = {};
    a.e.ids = static_cast<const uint8_t *>(d_ids);
    a.e.off = static_cast<const uint8_t *>(d_off);
    a.e.len = static_cast<const uint8_t *>(d_len);
    a.e.ulen = static_cast<const uint8_t *>(d_ulen);
    a.e.types = d_types;
    a.e.id_stride = id_stride, a.e.off_stride = off_stride;
    a.e.len_stride = len_stride, a.e.ulen_stride = ulen_stride;
    // rcdc_dindex_loc records on a 16-byte boundary: one load per entry
    a.e.loc_records = n && off_stride == 16 && len_stride == 16 && ulen_stride == 16 &&
                      a.e.len == a.e.off + 4 && a.e.ulen == a.e.off + 8 &&
                      (((uintptr_t)a.e.off - 4) & 15u) == 0;
    a.e.id_rows = n && id_stride == 32 && ((uintptr_t)d_ids & 15u) == 0;
    a.ranges = S.d_ranges;
    a.prefix = S.d_prefix;
    a.hdrs = hdrs ? S.d_hdrs.get() : nullptr;
    for (int t = 0; t < 2 && hdrs; t++) {
        a.hdr_ids[t] = static_cast<const uint8_t *>(d_hdr_ids[t]);
        a.hdr_locs[t] = d_hdr_locs[t];
    }
    a.n_packs = (uint32_t)n_packs;
    a.order_tmp = S.d_order;
    a.totals = S.d_totals;
    a.list = S.d_list;
    a.list_n = S.d_list_n;
    a.packs = S.d_packs;
    a.findings = d_findings;
    a.cap_findings = cap_findings;
    a.order = d_order;
    HIP_TRY(launch_ck_packs(a, st));
    uint64_t tot[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, S.d_totals, sizeof tot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(packs, S.d_packs, n_packs * sizeof *packs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    result->findings = tot[0];
    result->packs_host = tot[1];
    result->packs_sorted_on_device = tot[2];
    return RCDC_OK;
}

}  // extern "C"
