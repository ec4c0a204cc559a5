// rcdc_ingest_steps.h -- the ingest engine's steps that touch neither HIP nor
// a lock (rcdc_ingest.cpp stage A step 4, stage B steps 4-6): standard C++
// over the ABI's plain structs, so tools/ingest_steps_check.cpp can run them
// on a CPU (tests/test_ingest_steps_host.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/rcdc.h"

namespace rcdc {
namespace steps {

constexpr uint64_t kMaxPackSize = 4076ull << 20;  // packer.rs:58
constexpr uint32_t kMaxPackCount = 10000;         // packer.rs:60

// PackSizer (packer.rs:65-200): only pack_size() steers should_save.
struct PackSizer {
    uint64_t default_size, grow, limit, current;
    uint64_t pack_size() const {
        uint64_t size = default_size;
        if (grow) size = ((uint64_t)std::sqrt((double)current) * grow + default_size) & 0xFFFFFFFFull;
        return std::min(std::min(size, limit), kMaxPackSize);
    }
};

// A header entry's bytes (HeaderEntry::length, packfile.rs:158-163).
inline uint64_t header_entry_len(const rcdc_pack_blob &b) { return b.uncompressed_len ? 41 : 37; }

// Pack grouping.  should_save (packer.rs:659-671) pack by pack: a pack takes
// blobs (their sealed lengths, `len`) until its size reaches the sizer's
// pack_size() or it holds MAX_COUNT blobs; take_data adds each closed pack's
// size -- blobs, header entries, 32 B of header sealing and the u32 -- to the
// sizer (:749-758).  The last pack, if not closed by either rule, stays open
// (its blobs start at `open_from`; the sizer does not see it) unless
// `finalize` (Packer::finalize) closes it too.  `aged` (MAX_AGE,
// packer.rs:63,668-670) closes the first pack whatever its size and changes
// nothing else.  Returns (blob0, nblobs) per closed pack.
inline std::vector<std::pair<uint32_t, uint32_t>> group_packs(const rcdc_pack_blob *blobs,
                                                              size_t n, PackSizer &sizer,
                                                              bool finalize, bool aged,
                                                              size_t *open_from) {
    std::vector<std::pair<uint32_t, uint32_t>> grp;
    size_t b0 = 0;
    while (b0 < n) {
        const uint64_t limit = sizer.pack_size();
        uint64_t sz = 0, hdr = 0;
        size_t e = b0;
        while (e < n && sz < limit && e - b0 < kMaxPackCount) {
            sz += blobs[e].len;
            hdr += header_entry_len(blobs[e]);
            e++;
        }
        const bool closed = sz >= limit || e - b0 >= kMaxPackCount;
        if (!closed && !finalize && !(aged && b0 == 0)) break;
        grp.push_back({(uint32_t)b0, (uint32_t)(e - b0)});
        sizer.current += sz + hdr + 32 + 4;
        b0 = e;
    }
    *open_from = b0;
    return grp;
}

// Pack layout: the packs back to back in one output buffer.  A pack file is
// its blobs, one header entry per blob, 32 B of header sealing and the u32
// header length; packs[j] gets out_off, blob0 and nblobs (the nonces, size
// and header_len are not touched).  Returns the total.
inline uint64_t layout_packs(const rcdc_pack_blob *blobs,
                             const std::vector<std::pair<uint32_t, uint32_t>> &grp,
                             rcdc_pack *packs) {
    uint64_t total = 0;
    for (size_t j = 0; j < grp.size(); j++) {
        uint64_t sz = 32 + 4;
        for (uint32_t i = grp[j].first; i < grp[j].first + grp[j].second; i++)
            sz += blobs[i].len + header_entry_len(blobs[i]);
        packs[j].out_off = total;
        packs[j].blob0 = grp[j].first;
        packs[j].nblobs = grp[j].second;
        total += sz;
    }
    return total;
}

// D2H grouping: the packs [first, last) of one copy, bytes [lo, hi) of the
// pack buffer.  A group takes whole packs until it spans group_bytes (at
// least one pack; group_bytes 1: a pack each); the last group ends at total.
struct D2HRange {
    size_t first, last;
    uint64_t lo, hi;
};
inline std::vector<D2HRange> d2h_ranges(const rcdc_pack *packs, size_t n, uint64_t total,
                                        uint64_t group_bytes) {
    std::vector<D2HRange> out;
    for (size_t a = 0; a < n;) {
        size_t b = a + 1;
        while (b < n && packs[b].out_off - packs[a].out_off < group_bytes) b++;
        out.push_back({a, b, packs[a].out_off, b < n ? packs[b].out_off : total});
        a = b;
    }
    return out;
}

// Cut lists.  One plan stream of a batch as the chunker saw it: `off`, `len`
// in the arena; `stream`: part of a stream (else a whole file), with its
// device carry slot; `final`: the stream ends in this batch; `aborted`.
struct UnitView {
    bool stream, final, aborted;
    uint64_t off, len;
    int cslot;
};
// A unit's cuts (relative to the unit, `counts[i]` of them, consecutive in
// `cuts`) become chunks: (c_off, c_len) in the arena.  A stream's last chunk
// of a batch that is not its end is its carry, not a chunk yet -- every
// earlier cut is final -- and so is an aborted stream's (which carries
// nothing on).  A carry starts at `from` in its unit (0: the whole unit, also
// one with zero chunks); its bytes, if any, go to the stream's slot of
// max_chunk bytes in the carry pool (`copies`, src 0 = the arena).
struct CutLists {
    std::vector<uint64_t> cuts;     // per unit, consecutive (relative to the unit)
    std::vector<uint32_t> ncuts;    // per unit: chunks final in this batch
    std::vector<uint64_t> c_off, c_len;
    std::vector<std::pair<uint32_t, uint64_t>> carries;  // (unit, carry start in the unit)
    std::vector<rcdc_copy_ref> copies;
};
inline CutLists cut_lists(const std::vector<UnitView> &units, const uint64_t *counts,
                          const uint64_t *cuts, uint64_t max_chunk) {
    CutLists L;
    L.ncuts.resize(units.size());
    uint64_t k = 0;
    for (size_t i = 0; i < units.size(); i++) {
        const UnitView &u = units[i];
        const uint64_t n = counts[i];
        uint64_t keep = n;
        if (u.stream && (!u.final || u.aborted)) {
            keep = n ? n - 1 : 0;
            const uint64_t from = keep ? cuts[k + keep - 1] : 0;
            if (!u.aborted) {
                L.carries.push_back({(uint32_t)i, from});
                if (u.len > from) {
                    rcdc_copy_ref c{};
                    c.in_off = u.off + from;
                    c.out_off = (uint64_t)u.cslot * max_chunk;
                    c.len = u.len - from;
                    c.src = 0;
                    L.copies.push_back(c);
                }
            }
        }
        L.ncuts[i] = (uint32_t)keep;
        uint64_t prev = 0;
        for (uint64_t j = 0; j < keep; j++) {
            L.cuts.push_back(cuts[k + j]);
            L.c_off.push_back(u.off + prev);
            L.c_len.push_back(cuts[k + j] - prev);
            prev = cuts[k + j];
        }
        k += n;
    }
    return L;
}

}  // namespace steps
}  // namespace rcdc
