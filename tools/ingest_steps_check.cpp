// ingest_steps_check -- the ingest engine's pure steps
// (rustic_core_amd/csrc/rcdc_ingest_steps.h) on a CPU: reads cases on stdin,
// prints one result line per case (tests/test_ingest_steps_host.py).  Links
// nothing of HIP and nothing of librcdc.so.
//
// Cases, as whitespace-separated tokens:
//   group  DEFAULT GROW LIMIT CURRENT FINALIZE AGED N (LEN ULEN)*N
//     -> group  NPACKS (BLOB0 NBLOBS)* OPEN_FROM CURRENT
//   layout N (LEN ULEN)*N G (BLOB0 NBLOBS)*G
//     -> layout TOTAL (OUT_OFF SIZE)*G
//   d2h    GROUP_BYTES TOTAL N (OUT_OFF)*N
//     -> d2h    NGROUPS (FIRST LAST LO HI)*
//   cuts   MAX_CHUNK NUNITS (STREAM FINAL ABORTED OFF LEN CSLOT COUNT (CUT)*COUNT)*NUNITS
//     -> cuts   NUNITS (NCUTS)* NCHUNKS (CUT C_OFF C_LEN)* NCARRIES (UNIT FROM)*
//               NCOPIES (IN_OFF OUT_OFF LEN)*
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../rustic_core_amd/csrc/rcdc_ingest_steps.h"

using namespace rcdc::steps;

namespace {

template <typename T>
T rd() {
    unsigned long long v = 0;
    if (!(std::cin >> v)) {
        fprintf(stderr, "ingest_steps_check: case cut short\n");
        exit(2);
    }
    return (T)v;
}

std::vector<rcdc_pack_blob> rd_blobs() {
    std::vector<rcdc_pack_blob> b(rd<size_t>());
    for (auto &x : b) {
        x = rcdc_pack_blob{};
        x.len = rd<uint32_t>();
        x.uncompressed_len = rd<uint32_t>();
    }
    return b;
}

void do_group() {
    PackSizer s{};
    s.default_size = rd<uint64_t>();
    s.grow = rd<uint64_t>();
    s.limit = rd<uint64_t>();
    s.current = rd<uint64_t>();
    const bool finalize = rd<int>() != 0, aged = rd<int>() != 0;
    const auto blobs = rd_blobs();
    size_t open_from = 0;
    const auto grp = group_packs(blobs.data(), blobs.size(), s, finalize, aged, &open_from);
    printf("group %zu", grp.size());
    for (auto &g : grp) printf(" %u %u", g.first, g.second);
    printf(" %zu %llu\n", open_from, (unsigned long long)s.current);
}

void do_layout() {
    const auto blobs = rd_blobs();
    std::vector<std::pair<uint32_t, uint32_t>> grp(rd<size_t>());
    for (auto &g : grp) {
        g.first = rd<uint32_t>();
        g.second = rd<uint32_t>();
    }
    std::vector<rcdc_pack> packs(grp.size());
    const uint64_t total = layout_packs(blobs.data(), grp, packs.data());
    printf("layout %llu", (unsigned long long)total);
    for (size_t j = 0; j < packs.size(); j++) {
        const uint64_t end = j + 1 < packs.size() ? packs[j + 1].out_off : total;
        printf(" %llu %llu", (unsigned long long)packs[j].out_off,
               (unsigned long long)(end - packs[j].out_off));
    }
    printf("\n");
}

void do_d2h() {
    const uint64_t group_bytes = rd<uint64_t>(), total = rd<uint64_t>();
    std::vector<rcdc_pack> packs(rd<size_t>());
    for (auto &p : packs) {
        p = rcdc_pack{};
        p.out_off = rd<uint64_t>();
    }
    const auto r = d2h_ranges(packs.data(), packs.size(), total, group_bytes);
    printf("d2h %zu", r.size());
    for (auto &x : r)
        printf(" %zu %zu %llu %llu", x.first, x.last, (unsigned long long)x.lo,
               (unsigned long long)x.hi);
    printf("\n");
}

void do_cuts() {
    const uint64_t max_chunk = rd<uint64_t>();
    std::vector<UnitView> units(rd<size_t>());
    std::vector<uint64_t> counts, cuts;
    for (auto &u : units) {
        u.stream = rd<int>() != 0;
        u.final = rd<int>() != 0;
        u.aborted = rd<int>() != 0;
        u.off = rd<uint64_t>();
        u.len = rd<uint64_t>();
        u.cslot = rd<int>();
        counts.push_back(rd<uint64_t>());
        for (uint64_t j = 0; j < counts.back(); j++) cuts.push_back(rd<uint64_t>());
    }
    counts.push_back(0);  // (data() of an empty vector may be null)
    cuts.push_back(0);
    const CutLists L = cut_lists(units, counts.data(), cuts.data(), max_chunk);
    printf("cuts %zu", L.ncuts.size());
    for (uint32_t n : L.ncuts) printf(" %u", n);
    printf(" %zu", L.cuts.size());
    for (size_t k = 0; k < L.cuts.size(); k++)
        printf(" %llu %llu %llu", (unsigned long long)L.cuts[k], (unsigned long long)L.c_off[k],
               (unsigned long long)L.c_len[k]);
    printf(" %zu", L.carries.size());
    for (auto &c : L.carries) printf(" %u %llu", c.first, (unsigned long long)c.second);
    printf(" %zu", L.copies.size());
    for (auto &c : L.copies)
        printf(" %llu %llu %llu", (unsigned long long)c.in_off, (unsigned long long)c.out_off,
               (unsigned long long)c.len);
    printf("\n");
}

}  // namespace

int main() {
    std::ios::sync_with_stdio(false);
    std::string what;
    while (std::cin >> what) {
        if (what == "group") do_group();
        else if (what == "layout") do_layout();
        else if (what == "d2h") do_d2h();
        else if (what == "cuts") do_cuts();
        else {
            fprintf(stderr, "ingest_steps_check: unknown case '%s'\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
