// family_plans_check -- the family units' planners
// (rustic_core_amd/csrc/rcdc_family_plans.h) on a CPU: reads cases on stdin,
// prints one result line per case (tests/test_family_plans_host.py).  Links
// nothing of HIP and nothing of librcdc.so.  A refused case prints
// "<case> ERR <status> <the error text>".
//
// Cases, as whitespace-separated tokens:
//   keymat (BYTE)*64
//     -> keymat (RK256)*60 (RK128)*44 (RPOW)*325 (R2J)*160 (TE)*256
//   pmul   (A)*5 (B)*5   pnorm (A)*5   pfull (A)*5   pblock (W)*4 K   ptag (H)*5 SLO SHI
//     the limb arithmetic of rcdc_p1305.h (tests/test_p1305_host.py)
//     -> the 5 limbs of the result; ptag: the 16 tag bytes
//   pack   RAW N_SRC OUT_LEN NBLOBS (TYPE LEN ULEN IN_OFF PAD)* NPACKS (BLOB0 NBLOBS OUT_OFF)*
//     blob i: id byte j = (31 i + j) & 255, nonce byte j = (i + 3 j) & 255; pack p: header
//     nonce byte j = (5 p + j + 1) & 255; d_in = 0x10000, source j = 0x1000000 (j + 1)
//     -> pack 0 NHDR (BYTE)* NBLOBS (BLOB_OFFSET)* NPACKS (HEADER_LEN SIZE)*
//             then the data batch and the header batch, each as
//             IN NB (IN_OFF LEN OUT_OFF N0 N1 N2 N3 FLAGS)* NU (BLOB B0 B1)* N0 (UNIT0)*
//             then NCOPYWORDS (WORD)*
//   zwin   WBLOCKS N (LEN)*          blob i: in_off = 1000 i, out_off = 7 i
//     -> zwin MAXW NWIN (BLOB0 NBLOB BLK0 NBLK)* NBLOB (IN_OFF OUT_OFF LEN BLK0 NBLK)*
//             NBLK (BLOB START LEN FLAGS)*
//   zdx    WS_MAX N (NEED NBLK STATUS FLAGS NCOMP NTREELESS FRAME_LEN)*
//     -> zdx PEAK NGROUPS (A B NBLK DATA TOTAL)* N (BLK0 DATA0)*
//            per group: NLIST (J)* M (J)*      then STAT1 STAT2 STAT3
//   place  ZERO_TEST R N_INS (BASE LEN)* N_OUTS (BASE LEN)* NBLOBS (IN_OFF LEN SRC DEST0 NDESTS)*
//          NDESTS (OUT_OFF DST)* DUMP
//     -> place 0 ROUNDS NWIN (ROUND WIN NTILES)* and, with DUMP,
//              NTILES (SRC LEN BLOB DEST0 NDESTS OFF ALIGNED)*
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../rustic_core_amd/csrc/rcdc_family_plans.h"

using namespace rcdc;
using namespace rcdc::plans;
typedef unsigned long long ull;

namespace {

template <typename T>
T rd() {
    ull v = 0;
    if (!(std::cin >> v)) {
        fprintf(stderr, "family_plans_check: case cut short\n");
        exit(2);
    }
    return (T)v;
}

void do_keymat() {
    uint8_t key[64];
    for (uint8_t &b : key) b = rd<uint8_t>();
    AeadKeyDev K;
    aead_key_material(key, &K);
    printf("keymat");
    for (uint32_t v : K.rk256) printf(" %u", v);
    for (uint32_t v : K.rk128) printf(" %u", v);
    for (auto &r : K.rpow)
        for (uint32_t v : r) printf(" %u", v);
    for (auto &r : K.r2j)
        for (uint32_t v : r) printf(" %u", v);
    for (uint32_t v : K.te) printf(" %u", v);
    printf("\n");
}

// The limb arithmetic of rcdc_p1305.h, one call per case.
p1305::P26 rd_limbs() {
    p1305::P26 a;
    for (uint32_t &v : a.h) v = rd<uint32_t>();
    return a;
}

void print_limbs(const char *what, const p1305::P26 &a) {
    printf("%s %u %u %u %u %u\n", what, a.h[0], a.h[1], a.h[2], a.h[3], a.h[4]);
}

void do_pmul() {
    const p1305::P26 a = rd_limbs(), b = rd_limbs();
    print_limbs("pmul", p1305::pmul(a, b.h));
}

void do_pnorm() {
    p1305::P26 a = rd_limbs();
    p1305::pnorm(a);
    print_limbs("pnorm", a);
}

void do_pfull() {
    p1305::P26 a = rd_limbs();
    p1305::pfull(a);
    print_limbs("pfull", a);
}

void do_pblock() {
    uint32_t w[4];
    for (uint32_t &v : w) v = rd<uint32_t>();
    const uint32_t k = rd<uint32_t>();
    print_limbs("pblock", p1305::pblock(w, k));
}

void do_ptag() {
    const p1305::P26 h = rd_limbs();
    const uint64_t slo = rd<uint64_t>(), shi = rd<uint64_t>();
    uint8_t tag[16];
    p1305::ptag(h, slo, shi, tag);
    printf("ptag");
    for (uint8_t b : tag) printf(" %u", b);
    printf("\n");
}

void print_batch(const AeadBatch &B) {
    printf(" %llu %zu", (ull)(uintptr_t)B.in, B.blobs.size());
    for (const AeadBlob &b : B.blobs)
        printf(" %llu %llu %llu %u %u %u %u %u", (ull)b.in_off, (ull)b.len, (ull)b.out_off,
               b.nonce[0], b.nonce[1], b.nonce[2], b.nonce[3], b.flags);
    printf(" %zu", B.units.size());
    for (const AeadUnit &u : B.units) printf(" %u %u %u", u.blob, u.b0, u.b1);
    printf(" %zu", B.unit0.size());
    for (uint32_t v : B.unit0) printf(" %u", v);
}

void do_pack() {
    const bool raw = rd<int>() != 0;
    const uint32_t n_src = rd<uint32_t>();
    const uint64_t out_len = rd<uint64_t>();
    std::vector<rcdc_pack_blob> blobs(rd<size_t>());
    for (size_t i = 0; i < blobs.size(); i++) {
        rcdc_pack_blob &b = blobs[i];
        b = rcdc_pack_blob{};
        b.type = rd<uint32_t>();
        b.len = rd<uint32_t>();
        b.uncompressed_len = rd<uint32_t>();
        b.in_off = rd<uint64_t>();
        b.pad = rd<uint32_t>();
        for (int j = 0; j < 32; j++) b.id[j] = (uint8_t)(31 * i + j);
        for (int j = 0; j < 16; j++) b.nonce[j] = (uint8_t)(i + 3 * j);
    }
    std::vector<rcdc_pack> packs(rd<size_t>());
    for (size_t p = 0; p < packs.size(); p++) {
        packs[p] = rcdc_pack{};
        packs[p].blob0 = rd<uint32_t>();
        packs[p].nblobs = rd<uint32_t>();
        packs[p].out_off = rd<uint64_t>();
        for (int j = 0; j < 16; j++) packs[p].header_nonce[j] = (uint8_t)(5 * p + j + 1);
    }
    std::vector<const void *> srcs(n_src);
    for (uint32_t j = 0; j < n_src; j++) srcs[j] = (const void *)(uintptr_t)(0x1000000ull * (j + 1));
    std::vector<uint32_t> offs(blobs.size() + 1, 0xFFFFFFFFu);
    blobs.push_back(rcdc_pack_blob{});  // (data() of an empty vector may be null)
    packs.push_back(rcdc_pack{});
    PackPlan pp;
    char msg[kMsg];
    const rcdc_status st =
        pack_plan(true, n_src ? nullptr : (const void *)(uintptr_t)0x10000, blobs.data(),
                  (uint32_t)blobs.size() - 1, packs.data(), (uint32_t)packs.size() - 1,
                  (const void *)(uintptr_t)0x20, out_len, offs.data(), raw, srcs.data(), n_src, pp, msg);
    if (st) {
        printf("pack ERR %d %s\n", (int)st, msg);
        return;
    }
    printf("pack 0 %zu", pp.hdr.size());
    for (uint8_t b : pp.hdr) printf(" %u", b);
    printf(" %zu", blobs.size() - 1);
    for (size_t i = 0; i + 1 < blobs.size(); i++) printf(" %u", offs[i]);
    printf(" %zu", packs.size() - 1);
    for (size_t p = 0; p + 1 < packs.size(); p++) printf(" %u %llu", packs[p].header_len, (ull)packs[p].size);
    print_batch(pp.data);
    print_batch(pp.headers);
    printf(" %zu", pp.copies.size());
    for (uint64_t v : pp.copies) printf(" %llu", (ull)v);
    printf("\n");
}

void do_zwin() {
    const uint64_t wblocks = rd<uint64_t>();
    std::vector<rcdc_zstd_ref> refs(rd<size_t>());
    for (size_t i = 0; i < refs.size(); i++) refs[i] = {1000 * i, rd<uint64_t>(), 7 * i};
    const ZstdWindows W = zstd_windows(refs.data(), (uint32_t)refs.size(), wblocks);
    printf("zwin %llu %zu", (ull)W.maxw, W.wins.size());
    for (const ZstdWin &w : W.wins)
        printf(" %llu %llu %llu %llu", (ull)w.blob0, (ull)w.nblob, (ull)w.blk0, (ull)w.nblk);
    printf(" %zu", W.blobs.size());
    for (const ZstdBlob &b : W.blobs)
        printf(" %llu %llu %u %u %u", (ull)b.in_off, (ull)b.out_off, b.len, b.blk0, b.nblk);
    printf(" %zu", W.blks.size());
    for (const ZstdBlk &b : W.blks) printf(" %u %u %u %u", b.blob, b.start, b.len, b.flags);
    printf("\n");
}

void do_zdx() {
    const uint64_t ws_max = rd<uint64_t>();
    const uint32_t n = rd<uint32_t>();
    std::vector<ZdxFrame> hf(n + 1);
    std::vector<rcdc_zstd_dec_ref> refs(n + 1);
    for (uint32_t i = 0; i < n; i++) {
        hf[i] = ZdxFrame{};
        hf[i].need = rd<uint64_t>();
        hf[i].nblk = rd<uint32_t>();
        hf[i].status = rd<uint32_t>();
        hf[i].flags = rd<uint32_t>();
        hf[i].ncomp = rd<uint32_t>();
        hf[i].ntreeless = rd<uint32_t>();
        refs[i] = rcdc_zstd_dec_ref{};
        refs[i].frame_len = rd<uint64_t>();
    }
    const ZdxGroups R = zdx_groups(hf.data(), n, ws_max);
    printf("zdx %llu %zu", (ull)R.peak, R.groups.size());
    for (const ZdxGroup &G : R.groups)
        printf(" %u %u %llu %llu %llu", G.a, G.b, (ull)G.nblk, (ull)G.data,
               (ull)zdx_layout(G.nblk, G.data).total);
    printf(" %zu", R.place.size());
    for (const ZdxPlace &p : R.place) printf(" %llu %llu", (ull)p.blk0, (ull)p.data0);
    uint64_t stats[8] = {0};
    std::vector<uint32_t> list, order;
    for (const ZdxGroup &G : R.groups) {
        zdx_group_lists(hf.data(), refs.data(), G, list, order, stats);
        printf(" %zu", list.size());
        for (uint32_t j : list) printf(" %u", j);
        printf(" %zu", order.size());
        for (uint32_t j : order) printf(" %u", j);
    }
    printf(" %llu %llu %llu\n", (ull)stats[1], (ull)stats[2], (ull)stats[3]);
}

void do_place() {
    const bool zero_test = rd<int>() != 0;
    const uint64_t R = rd<uint64_t>();
    std::vector<const void *> d_ins(rd<size_t>());
    std::vector<uint64_t> in_lens(d_ins.size());
    for (size_t j = 0; j < d_ins.size(); j++) {
        d_ins[j] = (const void *)(uintptr_t)rd<uint64_t>();
        in_lens[j] = rd<uint64_t>();
    }
    std::vector<void *> d_outs(rd<size_t>());
    std::vector<uint64_t> out_lens(d_outs.size());
    for (size_t j = 0; j < d_outs.size(); j++) {
        d_outs[j] = (void *)(uintptr_t)rd<uint64_t>();
        out_lens[j] = rd<uint64_t>();
    }
    std::vector<rcdc_place_blob> blobs(rd<size_t>());
    for (rcdc_place_blob &b : blobs) {
        b = rcdc_place_blob{};
        b.in_off = rd<uint64_t>();
        b.len = rd<uint64_t>();
        b.src = rd<uint32_t>();
        b.dest0 = rd<uint32_t>();
        b.ndests = rd<uint32_t>();
    }
    std::vector<rcdc_place_dest> dests(rd<size_t>());
    for (rcdc_place_dest &d : dests) {
        d = rcdc_place_dest{};
        d.out_off = rd<uint64_t>();
        d.dst = rd<uint32_t>();
    }
    const bool dump = rd<int>() != 0;
    const uint32_t nblobs = (uint32_t)blobs.size(), ndests = (uint32_t)dests.size();
    std::vector<uint64_t> daddr(ndests + 1);
    blobs.push_back(rcdc_place_blob{});  // (data() of an empty vector may be null)
    dests.push_back(rcdc_place_dest{});
    d_ins.push_back(nullptr);
    in_lens.push_back(0);
    d_outs.push_back(nullptr);
    out_lens.push_back(0);
    char msg[kMsg];
    const rcdc_status st = place_validate(d_ins.data(), in_lens.data(), (uint32_t)d_ins.size() - 1,
                                          blobs.data(), nblobs, dests.data(), ndests, d_outs.data(),
                                          out_lens.data(), (uint32_t)d_outs.size() - 1, daddr.data(), msg);
    if (st) {
        printf("place ERR %d %s\n", (int)st, msg);
        return;
    }
    // the pass of rcdc_place.cpp, with a list in place of uploads and launches
    std::vector<PlaceTile> tiles(R), all;
    std::vector<uint64_t> wins;
    PlaceWindow W;
    PlaceCursor cur;
    auto flush = [&] {
        if (W.pos == W.w0) return;
        wins.insert(wins.end(), {W.rounds, (uint64_t)W.win, W.pos - W.w0});
        all.insert(all.end(), tiles.begin() + W.w0, tiles.begin() + W.pos);
        W.sent();
    };
    for (;;) {
        cur = place_fill(d_ins.data(), blobs.data(), nblobs, daddr.data(), zero_test, tiles.data(), &W.pos,
                         W.limit(R), cur);
        if (cur.blob == nblobs) break;
        flush();
        if (W.pos == R) W.new_round();
    }
    flush();
    printf("place 0 %llu %zu", (ull)W.rounds, wins.size() / 3);
    for (uint64_t v : wins) printf(" %llu", (ull)v);
    if (dump) {
        printf(" %zu", all.size());
        for (const PlaceTile &t : all)
            printf(" %llu %u %u %u %u %llu %d", (ull)t.src, t.len, t.blob, t.dest0, t.ndests,
                   (ull)(t.off & ~kPlaceAligned), (t.off & kPlaceAligned) ? 1 : 0);
    }
    printf("\n");
}

}  // namespace

int main() {
    std::ios::sync_with_stdio(false);
    std::string what;
    while (std::cin >> what) {
        if (what == "keymat") do_keymat();
        else if (what == "pack") do_pack();
        else if (what == "zwin") do_zwin();
        else if (what == "zdx") do_zdx();
        else if (what == "place") do_place();
        else if (what == "pmul") do_pmul();
        else if (what == "pnorm") do_pnorm();
        else if (what == "pfull") do_pfull();
        else if (what == "pblock") do_pblock();
        else if (what == "ptag") do_ptag();
        else {
            fprintf(stderr, "family_plans_check: unknown case '%s'\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
