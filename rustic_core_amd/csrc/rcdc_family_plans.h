// rcdc_family_plans.h -- the host-only half of the family units' calls
// (rcdc_aead.cpp, rcdc_zstd_host.cpp, rcdc_place.cpp): validation and the
// descriptor lists a call uploads, as plain functions over the ABI's structs
// and the kernels' descriptors.  No HIP call and no context, so a CPU runs
// them (tools/family_plans_check.cpp, tests/test_family_plans_host.py).  A
// function that can refuse its input returns a status and writes the error
// text to `msg` (kMsg bytes); the caller hands both to the error helper.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rcdc.h"
#include "rcdc_place.h"
#include "rcdc_internal.h"
#include "rcdc_p1305.h"

namespace rcdc {
namespace plans {

constexpr size_t kMsg = 512;

inline rcdc_status refuse(char *msg, rcdc_status st, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, kMsg, fmt, ap);
    va_end(ap);
    return st;
}

// ---- blob encryption: key material -------------------------------------------

// AES S-box from its definition (multiplicative inverse in GF(2^8), then the
// affine map; FIPS-197 5.1.1), and the T-table / key schedules on the host.
inline void aes_sbox(uint8_t sb[256]) {
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ (p << 1) ^ ((p & 0x80) ? 0x1b : 0));  // p * 3
        q ^= (uint8_t)(q << 1);                                  // q / 3
        q ^= (uint8_t)(q << 2);
        q ^= (uint8_t)(q << 4);
        if (q & 0x80) q ^= 0x09;
        const uint8_t x = (uint8_t)(q ^ (uint8_t)((q << 1) | (q >> 7)) ^
                                    (uint8_t)((q << 2) | (q >> 6)) ^
                                    (uint8_t)((q << 3) | (q >> 5)) ^ (uint8_t)((q << 4) | (q >> 4)));
        sb[p] = x ^ 0x63;
    } while (p != 1);
    sb[0] = 0x63;
}

inline void aes_expand_host(const uint8_t *key, int nk, const uint8_t sb[256], uint32_t *rk) {
    const int nr = nk + 6;
    uint8_t rcon = 1;
    for (int i = 0; i < nk; i++)
        rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 |
                (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
    auto sub = [&](uint32_t t) {
        return (uint32_t)sb[t >> 24] << 24 | (uint32_t)sb[(t >> 16) & 255] << 16 |
               (uint32_t)sb[(t >> 8) & 255] << 8 | sb[t & 255];
    };
    for (int i = nk; i < 4 * (nr + 1); i++) {
        uint32_t t = rk[i - 1];
        if (i % nk == 0) {
            t = sub((t << 8) | (t >> 24)) ^ (uint32_t)rcon << 24;
            rcon = (uint8_t)((rcon << 1) ^ ((rcon & 0x80) ? 0x1b : 0));
        } else if (nk > 6 && i % nk == 4) {
            t = sub(t);
        }
        rk[i] = rk[i - nk] ^ t;
    }
}

inline void aead_key_material(const uint8_t key[64], AeadKeyDev *K) {
    uint8_t sb[256];
    aes_sbox(sb);
    for (int x = 0; x < 256; x++) {
        const uint8_t s1 = sb[x], s2 = (uint8_t)((s1 << 1) ^ ((s1 & 0x80) ? 0x1b : 0));
        const uint8_t s3 = s2 ^ s1;
        K->te[x] = (uint32_t)s2 << 24 | (uint32_t)s1 << 16 | (uint32_t)s1 << 8 | s3;
    }
    aes_expand_host(key, 8, sb, K->rk256);
    aes_expand_host(key + 32, 4, sb, K->rk128);
    uint8_t rb[16];
    memcpy(rb, key + 48, 16);
    rb[3] &= 15; rb[7] &= 15; rb[11] &= 15; rb[15] &= 15;
    rb[4] &= 252; rb[8] &= 252; rb[12] &= 252;
    uint64_t t0 = 0, t1 = 0;
    for (int i = 7; i >= 0; i--) {
        t0 = t0 << 8 | rb[i];
        t1 = t1 << 8 | rb[8 + i];
    }
    const uint32_t r[5] = {(uint32_t)(t0 & 0x3ffffff), (uint32_t)((t0 >> 26) & 0x3ffffff),
                           (uint32_t)(((t0 >> 52) | (t1 << 12)) & 0x3ffffff),
                           (uint32_t)((t1 >> 14) & 0x3ffffff), (uint32_t)((t1 >> 40) & 0x3ffffff)};
    // table rows: the shared pmul, then pfull, so every limb is below 2^26 (the
    // bound of pmul's b operand, rcdc_p1305.h)
    auto mul = [](const uint32_t a[5], const uint32_t b[5], uint32_t out[5]) {
        p1305::P26 x;
        memcpy(x.h, a, sizeof x.h);
        x = p1305::pmul(x, b);
        p1305::pfull(x);
        memcpy(out, x.h, sizeof x.h);
    };
    const uint32_t one[5] = {1, 0, 0, 0, 0};
    memcpy(K->rpow[0], one, sizeof one);
    for (int i = 1; i <= 64; i++) mul(K->rpow[i - 1], r, K->rpow[i]);
    memcpy(K->r2j[0], r, sizeof r);
    for (int j = 1; j < 32; j++) mul(K->r2j[j - 1], K->r2j[j - 1], K->r2j[j]);
}

// ---- blob encryption: batches, pack files --------------------------------------

// A list of blobs over one input base, cut into units of kAeadUnitBlocks.
struct AeadBatch {
    const uint8_t *in = nullptr;
    std::vector<AeadBlob> blobs;
    std::vector<AeadUnit> units;
    std::vector<uint32_t> unit0;  // per blob + 1 (closed by aead_launch)
};

inline rcdc_status aead_add(AeadBatch &B, const AeadBlob &b, uint32_t caller_index, char *msg) {
    const uint64_t nb = (b.len + 15) / 16;
    if (nb >= (1ull << 32)) return refuse(msg, RCDC_ERR_UNSUPPORTED, "blob %u too large", caller_index);
    const uint32_t bi = (uint32_t)B.blobs.size();
    B.unit0.push_back((uint32_t)B.units.size());
    B.blobs.push_back(b);
    for (uint64_t b0 = 0; b0 < nb; b0 += kAeadUnitBlocks)
        B.units.push_back({bi, (uint32_t)b0, (uint32_t)std::min<uint64_t>(nb, b0 + kAeadUnitBlocks), 0});
    return RCDC_OK;
}

// Device range copies: units of {src, dst, len, source base address}, at
// most 1 MiB each.
inline void push_copy(std::vector<uint64_t> &copies, const void *src_base, uint64_t src, uint64_t dst,
                      uint64_t len) {
    for (uint64_t c = 0; c < len; c += 1u << 20) {
        copies.push_back(src + c);
        copies.push_back(dst + c);
        copies.push_back(std::min<uint64_t>(1u << 20, len - c));
        copies.push_back((uint64_t)(uintptr_t)src_base);
    }
}

// What a pack_build call uploads and launches.
struct PackPlan {
    AeadBatch data;     // the blobs to seal (not raw), over d_in
    AeadBatch headers;  // one per pack, over `hdr` (in == nullptr: the staging buffer)
    std::vector<uint8_t> hdr;      // every pack's header entries, + 4 bytes of padding
    std::vector<uint64_t> copies;  // raw: the sealed blobs' copy units
};

// Pack files (blob/packer.rs:615-655, 693-735; repofile/packfile.rs): blobs
// sealed back to back, then the sealed header (one HeaderEntry per blob:
// type, u32 length, [u32 raw length], id) and its u32 length.
// raw (add_raw): the blobs at in_off are sealed already (len = sealed bytes,
// >= 32); they are copied into place and only the headers are sealed.
// srcs (raw only, n_src > 0): blob i's bytes are at srcs[blobs[i].pad] +
// in_off (rcdc_pack_build_raw_multi); otherwise at d_in + in_off.
// Sets every pack's header_len and size, and blob_offsets (optional).
// have_ctx_key: the caller's context and key are not null.
inline rcdc_status pack_plan(bool have_ctx_key, const void *d_in, const rcdc_pack_blob *blobs,
                             uint32_t nblobs, rcdc_pack *packs, uint32_t npacks, const void *d_out,
                             uint64_t out_len, uint32_t *blob_offsets, bool raw,
                             const void *const *srcs, uint32_t n_src, PackPlan &pp, char *msg) {
    if (n_src) {
        if (!srcs) return refuse(msg, RCDC_ERR_INVALID_INPUT, "null argument");
        for (uint32_t j = 0; j < n_src; j++)
            if (!srcs[j]) return refuse(msg, RCDC_ERR_INVALID_INPUT, "source %u is null", j);
        d_in = srcs[0];
    }
    if (!have_ctx_key || (npacks && (!packs || !d_out)) || (nblobs && (!blobs || !d_in)))
        return refuse(msg, RCDC_ERR_INVALID_INPUT, "null argument");
    pp.data.in = (const uint8_t *)d_in;
    pp.headers.in = nullptr;  // headers: from the staging buffer
    std::vector<uint8_t> &hdr = pp.hdr;
    rcdc_status rs;
    for (uint32_t p = 0; p < npacks; p++) {
        rcdc_pack &P = packs[p];
        if (P.nblobs == 0 || (uint64_t)P.blob0 + P.nblobs > nblobs)
            return refuse(msg, RCDC_ERR_INVALID_INPUT, "pack %u: blobs [%u, +%u) of %u", p, P.blob0,
                          P.nblobs, nblobs);
        uint64_t off = 0;
        const size_t h0 = hdr.size();
        for (uint32_t i = P.blob0; i < P.blob0 + P.nblobs; i++) {
            const rcdc_pack_blob &b = blobs[i];
            if (b.type > 1) return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u: type %u", i, b.type);
            if (raw && b.len < 32)
                return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u: %u sealed bytes (< 32)", i, b.len);
            if (!raw && b.len > 0xFFFFFFFFu - 32u)
                return refuse(msg, RCDC_ERR_UNSUPPORTED, "blob %u: %u bytes", i, b.len);
            const uint32_t sealed = raw ? b.len : b.len + 32u;
            if (blob_offsets) blob_offsets[i] = (uint32_t)off;
            if (raw) {
                if (n_src && b.pad >= n_src)
                    return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u: source %u of %u", i, b.pad, n_src);
                push_copy(pp.copies, n_src ? srcs[b.pad] : d_in, b.in_off, P.out_off + off, sealed);
            } else {
                AeadBlob a{};
                a.in_off = b.in_off;
                a.len = b.len;
                a.out_off = P.out_off + off;
                memcpy(a.nonce, b.nonce, 16);
                if ((rs = aead_add(pp.data, a, i, msg))) return rs;
            }
            // HeaderEntry (packfile.rs:88-124, little-endian)
            hdr.push_back((uint8_t)(b.type + (b.uncompressed_len ? 2u : 0u)));
            for (int j = 0; j < 4; j++) hdr.push_back((uint8_t)(sealed >> (8 * j)));
            if (b.uncompressed_len)
                for (int j = 0; j < 4; j++) hdr.push_back((uint8_t)(b.uncompressed_len >> (8 * j)));
            hdr.insert(hdr.end(), b.id, b.id + 32);
            off += sealed;
        }
        const uint64_t hlen = hdr.size() - h0;
        P.header_len = (uint32_t)(hlen + 32);
        P.size = off + hlen + 32 + 4;
        if (P.size > 0xFFFFFFFFull)  // packer.rs:58 MAX_SIZE; offsets are u32
            return refuse(msg, RCDC_ERR_UNSUPPORTED, "pack %u: %llu bytes", p, (unsigned long long)P.size);
        if (P.out_off + P.size > out_len)
            return refuse(msg, RCDC_ERR_INVALID_INPUT,
                          "pack %u does not fit the output (%llu + %llu > %llu)", p,
                          (unsigned long long)P.out_off, (unsigned long long)P.size,
                          (unsigned long long)out_len);
        AeadBlob h{};
        h.in_off = h0;
        h.len = hlen;
        h.out_off = P.out_off + off;
        memcpy(h.nonce, P.header_nonce, 16);
        h.flags = kAeadAppendLen;
        if ((rs = aead_add(pp.headers, h, p, msg))) return rs;
    }
    hdr.resize(hdr.size() + 4, 0);  // the kernel may read 3 bytes past a blob
    return RCDC_OK;
}

// ---- blob compression: launch windows ------------------------------------------

inline uint64_t zstd_blocks(uint64_t len) { return len ? (len + kZstdBlock - 1) / kZstdBlock : 1; }

// Whole blobs of at most `wblocks` blocks together (a blob with more: a
// window of its own); a window's kernels see its blobs and blocks only.
struct ZstdWin {
    uint64_t blob0, nblob, blk0, nblk;
};
struct ZstdWindows {
    std::vector<ZstdBlob> blobs;  // blk0 counts from the window's first block
    std::vector<ZstdBlk> blks;    // blob counts from the window's first blob
    std::vector<ZstdWin> wins;
    uint64_t maxw = 0;  // blocks of the largest window
};

// descriptors of every window (block indices relative to the window,
// blob indices too), uploaded once
inline ZstdWindows zstd_windows(const rcdc_zstd_ref *refs, uint32_t n, uint64_t wblocks) {
    ZstdWindows W;
    for (uint32_t i = 0; i < n;) {
        ZstdWin w{W.blobs.size(), 0, W.blks.size(), 0};
        while (i < n) {
            const uint64_t nb = zstd_blocks(refs[i].len);
            if (w.nblk && w.nblk + nb > wblocks) break;
            ZstdBlob B{};
            B.in_off = refs[i].in_off;
            B.out_off = refs[i].out_off;
            B.len = (uint32_t)refs[i].len;
            B.blk0 = (uint32_t)w.nblk;
            B.nblk = (uint32_t)nb;
            for (uint64_t k = 0; k < nb; k++) {
                ZstdBlk b{};
                b.blob = (uint32_t)w.nblob;
                b.start = (uint32_t)(k * kZstdBlock);
                b.len = (uint32_t)std::min<uint64_t>(kZstdBlock, refs[i].len - k * kZstdBlock);
                b.flags = (k == 0 ? 1u : 0u) | (k + 1 == nb ? 2u : 0u);
                W.blks.push_back(b);
            }
            W.blobs.push_back(B);
            w.nblk += nb;
            w.nblob++;
            i++;
        }
        W.maxw = std::max(W.maxw, w.nblk);
        W.wins.push_back(w);
    }
    return W;
}

// ---- frame decompression: workspace and groups -----------------------------------

// The decompressor's workspace for nblk blocks and `data` bytes of literals
// and sequence records: the one place its regions are laid out.
inline ZdxLayout zdx_layout(uint64_t nblk, uint64_t data) {
    auto up = [](uint64_t v) { return (v + 255) & ~255ull; };
    ZdxLayout l;
    l.blk_off = 0;
    l.blk_cap = nblk * sizeof(ZdxBlk);
    l.res_off = up(l.blk_off + l.blk_cap);
    l.res_cap = nblk * sizeof(ZdxRes);
    l.data_off = up(l.res_off + l.res_cap);
    l.data_cap = data;
    l.total = up(l.data_off + l.data_cap);
    return l;
}

struct ZdxGroup {
    uint32_t a, b;  // frames [a, b)
    uint64_t nblk, data;
};
struct ZdxGroups {
    std::vector<ZdxGroup> groups;
    std::vector<ZdxPlace> place;  // per frame, relative to its group
    uint64_t peak = 0;            // the largest group's workspace
};

// groups of whole frames within the cap (a frame above it: a group of its own)
inline ZdxGroups zdx_groups(const ZdxFrame *hf, uint32_t n, uint64_t ws_max) {
    ZdxGroups R;
    R.place.resize(n);
    for (uint32_t i = 0; i < n;) {
        ZdxGroup G{i, i, 0, 0};
        while (G.b < n) {
            const ZdxFrame &F = hf[G.b];
            const uint64_t need = F.status ? 0 : F.need;
            if (G.b > G.a && (G.data + need > ws_max || G.nblk + F.nblk > (1ull << 31))) break;
            R.place[G.b].blk0 = G.nblk;  // (every block the walk reaches has a slot,
            R.place[G.b].data0 = G.data;  //  also in a frame it then refuses)
            G.nblk += F.nblk;
            G.data += need;
            G.b++;
        }
        R.peak = std::max(R.peak, zdx_layout(G.nblk, G.data).total);
        R.groups.push_back(G);
        i = G.b;
    }
    return R;
}

// One group's work lists, indices counting from its first frame: `list`, the
// frames of the in-order entropy pass, and `order`, every frame, longest
// first.  Adds the group's blocks to the counters (1: parallel, 2: in order,
// 3: treeless).
inline void zdx_group_lists(const ZdxFrame *hf, const rcdc_zstd_dec_ref *refs, const ZdxGroup &G,
                            std::vector<uint32_t> &list, std::vector<uint32_t> &order,
                            uint64_t stats[8]) {
    const uint32_t m = G.b - G.a;
    list.clear();
    order.resize(m);
    for (uint32_t j = 0; j < m; j++) {
        order[j] = j;
        const ZdxFrame &F = hf[G.a + j];
        if (F.status) continue;
        if (F.flags & kZdxInOrder) {
            list.push_back(j);
            stats[2] += F.ncomp;
        } else {
            stats[1] += F.ncomp;
            stats[3] += F.ntreeless;
        }
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return refs[G.a + x].frame_len > refs[G.a + y].frame_len;
    });
}

// ---- blob placement ----------------------------------------------------------------

// Every blob's source range and every destination's range, in order; writes
// each destination's device address to daddr[ndests_total].
inline rcdc_status place_validate(const void *const *d_ins, const uint64_t *in_lens, uint32_t n_ins,
                                  const rcdc_place_blob *blobs, uint32_t nblobs,
                                  const rcdc_place_dest *dests, uint32_t ndests_total,
                                  void *const *d_outs, const uint64_t *out_lens, uint32_t n_outs,
                                  uint64_t *daddr, char *msg) {
    for (uint32_t i = 0; i < nblobs; i++) {
        const rcdc_place_blob &b = blobs[i];
        if (b.src >= n_ins)
            return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u: src %u >= n_ins %u", i, b.src, n_ins);
        if (b.len > in_lens[b.src] || b.in_off > in_lens[b.src] - b.len)
            return refuse(msg, RCDC_ERR_INVALID_INPUT,
                          "blob %u: in_off %llu + len %llu > in_lens[%u] = %llu", i,
                          (unsigned long long)b.in_off, (unsigned long long)b.len, b.src,
                          (unsigned long long)in_lens[b.src]);
        if (b.len && !d_ins[b.src])
            return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u: d_ins[%u] is NULL", i, b.src);
        if ((uint64_t)b.dest0 + b.ndests > ndests_total)
            return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u: dest0 %u + ndests %u > ndests_total %u",
                          i, b.dest0, b.ndests, ndests_total);
        for (uint32_t d = b.dest0; d < b.dest0 + b.ndests; d++) {
            const rcdc_place_dest &o = dests[d];
            if (o.dst >= n_outs)
                return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u, dest %u: dst %u >= n_outs %u", i, d,
                              o.dst, n_outs);
            if (b.len > out_lens[o.dst] || o.out_off > out_lens[o.dst] - b.len)
                return refuse(msg, RCDC_ERR_INVALID_INPUT,
                              "blob %u, dest %u: out_off %llu + len %llu > out_lens[%u] = %llu", i, d,
                              (unsigned long long)o.out_off, (unsigned long long)b.len, o.dst,
                              (unsigned long long)out_lens[o.dst]);
            if (b.len && !d_outs[o.dst])
                return refuse(msg, RCDC_ERR_INVALID_INPUT, "blob %u, dest %u: d_outs[%u] is NULL", i, d,
                              o.dst);
            daddr[d] = (uint64_t)(uintptr_t)d_outs[o.dst] + o.out_off;
        }
    }
    return RCDC_OK;
}

// Where one pass over a call's tiles stands.  Tiles [w0, pos) of the buffers
// (R tiles) are the window being built; windows grow from 4096 tiles,
// doubling.  When the buffers are full the pass starts a new round at 0,
// once the stream has been drained.
struct PlaceWindow {
    uint64_t pos = 0, w0 = 0, w = 4096, rounds = 0;
    uint32_t win = 0;  // windows sent in this round
    uint64_t limit(uint64_t R) const { return std::min(R, w0 + w); }
    bool full() const { return pos - w0 >= w; }  // (otherwise a stop at the limit: the buffers are)
    void sent() {
        w0 = pos;
        w *= 2;
        win++;
    }
    void new_round() {
        pos = w0 = 0;
        win = 0;
        rounds++;
    }
};

// The next tile to make: byte `off` of blob `blob`; blob == nblobs: none left.
struct PlaceCursor {
    uint32_t blob = 0;
    uint64_t off = 0;
};

// Tiles from `cur` on into tiles[*pos ..), until *pos == limit or no tile is
// left; returns the cursor of the next tile.  Blobs without bytes make no
// tile, nor do blobs without a destination unless zero_test.
inline PlaceCursor place_fill(const void *const *d_ins, const rcdc_place_blob *blobs, uint32_t nblobs,
                              const uint64_t *daddr, bool zero_test, PlaceTile *tiles, uint64_t *pos,
                              uint64_t limit, PlaceCursor cur) {
    for (; cur.blob < nblobs; cur.blob++, cur.off = 0) {
        const rcdc_place_blob &b = blobs[cur.blob];
        if (!b.len || (!zero_test && !b.ndests)) continue;
        const uint64_t src = (uint64_t)(uintptr_t)d_ins[b.src] + b.in_off;
        uint64_t aligned = kPlaceAligned;
        for (uint32_t d = b.dest0; d < b.dest0 + b.ndests; d++)
            if ((daddr[d] ^ src) & 15u) aligned = 0;
        for (; cur.off < b.len; cur.off += kPlaceTile) {
            if (*pos == limit) return cur;
            PlaceTile &t = tiles[(*pos)++];
            t.src = src + cur.off;
            t.len = (uint32_t)std::min<uint64_t>(kPlaceTile, b.len - cur.off);
            t.blob = cur.blob;
            t.dest0 = b.dest0;
            t.ndests = b.ndests;
            t.off = cur.off | aligned;
        }
    }
    return cur;
}

}  // namespace plans
}  // namespace rcdc
