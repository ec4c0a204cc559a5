// rcdc_index_parse (include/rcdc.h): index files as JSON text in HBM ->
// the collector's arrays (index/binarysorted.rs:127-163).  gfx950, wave64.
//
// Stage 1, structure: the structural pass of rcdc_json_tiles.h.  The grammar
// has no escapes (ESC false), so a byte is inside a string exactly when an
// odd number of quotes precedes it.  The four kinds of byte it records: '{'
// at depth 4 (a blob object), '{' at depth 2 (a pack object), ']' at depth 4
// (ends a "blobs" array), ']' at depth 2 (ends an array of the root).
//
// Stages 2 and 3, strict parsers, one lane each.  Every byte of a file in G
// is checked by exactly one lane:
//   a blob lane   its object, and the gap after it up to the '{' of the next
//                 blob or the ']' of the array;
//   a pack lane   its object without the blob objects (from the '[' of
//                 "blobs" it checks up to the first '{' or the ']', and goes
//                 on at the recorded ']'), and the gap after it likewise;
//   the file lane everything else: the root object without the pack objects,
//                 and what surrounds it.
// Any lane that fails marks its file, and a marked file is NOT_PARSED: nothing
// of it is collected.
//
// Stage 4, numbering.  One workgroup scans the pack records (collected or
// not, type, blobs) into pack numbers and entry offsets per type; one lane
// per blob then copies its id and loc to its entry.

#include "rcdc_ixparse.h"

namespace {

using namespace rcdc;
using namespace rcdc::jt;

static_assert(kIxBlock == kTileBlock, "the structural kernels run kTileBlock threads");

__device__ __forceinline__ Tiles<rcdc_ixparse_ref> tiles(const IxArgs &a) {
    return {a.json, a.json_len, a.refs, a.tile_first, a.n_files, a.n_tiles,
            kIxTile, a.sums,    a.ins,  a.counts,     nullptr,   nullptr};
}

// ---- strict parsers ----------------------------------------------------------

// an integer of G
__device__ __forceinline__ bool parse_u32(Cur &c, uint32_t *out) {
    uint64_t v = 0;
    if (!parse_uint(c, 0xFFFFFFFFull, &v)) return false;
    *out = (uint32_t)v;
    return true;
}

__device__ bool parse_blob(Cur &c, uint32_t id[8], IxBlobTmp *o) {
    if (!c.eat('{')) return false;
    c.ws();
    uint32_t seen = 0;
    o->ulen = 0;
    for (bool more = true; more;) {
        if (!c.eat('"')) return false;
        uint32_t k;
        if (c.lit("id\"", 3)) k = 0;
        else if (c.lit("type\"", 5)) k = 1;
        else if (c.lit("offset\"", 7)) k = 2;
        else if (c.lit("length\"", 7)) k = 3;
        else if (c.lit("uncompressed_length\"", 20)) k = 4;
        else return false;
        if ((seen >> k) & 1u) return false;
        seen |= 1u << k;
        c.ws();
        if (!c.eat(':')) return false;
        c.ws();
        if (k == 0) {
            if (!parse_id(c, id)) return false;
        } else if (k == 1) {
            if (c.lit("\"data\"", 6)) o->type = 0;
            else if (c.lit("\"tree\"", 6)) o->type = 1;
            else return false;
        } else if (k == 2) {
            if (!parse_u32(c, &o->offset)) return false;
        } else if (k == 3) {
            if (!parse_u32(c, &o->length)) return false;
        } else if (!c.lit("null", 4)) {
            if (!parse_u32(c, &o->ulen) || o->ulen == 0) return false;
        }
        if (!after_value(c, &more)) return false;
    }
    return (seen & 15u) == 15u && after_element(c, '{');
}

}  // namespace

// ---- stage 1 ---------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ix_tile_sum_kernel(IxArgs a) {
    tile_sum<false, IxGrammar>(tiles(a));
}

__global__ __launch_bounds__(64) void rcdc_ix_tile_state_kernel(IxArgs a) { tile_state(tiles(a)); }

__global__ __launch_bounds__(256) void rcdc_ix_tile_count_kernel(IxArgs a) {
    tile_count<false, IxGrammar>(tiles(a));
}

__global__ __launch_bounds__(1024) void rcdc_ix_count_scan_kernel(IxArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.counts), a.n_tiles, lds);
}

__global__ __launch_bounds__(256) void rcdc_ix_tile_emit_kernel(IxArgs a) {
    tile_emit<false, IxGrammar>(tiles(a), a.total,
                                [&](int e, uint64_t pos, uint32_t f, const uint32_t *my) {
        if (e == kIxBlob) a.blob_open[my[kIxBlob]] = IxBlobOpen{pos, f, 0u};
        else if (e == kIxPack)
            a.pack_open[my[kIxPack]] = IxPackOpen{pos, f, my[kIxBlob], my[kIxC4], 0u};
        else if (e == kIxC4) a.c4[my[kIxC4]] = IxClose{pos, f, my[kIxBlob]};
        else a.c2[my[kIxC2]] = IxClose{pos, f, my[kIxPack]};
    });
}

// ---- stages 2 and 3 -----------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ix_blob_kernel(IxArgs a) {
    const uint32_t i = blockIdx.x * kIxBlock + threadIdx.x;
    if (i >= a.total.n[kIxBlob]) return;
    const IxBlobOpen r = a.blob_open[i];
    const rcdc_ixparse_ref ref = a.refs[r.ref];
    Cur c = {a.json, r.pos, ref.off + ref.len};
    uint32_t id[8];
    IxBlobTmp o = {0u, 0u, 0u, 0u};
    if (!parse_blob(c, id, &o)) {
        a.file_bad[r.ref] = 1u;
        return;
    }
    u32x4v *d = reinterpret_cast<u32x4v *>(a.tmp_ids + (uint64_t)i * 32u);
    d[0] = u32x4v{id[0], id[1], id[2], id[3]};
    d[1] = u32x4v{id[4], id[5], id[6], id[7]};
    *reinterpret_cast<u32x4v *>(a.tmp_blobs + i) = u32x4v{o.offset, o.length, o.ulen, o.type};
}

namespace {

// null or a string of bytes 0x20..0x7E without '"' and '\'
__device__ bool parse_time(Cur &c) {
    if (c.lit("null", 4)) return true;
    if (!c.eat('"')) return false;
    for (;;) {
        const int ch = c.peek();
        if (ch == '"') break;
        if (ch < 0x20 || ch > 0x7E || ch == '\\') return false;
        c.pos++;
    }
    return c.eat('"');
}

__device__ bool parse_pack(const IxArgs &a, Cur &c, const IxPackOpen &r, IxPackTmp *o) {
    if (!c.eat('{')) return false;
    c.ws();
    uint32_t seen = 0;
    for (bool more = true; more;) {
        if (!c.eat('"')) return false;
        uint32_t k;
        if (c.lit("id\"", 3)) k = 0;
        else if (c.lit("blobs\"", 6)) k = 1;
        else if (c.lit("time\"", 5)) k = 2;
        else if (c.lit("size\"", 5)) k = 3;
        else return false;
        if ((seen >> k) & 1u) return false;
        seen |= 1u << k;
        c.ws();
        if (!c.eat(':')) return false;
        c.ws();
        if (k == 0) {
            if (!parse_id(c, o->id)) return false;
        } else if (k == 1) {
            uint32_t rank = 0;
            if (!skip_array(c, '{', a.c4, r.rank_b, a.total.n[kIxC4], r.ref, &rank)) return false;
            if (rank < r.rank_a) return false;
            o->nblobs = rank - r.rank_a;
        } else if (k == 2) {
            if (!parse_time(c)) return false;
        } else if (!c.lit("null", 4)) {
            if (!parse_u32(c, &o->size)) return false;
            o->has_size = 1u;
        }
        if (!after_value(c, &more)) return false;
    }
    return (seen & 3u) == 3u && after_element(c, '{');
}

// the root object and what surrounds it
__device__ bool parse_root(const IxArgs &a, Cur &c, uint32_t f, IxFileTmp *o) {
    const IxCounts fb = a.counts[a.tile_first[f]], fe = a.counts[a.tile_first[f + 1]];
    uint32_t arrays = fb.n[kIxC2];      // the next ']' at depth 2 of this file
    uint32_t packs_at = fb.n[kIxPack]; // pack opens before the next array
    c.ws();
    if (!c.eat('{')) return false;
    c.ws();
    uint32_t seen = 0;
    for (bool more = true; more;) {
        if (!c.eat('"')) return false;
        uint32_t k;
        if (c.lit("supersedes\"", 11)) k = 0;
        else if (c.lit("packs_to_delete\"", 16)) k = 2;
        else if (c.lit("packs\"", 6)) k = 1;
        else return false;
        if ((seen >> k) & 1u) return false;
        seen |= 1u << k;
        c.ws();
        if (!c.eat(':')) return false;
        c.ws();
        if (k == 0) {
            if (!c.lit("null", 4)) {
                if (!c.eat('[')) return false;
                c.ws();
                if (!c.eat(']')) {
                    for (;;) {
                        uint32_t id[8];
                        if (!parse_id(c, id)) return false;
                        c.ws();
                        if (c.eat(']')) break;
                        if (!c.eat(',')) return false;
                        c.ws();
                    }
                }
                arrays++;  // its ']' is one of the file's at depth 2
            }
        } else {
            uint32_t rank = 0;
            if (!skip_array(c, '{', a.c2, arrays, fe.n[kIxC2], f, &rank)) return false;
            arrays++;
            if (rank < packs_at || rank > fe.n[kIxPack]) return false;
            if (k == 1) {
                o->pack_a = packs_at;
                o->pack_b = rank;
            } else {
                o->ndelete = rank - packs_at;
            }
            packs_at = rank;
        }
        if (!after_value(c, &more)) return false;
    }
    c.ws();
    return (seen & 2u) != 0u && c.pos == c.end;
}

}  // namespace

__global__ __launch_bounds__(256) void rcdc_ix_pack_kernel(IxArgs a) {
    const uint32_t i = blockIdx.x * kIxBlock + threadIdx.x;
    if (i >= a.total.n[kIxPack]) return;
    const IxPackOpen r = a.pack_open[i];
    const rcdc_ixparse_ref ref = a.refs[r.ref];
    Cur c = {a.json, r.pos, ref.off + ref.len};
    IxPackTmp o = {};
    o.blob0 = r.rank_a;
    o.file = r.ref;
    o.ok = parse_pack(a, c, r, &o) ? 1u : 0u;
    if (!o.ok) a.file_bad[r.ref] = 1u;
    a.tmp_packs[i] = o;
}

__global__ __launch_bounds__(256) void rcdc_ix_root_kernel(IxArgs a) {
    const uint32_t f = blockIdx.x * kIxBlock + threadIdx.x;
    if (f >= a.n_files) return;
    const rcdc_ixparse_ref ref = a.refs[f];
    Cur c = {a.json, ref.off, ref.off + ref.len};
    IxFileTmp o = {0u, 0u, 0u, 0u};
    o.ok = parse_root(a, c, f, &o) ? 1u : 0u;
    a.tmp_files[f] = o;
}

// ---- stage 4 ------------------------------------------------------------------------

// A file is in G when its own lane and every blob and pack lane of it agreed;
// the blob and pack kernels have ended, so file_bad is final here.
__global__ __launch_bounds__(256) void rcdc_ix_file_kernel(IxArgs a) {
    const uint32_t f = blockIdx.x * kIxBlock + threadIdx.x;
    if (f >= a.n_files) return;
    IxFileTmp o = a.tmp_files[f];
    if (a.file_bad[f]) o.ok = 0u;
    a.tmp_files[f].ok = o.ok;
    rcdc_ixparse_file r = {};
    r.status = o.ok ? RCDC_IXPARSE_OK : RCDC_IXPARSE_NOT_PARSED;
    r.packs_to_delete = o.ok ? o.ndelete : 0u;
    a.files[f] = r;
}

// One workgroup: what each pack adds (a pack and its blobs, to its type),
// scanned over the packs in order.
__global__ __launch_bounds__(1024) void rcdc_ix_number_kernel(IxArgs a) {
    __shared__ u32x4v lds[16];
    u32x4v *adds = reinterpret_cast<u32x4v *>(a.adds);
    const uint32_t n = a.total.n[kIxPack];
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        IxPackTmp p = a.tmp_packs[i];
        const IxFileTmp ft = a.tmp_files[p.file];
        const bool in = ft.ok && p.ok && i >= ft.pack_a && i < ft.pack_b;
        const uint32_t type = (in && p.nblobs) ? a.tmp_blobs[p.blob0].type : 0u;
        a.tmp_packs[i].collected = in ? 1u : 0u;
        a.tmp_packs[i].type = type;
        u32x4v x = {0u, 0u, 0u, 0u};
        if (in) {
            if (type) { x.y = 1u; x.w = p.nblobs; } else { x.x = 1u; x.z = p.nblobs; }
        }
        adds[i] = x;
    }
    __syncthreads();
    block_scan4(adds, n, lds);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) {
        const IxPackTmp p = a.tmp_packs[i];
        if (!p.collected) continue;
        const u32x4v ex = adds[i];
        const uint32_t number = a.pack_base[p.type] + (p.type ? ex.y : ex.x);
        const uint32_t out = ex.x + ex.y;
        a.tmp_packs[i].number = number;
        a.tmp_packs[i].entry0 = p.type ? ex.w : ex.z;
        a.tmp_packs[i].out = out;
        if (out < a.cap_packs) {  // the bound: always
            uint32_t *w = reinterpret_cast<uint32_t *>(a.packs + out);
            for (int k = 0; k < 8; k++) w[k] = p.id[k];
            w[8] = p.type;
            w[9] = number;
            // pack_size(): the blobs' share is added by the scatter kernel
            a.packs[out].size = p.has_size ? (uint64_t)p.size : 36ull;
        }
        __hip_atomic_fetch_add(&a.files[p.file].packs[p.type], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&a.files[p.file].entries[p.type], p.nblobs, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        const u32x4v tot = adds[n];
        a.result[0] = tot.x;
        a.result[1] = tot.y;
        a.result[2] = tot.z;
        a.result[3] = tot.w;
    }
}

__global__ __launch_bounds__(256) void rcdc_ix_scatter_kernel(IxArgs a) {
    const uint32_t i = blockIdx.x * kIxBlock + threadIdx.x;
    if (i >= a.total.n[kIxBlob]) return;
    // the pack of blob i: the last pack opened with blob_rank <= i
    uint32_t lo = 0, hi = a.total.n[kIxPack];
    if (hi == 0 || a.tmp_packs[0].blob0 > i) return;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.tmp_packs[mid].blob0 <= i) lo = mid; else hi = mid;
    }
    const IxPackTmp *p = a.tmp_packs + lo;
    if (!p->collected || i - p->blob0 >= p->nblobs) return;
    const uint32_t type = p->type;
    const uint64_t dst = (uint64_t)p->entry0 + (i - p->blob0);
    const IxBlobTmp b = a.tmp_blobs[i];
    if (!p->has_size && p->out < a.cap_packs)
        __hip_atomic_fetch_add(&a.packs[p->out].size,
                               (uint64_t)b.length + (b.ulen ? 41u : 37u), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    if (dst >= a.cap_entries) return;  // the bound: never
    if (a.ids[type]) {
        const u32x4v *s = reinterpret_cast<const u32x4v *>(a.tmp_ids + (uint64_t)i * 32u);
        u32x4v *d = reinterpret_cast<u32x4v *>(a.ids[type] + dst * 32u);
        d[0] = s[0];
        d[1] = s[1];
    }
    if (a.locs[type])
        *reinterpret_cast<u32x4v *>(a.locs[type] + dst) =
            u32x4v{p->number, b.offset, b.length, b.ulen};
}

namespace rcdc {

hipError_t launch_ix_structure(const IxArgs &a, hipStream_t st) {
    if (a.n_tiles) {
        RCDC_LAUNCH(rcdc_ix_tile_sum_kernel, blocks(a.n_tiles, kIxBlock / 64), kIxBlock, a);
        RCDC_LAUNCH(rcdc_ix_tile_state_kernel, a.n_files, 64, a);
        RCDC_LAUNCH(rcdc_ix_tile_count_kernel, blocks(a.n_tiles, kIxBlock / 64), kIxBlock, a);
    }
    RCDC_LAUNCH(rcdc_ix_count_scan_kernel, 1, 1024, a);
    return hipSuccess;
}

hipError_t launch_ix_parse(const IxArgs &a, hipStream_t st) {
    const uint32_t n_blobs = a.total.n[kIxBlob], n_packs = a.total.n[kIxPack];
    if (a.n_tiles)
        RCDC_LAUNCH(rcdc_ix_tile_emit_kernel, blocks(a.n_tiles, kIxBlock / 64), kIxBlock, a);
    if (n_blobs) RCDC_LAUNCH(rcdc_ix_blob_kernel, blocks(n_blobs, kIxBlock), kIxBlock, a);
    if (n_packs) RCDC_LAUNCH(rcdc_ix_pack_kernel, blocks(n_packs, kIxBlock), kIxBlock, a);
    RCDC_LAUNCH(rcdc_ix_root_kernel, blocks(a.n_files, kIxBlock), kIxBlock, a);
    RCDC_LAUNCH(rcdc_ix_file_kernel, blocks(a.n_files, kIxBlock), kIxBlock, a);
    RCDC_LAUNCH(rcdc_ix_number_kernel, 1, 1024, a);
    if (n_blobs) RCDC_LAUNCH(rcdc_ix_scatter_kernel, blocks(n_blobs, kIxBlock), kIxBlock, a);
    return hipSuccess;
}

}  // namespace rcdc
