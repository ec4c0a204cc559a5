// rcdc_index_parse (include/rcdc.h): index files as JSON text in HBM ->
// the collector's arrays (index/binarysorted.rs:127-163).  gfx950, wave64.
//
// Stage 1, structure.  The grammar has no escapes, so a byte is inside a
// string exactly when an odd number of quotes precedes it, and the nesting
// depth is the count of brackets outside strings.  A tile (kIxTile bytes, one
// wave, 16 bytes per lane and row) is summarised as a function of the state
// at its first byte (IxTileSum); one wave per file scans its tiles'
// functions into states (IxTileIn); with the state known, the tiles count and
// then write, in order of position, the four kinds of byte the later stages
// start from or jump to: '{' at depth 4 (a blob object), '{' at depth 2 (a
// pack object), ']' at depth 4 (ends a "blobs" array), ']' at depth 2 (ends
// an array of the root).  Stage 1 validates nothing.
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
// A lane's parse follows the same quotes and brackets as stage 1, so where a
// lane expects the next object to begin, stage 1 has recorded an open of
// that kind and a lane of its own checks it; the recorded ']' is the one the
// chain of those lanes ends at.  Any lane that fails marks its file, and a
// marked file is NOT_PARSED: nothing of it is collected.
//
// Stage 4, numbering.  One workgroup scans the pack records (collected or
// not, type, blobs) into pack numbers and entry offsets per type; one lane
// per blob then copies its id and loc to its entry.

#include "rcdc_ixparse.h"

namespace {

using namespace rcdc;

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// ---- wave helpers -----------------------------------------------------------

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// g after f, both IxTileSum
__device__ __forceinline__ IxTileSum compose(const IxTileSum &f, const IxTileSum &g) {
    IxTileSum r;
    r.q = f.q ^ g.q;
    r.d0 = f.d0 + (f.q ? g.d1 : g.d0);
    r.d1 = f.d1 + (f.q ? g.d0 : g.d1);
    return r;
}

__device__ __forceinline__ IxTileSum wave_incl_compose(IxTileSum v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        IxTileSum o;
        o.d0 = __shfl_up(v.d0, d, 64);
        o.d1 = __shfl_up(v.d1, d, 64);
        o.q = __shfl_up(v.q, d, 64);
        if (lane >= d) v = compose(o, v);
    }
    return v;
}

__device__ __forceinline__ IxTileIn apply(const IxTileIn &s, const IxTileSum &f) {
    IxTileIn r;
    r.instr = s.instr ^ f.q;
    r.depth = s.depth + (s.instr ? f.d1 : f.d0);
    return r;
}

// ---- a tile's bytes ------------------------------------------------------------

// The file of tile t (uniform over the wave): the last f with tile_first[f] <= t.
__device__ __forceinline__ uint32_t file_of_tile(const IxArgs &a, uint32_t t) {
    uint32_t lo = 0, hi = a.n_files;  // tile_first[lo] <= t < tile_first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

struct Chunk {
    uint8_t b[16];
    uint32_t valid;   // bit j: byte j belongs to the file
    uint64_t pos;     // arena offset of byte 0 (may wrap below 0 for the arena's first chunk)
};

// The 16 bytes of this lane in row `row` of tile `k` of the file [lo, hi).
// Chunks are 16-byte aligned addresses; one that lies wholly in the arena is
// one dword x4 load, the arena's ragged first and last chunk go byte by byte.
__device__ __forceinline__ Chunk load_chunk(const IxArgs &a, uint64_t lo, uint64_t hi, uint32_t k,
                                            uint32_t row) {
    const uint64_t mis = (uint64_t)(uintptr_t)a.json & 15u;
    const uint64_t v0 = (lo + mis) & ~15ull;  // in "arena offset + mis": aligned when a multiple of 16
    const uint64_t v = v0 + (uint64_t)k * kIxTile + (uint64_t)row * kIxRow + lane_id() * 16u;
    Chunk c;
    c.pos = v - mis;
    c.valid = 0;
    // the chunk's bytes [from, to) are the file's
    const int64_t s = (int64_t)v - (int64_t)mis;
    const int64_t from = (int64_t)lo > s ? (int64_t)lo - s : 0;
    const int64_t to = (int64_t)hi - s < 16 ? (int64_t)hi - s : 16;
    if (to <= from) {
#pragma unroll
        for (int j = 0; j < 16; j++) c.b[j] = ' ';
        return c;
    }
    c.valid = ((1u << to) - 1u) & ~((1u << from) - 1u);
    if (s >= 0 && (uint64_t)s + 16u <= a.json_len) {
        const u32x4v w = *reinterpret_cast<const u32x4v *>(a.json + s);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 16; j++) c.b[j] = (uint8_t)(ws[j >> 2] >> ((j & 3) * 8));
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            c.b[j] = ((c.valid >> j) & 1u) ? a.json[s + j] : (uint8_t)' ';
    }
    return c;
}

__device__ __forceinline__ int bracket(uint8_t c) {
    return (c == '{' || c == '[') ? 1 : (c == '}' || c == ']') ? -1 : 0;
}

__device__ __forceinline__ IxTileSum chunk_sum(const Chunk &c) {
    IxTileSum s = {0, 0, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        const uint8_t ch = c.b[j];
        if (ch == '"') {
            s.q ^= 1u;
        } else {
            const int d = bracket(ch);
            if (s.q) s.d1 += d; else s.d0 += d;
        }
    }
    return s;
}

// The state at this lane's chunk, given the state `in` at the row's first
// byte; *total: the row as a function.
__device__ __forceinline__ IxTileIn lane_state(const IxTileIn &in, const IxTileSum &mine,
                                               IxTileSum *total) {
    const IxTileSum inc = wave_incl_compose(mine);
    IxTileSum ex;
    ex.d0 = __shfl_up(inc.d0, 1, 64);
    ex.d1 = __shfl_up(inc.d1, 1, 64);
    ex.q = __shfl_up(inc.q, 1, 64);
    if (lane_id() == 0) ex = IxTileSum{0, 0, 0u};
    total->d0 = __shfl(inc.d0, 63, 64);
    total->d1 = __shfl(inc.d1, 63, 64);
    total->q = __shfl(inc.q, 63, 64);
    return apply(in, ex);
}

// kinds of event: 0 blob open, 1 pack open, 2 ']' at depth 4, 3 ']' at depth 2; -1 none
__device__ __forceinline__ int event_of(uint8_t ch, int32_t depth) {
    if (ch == '{') return depth == 4 ? 0 : depth == 2 ? 1 : -1;
    if (ch == ']') return depth == 4 ? 2 : depth == 2 ? 3 : -1;
    return -1;
}

__device__ __forceinline__ void chunk_counts(const Chunk &c, IxTileIn s, uint32_t n[4]) {
    n[0] = n[1] = n[2] = n[3] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        const uint8_t ch = c.b[j];
        if (ch == '"') {
            s.instr ^= 1u;
        } else if (!s.instr) {
            const int e = event_of(ch, s.depth);
            if (e >= 0) n[e]++;
            s.depth += bracket(ch);
        }
    }
}

// ---- strict parsers ----------------------------------------------------------

struct Cur {
    const uint8_t *j;
    uint64_t pos, end;
    __device__ __forceinline__ int peek() const { return pos < end ? (int)j[pos] : -1; }
    __device__ __forceinline__ bool eat(int c) {
        if (peek() != c) return false;
        pos++;
        return true;
    }
    __device__ __forceinline__ void ws() {
        while (pos < end) {
            const uint8_t c = j[pos];
            if (c != ' ' && c != '\t' && c != '\n' && c != '\r') break;
            pos++;
        }
    }
    // the n bytes of s, or nothing consumed
    __device__ __forceinline__ bool lit(const char *s, uint32_t n) {
        if (end - pos < n) return false;
        for (uint32_t i = 0; i < n; i++)
            if (j[pos + i] != (uint8_t)s[i]) return false;
        pos += n;
        return true;
    }
};

__device__ __forceinline__ int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// "<64 hex digits>" -> 32 bytes as 8 little-endian words (memory order)
__device__ bool parse_id(Cur &c, uint32_t id[8]) {
    if (!c.eat('"')) return false;
    if (c.end - c.pos < 65) return false;
    for (int w = 0; w < 8; w++) {
        uint32_t v = 0;
        for (int b = 0; b < 4; b++) {
            const int h = hexval(c.j[c.pos]), l = hexval(c.j[c.pos + 1]);
            if ((h | l) < 0) return false;
            v |= (uint32_t)(h * 16 + l) << (b * 8);
            c.pos += 2;
        }
        id[w] = v;
    }
    return c.eat('"');
}

// an integer of G; what follows it is the caller's to check
__device__ bool parse_uint(Cur &c, uint32_t *out) {
    int ch = c.peek();
    if (ch < '0' || ch > '9') return false;
    c.pos++;
    uint64_t v = (uint64_t)(ch - '0');
    const bool zero = ch == '0';
    for (;;) {
        ch = c.peek();
        if (ch < '0' || ch > '9') break;
        if (zero) return false;  // a leading zero
        v = v * 10u + (uint64_t)(ch - '0');
        if (v > 0xFFFFFFFFull) return false;
        c.pos++;
    }
    *out = (uint32_t)v;
    return true;
}

// after a member's value: true with *more when a ',' and the next key's quote
// follow, true with !*more when the object's '}' does
__device__ __forceinline__ bool after_value(Cur &c, bool *more) {
    c.ws();
    if (c.eat(',')) {
        c.ws();
        *more = true;
        return true;
    }
    *more = false;
    return c.eat('}');
}

// after an object of an array: ws, then ',' ws and the next object's '{'
// (left to its own lane), or the array's ']' (left to the lane that owns it)
__device__ __forceinline__ bool after_object(Cur &c) {
    c.ws();
    if (c.eat(',')) {
        c.ws();
        return c.peek() == '{';
    }
    return c.peek() == ']';
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
            if (!parse_uint(c, &o->offset)) return false;
        } else if (k == 3) {
            if (!parse_uint(c, &o->length)) return false;
        } else if (!c.lit("null", 4)) {
            if (!parse_uint(c, &o->ulen) || o->ulen == 0) return false;
        }
        if (!after_value(c, &more)) return false;
    }
    return (seen & 15u) == 15u && after_object(c);
}

}  // namespace

// ---- stage 1 ---------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ix_tile_sum_kernel(IxArgs a) {
    const uint32_t t = blockIdx.x * (kIxBlock / 64) + threadIdx.x / 64;
    if (t >= a.n_tiles) return;
    const uint32_t f = file_of_tile(a, t);
    const uint64_t lo = a.refs[f].off, hi = lo + a.refs[f].len;
    IxTileSum tile = {0, 0, 0u};
    for (uint32_t row = 0; row < kIxRows; row++) {
        const Chunk c = load_chunk(a, lo, hi, t - a.tile_first[f], row);
        IxTileSum total;
        (void)lane_state(IxTileIn{0u, 0}, chunk_sum(c), &total);
        tile = compose(tile, total);
    }
    if (lane_id() == 0) a.sums[t] = tile;
}

// one wave per file: the state at the first byte of each of its tiles
__global__ __launch_bounds__(64) void rcdc_ix_tile_state_kernel(IxArgs a) {
    const uint32_t f = blockIdx.x;
    const uint32_t t0 = a.tile_first[f], t1 = a.tile_first[f + 1];
    IxTileIn carry = {0u, 0};
    for (uint32_t base = t0; base < t1; base += 64) {
        const uint32_t t = base + lane_id();
        IxTileSum mine = {0, 0, 0u};
        if (t < t1) mine = a.sums[t];
        IxTileSum total;
        const IxTileIn in = lane_state(carry, mine, &total);
        if (t < t1) a.ins[t] = in;
        carry = apply(carry, total);
    }
}

__global__ __launch_bounds__(256) void rcdc_ix_tile_count_kernel(IxArgs a) {
    const uint32_t t = blockIdx.x * (kIxBlock / 64) + threadIdx.x / 64;
    if (t >= a.n_tiles) return;
    const uint32_t f = file_of_tile(a, t);
    const uint64_t lo = a.refs[f].off, hi = lo + a.refs[f].len;
    IxTileIn in = a.ins[t];
    uint32_t sum[4] = {0, 0, 0, 0};
    for (uint32_t row = 0; row < kIxRows; row++) {
        const Chunk c = load_chunk(a, lo, hi, t - a.tile_first[f], row);
        IxTileSum total;
        const IxTileIn s = lane_state(in, chunk_sum(c), &total);
        uint32_t n[4];
        chunk_counts(c, s, n);
        for (int e = 0; e < 4; e++) sum[e] += n[e];
        in = apply(in, total);
    }
    for (int e = 0; e < 4; e++) sum[e] = __shfl(wave_incl_add(sum[e]), 63, 64);
    if (lane_id() == 0) a.counts[t] = IxCounts{sum[0], sum[1], sum[2], sum[3]};
}

// Exclusive scan of n records of four uint32 in place, the totals to v[n]:
// one workgroup of 1024, a chunk of 1024 records per pass.
__device__ void block_scan4(u32x4v *v, uint32_t n, u32x4v *lds /* 16 */) {
    const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
    u32x4v carry = {0u, 0u, 0u, 0u};
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        u32x4v x = {0u, 0u, 0u, 0u};
        if (i < n) x = v[i];
        u32x4v inc;
        inc.x = wave_incl_add(x.x);
        inc.y = wave_incl_add(x.y);
        inc.z = wave_incl_add(x.z);
        inc.w = wave_incl_add(x.w);
        __syncthreads();  // the previous pass has read lds
        if (lane == 63) lds[wave] = inc;
        __syncthreads();
        u32x4v before = carry, all = carry;
        for (uint32_t w = 0; w < 16; w++) {
            const u32x4v s = lds[w];
            if (w < wave) before += s;
            all += s;
        }
        if (i < n) v[i] = before + inc - x;
        carry = all;
    }
    if (threadIdx.x == 0) v[n] = carry;
}

__global__ __launch_bounds__(1024) void rcdc_ix_count_scan_kernel(IxArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.counts), a.n_tiles, lds);
}

__global__ __launch_bounds__(256) void rcdc_ix_tile_emit_kernel(IxArgs a) {
    const uint32_t t = blockIdx.x * (kIxBlock / 64) + threadIdx.x / 64;
    if (t >= a.n_tiles) return;
    const uint32_t f = file_of_tile(a, t);
    const uint64_t lo = a.refs[f].off, hi = lo + a.refs[f].len;
    IxTileIn in = a.ins[t];
    const IxCounts before = a.counts[t];
    uint32_t at[4] = {before.blobs, before.packs, before.c4, before.c2};  // before this row
    const uint32_t cap[4] = {a.total.blobs, a.total.packs, a.total.c4, a.total.c2};
    for (uint32_t row = 0; row < kIxRows; row++) {
        const Chunk c = load_chunk(a, lo, hi, t - a.tile_first[f], row);
        IxTileSum total;
        IxTileIn s = lane_state(in, chunk_sum(c), &total);
        uint32_t n[4], my[4];
        chunk_counts(c, s, n);
        for (int e = 0; e < 4; e++) {
            const uint32_t inc = wave_incl_add(n[e]);
            my[e] = at[e] + inc - n[e];
            at[e] += __shfl(inc, 63, 64);
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (!((c.valid >> j) & 1u)) continue;
            const uint8_t ch = c.b[j];
            if (ch == '"') {
                s.instr ^= 1u;
            } else if (!s.instr) {
                const int e = event_of(ch, s.depth);
                const uint64_t pos = c.pos + (uint64_t)j;
                if (e >= 0 && my[e] < cap[e]) {  // the counts of the pass before: always within
                    if (e == 0) a.blob_open[my[0]] = IxBlobOpen{pos, f, 0u};
                    else if (e == 1) a.pack_open[my[1]] = IxPackOpen{pos, f, my[0], my[2], 0u};
                    else if (e == 2) a.c4[my[2]] = IxClose{pos, f, my[0]};
                    else a.c2[my[3]] = IxClose{pos, f, my[1]};
                }
                if (e >= 0) my[e]++;
                s.depth += bracket(ch);
            }
        }
        in = apply(in, total);
    }
}

// ---- stages 2 and 3 -----------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ix_blob_kernel(IxArgs a) {
    const uint32_t i = blockIdx.x * kIxBlock + threadIdx.x;
    if (i >= a.total.blobs) return;
    const IxBlobOpen r = a.blob_open[i];
    const rcdc_ixparse_ref ref = a.refs[r.file];
    Cur c = {a.json, r.pos, ref.off + ref.len};
    uint32_t id[8];
    IxBlobTmp o = {0u, 0u, 0u, 0u};
    if (!parse_blob(c, id, &o)) {
        a.file_bad[r.file] = 1u;
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

// At the '[' of an array of objects whose ']' stage 1 recorded as cl (of the
// same file): '[' ws, then the first object's '{' or the ']' itself; the
// cursor goes on after the ']'.
__device__ bool skip_array(Cur &c, const IxClose *cl, uint32_t k, uint32_t n, uint32_t file,
                           uint32_t *rank) {
    if (!c.eat('[')) return false;
    c.ws();
    const int ch = c.peek();
    if (ch != '{' && ch != ']') return false;
    if (k >= n) return false;
    const IxClose r = cl[k];
    if (r.file != file || r.pos < c.pos || r.pos >= c.end) return false;
    *rank = r.rank;
    c.pos = r.pos + 1;
    return true;
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
            if (!skip_array(c, a.c4, r.c4_rank, a.total.c4, r.file, &rank)) return false;
            if (rank < r.blob_rank) return false;
            o->nblobs = rank - r.blob_rank;
        } else if (k == 2) {
            if (!parse_time(c)) return false;
        } else if (!c.lit("null", 4)) {
            if (!parse_uint(c, &o->size)) return false;
            o->has_size = 1u;
        }
        if (!after_value(c, &more)) return false;
    }
    return (seen & 3u) == 3u && after_object(c);
}

// the root object and what surrounds it
__device__ bool parse_root(const IxArgs &a, Cur &c, uint32_t f, IxFileTmp *o) {
    const IxCounts fb = a.counts[a.tile_first[f]], fe = a.counts[a.tile_first[f + 1]];
    uint32_t arrays = fb.c2;      // the next ']' at depth 2 of this file
    uint32_t packs_at = fb.packs; // pack opens before the next array
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
            if (!skip_array(c, a.c2, arrays, fe.c2, f, &rank)) return false;
            arrays++;
            if (rank < packs_at || rank > fe.packs) return false;
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
    if (i >= a.total.packs) return;
    const IxPackOpen r = a.pack_open[i];
    const rcdc_ixparse_ref ref = a.refs[r.file];
    Cur c = {a.json, r.pos, ref.off + ref.len};
    IxPackTmp o = {};
    o.blob0 = r.blob_rank;
    o.file = r.file;
    o.ok = parse_pack(a, c, r, &o) ? 1u : 0u;
    if (!o.ok) a.file_bad[r.file] = 1u;
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
    const uint32_t n = a.total.packs;
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
    if (i >= a.total.blobs) return;
    // the pack of blob i: the last pack opened with blob_rank <= i
    uint32_t lo = 0, hi = a.total.packs;
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

static inline uint32_t ix_blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

#define IX_LAUNCH(kernel, grid, block, ...)                                        \
    do {                                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);   \
        if (hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return e_;        \
    } while (0)

hipError_t launch_ix_structure(const IxArgs &a, hipStream_t st) {
    if (a.n_tiles) {
        IX_LAUNCH(rcdc_ix_tile_sum_kernel, ix_blocks(a.n_tiles, kIxBlock / 64), kIxBlock, a);
        IX_LAUNCH(rcdc_ix_tile_state_kernel, a.n_files, 64, a);
        IX_LAUNCH(rcdc_ix_tile_count_kernel, ix_blocks(a.n_tiles, kIxBlock / 64), kIxBlock, a);
    }
    IX_LAUNCH(rcdc_ix_count_scan_kernel, 1, 1024, a);
    return hipSuccess;
}

hipError_t launch_ix_parse(const IxArgs &a, hipStream_t st) {
    if (a.n_tiles)
        IX_LAUNCH(rcdc_ix_tile_emit_kernel, ix_blocks(a.n_tiles, kIxBlock / 64), kIxBlock, a);
    if (a.total.blobs) IX_LAUNCH(rcdc_ix_blob_kernel, ix_blocks(a.total.blobs, kIxBlock), kIxBlock, a);
    if (a.total.packs) IX_LAUNCH(rcdc_ix_pack_kernel, ix_blocks(a.total.packs, kIxBlock), kIxBlock, a);
    IX_LAUNCH(rcdc_ix_root_kernel, ix_blocks(a.n_files, kIxBlock), kIxBlock, a);
    IX_LAUNCH(rcdc_ix_file_kernel, ix_blocks(a.n_files, kIxBlock), kIxBlock, a);
    IX_LAUNCH(rcdc_ix_number_kernel, 1, 1024, a);
    if (a.total.blobs)
        IX_LAUNCH(rcdc_ix_scatter_kernel, ix_blocks(a.total.blobs, kIxBlock), kIxBlock, a);
    return hipSuccess;
}

}  // namespace rcdc
