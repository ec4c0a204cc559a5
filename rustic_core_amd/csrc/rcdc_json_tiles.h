// rcdc_json_tiles.h -- what the device JSON parsers (rcdc_ixparse.hip,
// rcdc_trparse.hip) share: the structural pass over tiles, and the primitives
// of the strict lanes.  The byte-level part is plain C++ and also compiles
// for the host (tools/json_tiles_check.cpp); the wave-level part is for the
// device, wave64.
//
// The structural pass.  Many texts ("refs": files, blobs) lie in one arena.
// A byte is ESCAPED when an odd run of backslashes ends right before it; an
// escaped byte and a backslash that is not escaped count for nothing, every
// other quote toggles the string state, and the nesting depth is the count of
// brackets outside strings.  (A grammar without escapes runs the pass with
// ESC false: a backslash is then a byte like any other.)  Whether a byte is
// escaped depends on the bytes before it alone, not on the string state, so
// it is settled first: a tile (one wave, rows of 16 bytes per lane) looks back
// from its first byte over the backslash run before it, one tile at most (a
// longer run marks the ref), and inside a row every lane learns the parity of
// the run that ends before its chunk from two ballots (a chunk of 16
// backslashes hands the parity on, any other chunk sets it).  Then a tile is
// summarised as a function of the string state at its first byte (TileSum);
// one wave per ref scans its tiles' functions into states (TileIn); with the
// state known, the tiles count and then write, in order of position, the
// four kinds of byte ("events", the Grammar's event_of) the strict lanes
// start from or jump to.  The pass validates nothing.
//
// The strict lanes, one lane each, are the units' own; every byte of an
// accepted ref is checked by exactly one of them.  A lane accepts only what
// follows the same quotes and brackets as the structural pass, so where a
// lane expects the next element to begin, the pass has recorded an open of
// that kind and a lane of its own checks it; the recorded ']' is the one the
// chain of those lanes ends at (skip_array).
#pragma once
#include <stdint.h>

// RCDC_JT_FN marks the byte-level part, as RCDC_P1305_FN does.  Every unit of
// the library, .hip and .cpp, is compiled by hipcc and sees the first form;
// the plain `inline` form is for programs built by the host compiler alone
// (tools/json_tiles_check), which link nothing of the library.
#if defined(__HIPCC__)
#include "rcdc_wave.h"
#define RCDC_JT_FN __host__ __device__ __forceinline__
#define RCDC_JT_UNROLL _Pragma("unroll")
#else
#define RCDC_JT_FN inline
#define RCDC_JT_UNROLL
#endif

namespace rcdc {
namespace jt {

constexpr uint32_t kRow = 64 * 16;    // one 16-byte load per lane
constexpr uint32_t kTileBlock = 256;  // 4 tiles per workgroup

// A tile as a function of the string state at its first byte (whether that
// byte is escaped is known before): the parity of its quotes that count, and
// the change of depth when it starts outside (d0) or inside (d1) a string.
struct TileSum {
    int32_t d0, d1;
    uint32_t q;
};
// The state at a tile's first byte.
struct TileIn {
    uint32_t instr;
    int32_t depth;
};
// Per tile, then (after the scan) before the tile: the events of each kind.
struct TileCounts {
    uint32_t n[4];
};
// The records of the events: where, of which ref, and how many events of
// other kinds (the grammar says which) come before it.
struct TileOpen {
    uint64_t pos;
    uint32_t ref, pad;
};
struct TileOpenRanked {
    uint64_t pos;
    uint32_t ref, rank_a, rank_b, pad;
};
struct TileClose {
    uint64_t pos;
    uint32_t ref, rank;
};

// ---- byte level -------------------------------------------------------------

// g after f
RCDC_JT_FN TileSum compose(const TileSum &f, const TileSum &g) {
    TileSum r;
    r.q = f.q ^ g.q;
    r.d0 = f.d0 + (f.q ? g.d1 : g.d0);
    r.d1 = f.d1 + (f.q ? g.d0 : g.d1);
    return r;
}

RCDC_JT_FN TileIn apply(const TileIn &s, const TileSum &f) {
    TileIn r;
    r.instr = s.instr ^ f.q;
    r.depth = s.depth + (s.instr ? f.d1 : f.d0);
    return r;
}

RCDC_JT_FN int bracket(uint8_t c) {
    return (c == '{' || c == '[') ? 1 : (c == '}' || c == ']') ? -1 : 0;
}

// 16 bytes of a ref at a 16-byte aligned address
struct Chunk {
    uint8_t b[16];    // bytes outside the ref read as spaces
    uint32_t valid;   // bit j: byte j belongs to the ref
    uint64_t pos;     // arena offset of byte 0 (may wrap below 0 for the arena's first chunk)
};

// The chunk as a function of the string state at its first byte; esc: that
// byte is escaped.
template <bool ESC>
RCDC_JT_FN TileSum chunk_sum(const Chunk &c, uint32_t esc) {
    TileSum s = {0, 0, 0u};
    RCDC_JT_UNROLL
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        const uint8_t ch = c.b[j];
        if (ESC && esc) {
            esc = 0u;
        } else if (ESC && ch == '\\') {
            esc = 1u;
        } else if (ch == '"') {
            s.q ^= 1u;
        } else {
            const int d = bracket(ch);
            if (s.q) s.d1 += d; else s.d0 += d;
        }
    }
    return s;
}

// The chunk's events in order of position, given the state s at its first
// byte: on_event(e, j) for an event of kind e = Grammar::event_of(byte, depth)
// >= 0 at byte j.  event_of sees the bytes that count, outside strings, the
// quote that opens a string included.
template <bool ESC, class Grammar, class F>
RCDC_JT_FN void chunk_events(const Chunk &c, uint32_t esc, TileIn s, F &&on_event) {
    RCDC_JT_UNROLL
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        const uint8_t ch = c.b[j];
        if (ESC && esc) {
            esc = 0u;
        } else if (ESC && ch == '\\') {
            esc = 1u;
        } else if (s.instr) {
            if (ch == '"') s.instr = 0u;
        } else {
            const int e = Grammar::event_of(ch, s.depth);
            if (e >= 0) on_event(e, j);
            if (ch == '"') s.instr = 1u;
            s.depth += bracket(ch);
        }
    }
}

template <bool ESC, class Grammar>
RCDC_JT_FN void chunk_counts(const Chunk &c, uint32_t esc, TileIn s, uint32_t n[4]) {
    n[0] = n[1] = n[2] = n[3] = 0;
    chunk_events<ESC, Grammar>(c, esc, s, [&](int e, int) { n[e]++; });
}

// What tile_emit does with a chunk.  my[e]: the events of kind e before the
// chunk; emit(e, pos, my) sees my[] as the counts before its event.  An event
// at or above cap[e] is not emitted (the counts are the pass's before: never).
template <bool ESC, class Grammar, class F>
RCDC_JT_FN void chunk_emit(const Chunk &c, uint32_t esc, TileIn s, uint32_t my[4],
                           const uint32_t cap[4], F &&emit) {
    chunk_events<ESC, Grammar>(c, esc, s, [&](int e, int j) {
        if (my[e] < cap[e]) emit(e, c.pos + (uint64_t)j, my);
        my[e]++;
    });
}

// ---- the strict lanes' primitives ------------------------------------------------

struct Cur {
    const uint8_t *j;
    uint64_t pos, end;
    RCDC_JT_FN int peek() const { return pos < end ? (int)j[pos] : -1; }
    RCDC_JT_FN bool eat(int c) {
        if (peek() != c) return false;
        pos++;
        return true;
    }
    RCDC_JT_FN void ws() {
        while (pos < end) {
            const uint8_t c = j[pos];
            if (c != ' ' && c != '\t' && c != '\n' && c != '\r') break;
            pos++;
        }
    }
    // the n bytes of s, or nothing consumed
    RCDC_JT_FN bool lit(const char *s, uint32_t n) {
        if (end - pos < n) return false;
        for (uint32_t i = 0; i < n; i++)
            if (j[pos + i] != (uint8_t)s[i]) return false;
        pos += n;
        return true;
    }
};

RCDC_JT_FN int hexval(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// "<64 hex digits>" -> 32 bytes as 8 little-endian words (memory order)
RCDC_JT_FN bool parse_id(Cur &c, uint32_t id[8]) {
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

// an integer without a leading zero, of at most `max` (9 or more); what
// follows it is the caller's to check
RCDC_JT_FN bool parse_uint(Cur &c, uint64_t max, uint64_t *out) {
    int ch = c.peek();
    if (ch < '0' || ch > '9') return false;
    c.pos++;
    uint64_t v = (uint64_t)(ch - '0');
    const bool zero = ch == '0';
    for (;;) {
        ch = c.peek();
        if (ch < '0' || ch > '9') break;
        if (zero) return false;  // a leading zero
        const uint64_t d = (uint64_t)(ch - '0');
        if (v > (max - d) / 10u) return false;
        v = v * 10u + d;
        c.pos++;
    }
    *out = v;
    return true;
}

// after a member's value: true with *more when a ',' and the next key's quote
// follow, true with !*more when the object's '}' does
RCDC_JT_FN bool after_value(Cur &c, bool *more) {
    c.ws();
    if (c.eat(',')) {
        c.ws();
        *more = true;
        return true;
    }
    *more = false;
    return c.eat('}');
}

// after an element of an array: ws, then ',' ws and the next element's first
// byte `open` (left to its own lane), or the array's ']' (left to the lane
// that owns it)
RCDC_JT_FN bool after_element(Cur &c, int open) {
    c.ws();
    if (c.eat(',')) {
        c.ws();
        return c.peek() == open;
    }
    return c.peek() == ']';
}

// At the '[' of an array whose elements begin with `open` and have lanes of
// their own, and whose ']' the structural pass recorded as cl[k] (of the same
// ref): '[' ws, then the first element's first byte or the ']' itself; the
// cursor goes on after the ']'.
RCDC_JT_FN bool skip_array(Cur &c, int open, const TileClose *cl, uint32_t k, uint32_t n,
                           uint32_t ref, uint32_t *rank) {
    if (!c.eat('[')) return false;
    c.ws();
    const int ch = c.peek();
    if (ch != open && ch != ']') return false;
    if (k >= n) return false;
    const TileClose r = cl[k];
    if (r.ref != ref || r.pos < c.pos || r.pos >= c.end) return false;
    *rank = r.rank;
    c.pos = r.pos + 1;
    return true;
}

// ---- wave level ---------------------------------------------------------------
#if defined(__HIPCC__)

__device__ __forceinline__ TileSum wave_incl_compose(TileSum v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        TileSum o;
        o.d0 = __shfl_up(v.d0, d, 64);
        o.d1 = __shfl_up(v.d1, d, 64);
        o.q = __shfl_up(v.q, d, 64);
        if (lane >= d) v = compose(o, v);
    }
    return v;
}

// The state at this lane's chunk, given the state `in` at the row's first
// byte; *total: the row as a function.
__device__ __forceinline__ TileIn lane_state(const TileIn &in, const TileSum &mine,
                                             TileSum *total) {
    const TileSum inc = wave_incl_compose(mine);
    TileSum ex;
    ex.d0 = __shfl_up(inc.d0, 1, 64);
    ex.d1 = __shfl_up(inc.d1, 1, 64);
    ex.q = __shfl_up(inc.q, 1, 64);
    if (lane_id() == 0) ex = TileSum{0, 0, 0u};
    total->d0 = __shfl(inc.d0, 63, 64);
    total->d1 = __shfl(inc.d1, 63, 64);
    total->q = __shfl(inc.q, 63, 64);
    return apply(in, ex);
}

// The ref of tile t (uniform over the wave): the last r with tile_first[r] <= t.
__device__ __forceinline__ uint32_t ref_of_tile(const uint32_t *tile_first, uint32_t n, uint32_t t) {
    uint32_t lo = 0, hi = n;  // tile_first[lo] <= t < tile_first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// The 16 bytes of this lane in row `row` of tile `k` of the ref [lo, hi).
// Chunks are 16-byte aligned addresses; one that lies wholly in the arena is
// one dword x4 load, the arena's ragged first and last chunk go byte by byte.
// Bytes outside the ref read as spaces.
__device__ __forceinline__ Chunk load_chunk(const uint8_t *text, uint64_t text_len, uint64_t lo,
                                            uint64_t hi, uint32_t k, uint32_t row,
                                            uint32_t tile_bytes) {
    const uint64_t mis = (uint64_t)(uintptr_t)text & 15u;
    const uint64_t v0 = (lo + mis) & ~15ull;  // in "arena offset + mis": aligned when a multiple of 16
    const uint64_t v = v0 + (uint64_t)k * tile_bytes + (uint64_t)row * kRow + lane_id() * 16u;
    Chunk c;
    c.pos = v - mis;
    c.valid = 0;
    // the chunk's bytes [from, to) are the ref's
    const int64_t s = (int64_t)v - (int64_t)mis;
    const int64_t from = (int64_t)lo > s ? (int64_t)lo - s : 0;
    const int64_t to = (int64_t)hi - s < 16 ? (int64_t)hi - s : 16;
    if (to <= from) {
#pragma unroll
        for (int j = 0; j < 16; j++) c.b[j] = ' ';
        return c;
    }
    c.valid = ((1u << to) - 1u) & ~((1u << from) - 1u);
    if (s >= 0 && (uint64_t)s + 16u <= text_len) {
        const u32x4v w = *reinterpret_cast<const u32x4v *>(text + s);
        uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // the word's four valid bits, each spread over its byte
            const uint32_t bits = (c.valid >> (4 * i)) & 15u;
            const uint32_t m = ((bits * 0x00204081u) & 0x01010101u) * 0xFFu;
            ws[i] = (ws[i] & m) | (0x20202020u & ~m);
        }
#pragma unroll
        for (int j = 0; j < 16; j++) c.b[j] = (uint8_t)(ws[j >> 2] >> ((j & 3) * 8));
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            c.b[j] = ((c.valid >> j) & 1u) ? text[s + j] : (uint8_t)' ';
    }
    return c;
}

// Whether the first byte of tile k (k >= 1) of the ref that starts at lo is
// escaped: the parity of the backslash run before it.  *too_long: the run has
// more than tile_bytes bytes.  Uniform over the wave.
__device__ __forceinline__ uint32_t tile_esc(const uint8_t *text, uint64_t lo, uint32_t k,
                                             uint32_t tile_bytes, bool *too_long) {
    *too_long = false;
    if (k == 0) return 0u;
    const uint64_t mis = (uint64_t)(uintptr_t)text & 15u;
    const uint64_t p = ((lo + mis) & ~15ull) + (uint64_t)k * tile_bytes - mis;  // > lo
    uint32_t run = 0;
    while (run <= tile_bytes && p - run > lo && text[p - 1 - run] == '\\') run++;
    *too_long = run > tile_bytes;
    return run & 1u;
}

// Whether this lane's chunk starts escaped, given that for the row's first
// byte (row_in); *row_out: the same for the byte after the row.  Relies on
// the bytes outside the ref being no backslashes.
__device__ __forceinline__ uint32_t lane_esc(const Chunk &c, uint32_t row_in, uint32_t *row_out) {
    uint32_t tb = 0;  // backslashes at the chunk's end
#pragma unroll
    for (int j = 15; j >= 0; j--) {
        if (c.b[j] != '\\') break;
        tb++;
    }
    const uint64_t sets = ~__ballot(tb == 16u);  // lanes that set the parity; the others hand it on
    const uint64_t par = __ballot(tb & 1u);
    const uint64_t before = sets & ((1ull << lane_id()) - 1ull);
    *row_out = sets ? (uint32_t)(par >> (63 - __clzll((long long)sets))) & 1u : row_in;
    return before ? (uint32_t)(par >> (63 - __clzll((long long)before))) & 1u : row_in;
}

// What the structural kernels read of a unit's arguments.  Ref is {off, len}.
template <class Ref>
struct Tiles {
    const uint8_t *text;
    uint64_t text_len;
    const Ref *refs;
    const uint32_t *tile_first;  // n_refs + 1
    uint32_t n_refs, n_tiles;
    uint32_t tile_bytes;         // one wave, tile_bytes / kRow rows
    TileSum *sums;
    TileIn *ins;
    TileCounts *counts;          // n_tiles + 1: the last one holds the totals
    uint8_t *esc;                // ESC: per tile, its first byte is escaped
    uint32_t *ref_bad;           // ESC: a backslash run longer than a tile marks its ref
};

// One wave's tile in the kernels of kTileBlock threads, or none; the wave's
// row state as it goes through the tile.
template <bool ESC, class Ref>
struct TileWalk {
    uint32_t t, ref, k;
    uint64_t lo, hi;
    uint32_t esc;  // the next row's first byte is escaped

    __device__ __forceinline__ bool begin(const Tiles<Ref> &v) {
        t = blockIdx.x * (kTileBlock / 64) + threadIdx.x / 64;
        if (t >= v.n_tiles) return false;
        ref = ref_of_tile(v.tile_first, v.n_refs, t);
        k = t - v.tile_first[ref];
        lo = v.refs[ref].off;
        hi = lo + v.refs[ref].len;
        esc = 0u;
        return true;
    }
    // the lane's chunk of a row, and *mine: it starts escaped
    __device__ __forceinline__ Chunk row(const Tiles<Ref> &v, uint32_t r, uint32_t *mine) {
        const Chunk c = load_chunk(v.text, v.text_len, lo, hi, k, r, v.tile_bytes);
        *mine = 0u;
        if constexpr (ESC) {
            uint32_t next;
            *mine = lane_esc(c, esc, &next);
            esc = next;
        }
        return c;
    }
};

// ---- the bodies of the structural kernels ---------------------------------------

template <bool ESC, class Grammar, class Ref>
__device__ __forceinline__ void tile_sum(const Tiles<Ref> &v) {
    TileWalk<ESC, Ref> w;
    if (!w.begin(v)) return;
    if constexpr (ESC) {
        bool too_long;
        w.esc = tile_esc(v.text, w.lo, w.k, v.tile_bytes, &too_long);
        if (lane_id() == 0) {
            v.esc[w.t] = (uint8_t)w.esc;
            if (too_long) v.ref_bad[w.ref] = 1u;
        }
    }
    TileSum tile = {0, 0, 0u};
    for (uint32_t r = 0; r < v.tile_bytes / kRow; r++) {
        uint32_t mine;
        const Chunk c = w.row(v, r, &mine);
        TileSum total;
        (void)lane_state(TileIn{0u, 0}, chunk_sum<ESC>(c, mine), &total);
        tile = compose(tile, total);
    }
    if (lane_id() == 0) v.sums[w.t] = tile;
}

// one wave per ref: the state at the first byte of each of its tiles
template <class Ref>
__device__ __forceinline__ void tile_state(const Tiles<Ref> &v) {
    const uint32_t t0 = v.tile_first[blockIdx.x], t1 = v.tile_first[blockIdx.x + 1];
    TileIn carry = {0u, 0};
    for (uint32_t base = t0; base < t1; base += 64) {
        const uint32_t t = base + lane_id();
        TileSum mine = {0, 0, 0u};
        if (t < t1) mine = v.sums[t];
        TileSum total;
        const TileIn in = lane_state(carry, mine, &total);
        if (t < t1) v.ins[t] = in;
        carry = apply(carry, total);
    }
}

template <bool ESC, class Grammar, class Ref>
__device__ __forceinline__ void tile_count(const Tiles<Ref> &v) {
    TileWalk<ESC, Ref> w;
    if (!w.begin(v)) return;
    if constexpr (ESC) w.esc = v.esc[w.t];
    TileIn in = v.ins[w.t];
    uint32_t sum[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < v.tile_bytes / kRow; r++) {
        uint32_t mine;
        const Chunk c = w.row(v, r, &mine);
        TileSum total;
        const TileIn s = lane_state(in, chunk_sum<ESC>(c, mine), &total);
        uint32_t n[4];
        chunk_counts<ESC, Grammar>(c, mine, s, n);
        for (int e = 0; e < 4; e++) sum[e] += n[e];
        in = apply(in, total);
    }
    for (int e = 0; e < 4; e++) sum[e] = __shfl(wave_incl_add(sum[e]), 63, 64);
    if (lane_id() == 0) v.counts[w.t] = TileCounts{{sum[0], sum[1], sum[2], sum[3]}};
}

// counts (scanned) -> the records, through emit(e, pos, ref, my): the event of
// kind e at arena offset pos, my[] the events of each kind before it
template <bool ESC, class Grammar, class Ref, class F>
__device__ __forceinline__ void tile_emit(const Tiles<Ref> &v, const TileCounts &cap, F &&emit) {
    TileWalk<ESC, Ref> w;
    if (!w.begin(v)) return;
    if constexpr (ESC) w.esc = v.esc[w.t];
    TileIn in = v.ins[w.t];
    const TileCounts before = v.counts[w.t];
    uint32_t at[4] = {before.n[0], before.n[1], before.n[2], before.n[3]};  // before this row
    for (uint32_t r = 0; r < v.tile_bytes / kRow; r++) {
        uint32_t mine;
        const Chunk c = w.row(v, r, &mine);
        TileSum total;
        const TileIn s = lane_state(in, chunk_sum<ESC>(c, mine), &total);
        uint32_t n[4], my[4];
        chunk_counts<ESC, Grammar>(c, mine, s, n);
        for (int e = 0; e < 4; e++) {
            const uint32_t inc = wave_incl_add(n[e]);
            my[e] = at[e] + inc - n[e];
            at[e] += __shfl(inc, 63, 64);
        }
        chunk_emit<ESC, Grammar>(
            c, mine, s, my, cap.n,
            [&](int e, uint64_t pos, const uint32_t *m) { emit(e, pos, w.ref, m); });
        in = apply(in, total);
    }
}

#endif  // __HIPCC__

}  // namespace jt
}  // namespace rcdc
