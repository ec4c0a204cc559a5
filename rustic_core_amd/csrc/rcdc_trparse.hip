// rcdc_tree_parse (include/rcdc.h): tree blobs as JSON text in HBM -> the ids
// find_used_blobs and TreeStreamerOnce read out of them (commands/prune.rs:
// 1582-1632, blob/tree.rs:618-800).  gfx950, wave64.  The plan is
// rcdc_ixparse.hip's; what is new is that strings hold backslashes.
// rcdc_tree_nodes is the same kernels with TrArgs::gn set (the grammar G_N)
// and one more at the end, which writes a record per node.
//
// The structural pass.  A byte is ESCAPED when an odd run of backslashes ends
// right before it; an escaped byte and a backslash that is not escaped count
// for nothing, every other quote toggles the string state, and the nesting
// depth is the count of brackets outside strings.  Whether a byte is escaped
// depends on the bytes before it alone, not on the string state, so it is
// settled first: a tile (kTrTile bytes, one wave, 16 bytes per lane and row)
// looks back from its first byte over the backslash run before it, one tile
// at most (a longer run marks the blob), and inside a row every lane learns
// the parity of the run that ends before its chunk from two ballots (a chunk
// of 16 backslashes hands the parity on, any other chunk sets it).  From
// there the pass is G's: a tile is summarised as a function of the string
// state at its first byte (TrTileSum); one wave per blob scans its tiles'
// functions into states (TrTileIn); with the state known, the tiles count and
// then write, in order of position, the four kinds of byte the strict lanes
// start from or jump to: '{' at depth 2 (a node), '"' opening a string at
// depth 4 (an element of "content"), ']' at depth 4 (ends "content" or
// "extended_attributes"), ']' at depth 2 (ends "nodes").  The pass validates
// nothing.
//
// The strict lanes, one lane each.  Every byte of a blob in G_T is checked by
// exactly one lane:
//   an id lane    its string, and the gap after it up to the '"' of the next
//                 id or the ']' of the array: a content array of any length
//                 is spread over the whole device;
//   a node lane   its object without the ids of "content" (from the '[' it
//                 checks up to the first '"' or the ']', and goes on at the
//                 recorded ']'), "extended_attributes" included, and the gap
//                 after it up to the next node's '{' or the ']' of "nodes";
//   the blob lane the root object without the nodes, and what surrounds it.
// A lane accepts only strings whose escapes are JSON's, so its parse follows
// the same quotes and brackets as the structural pass: where a lane expects
// the next id or node to begin, the pass has recorded an open of that kind and
// a lane of its own checks it; the recorded ']' is the one the chain of those
// lanes ends at.  Any lane that fails marks its blob, and a marked blob is
// NOT_PARSED: nothing of it is written.
//
// Numbering.  The node records (content ids of "file" nodes, subtrees, nodes;
// zero for a blob that is not OK) are scanned into positions, a workgroup per
// kTrScan records and one workgroup over their sums; one lane per blob writes
// its record from the scan at its first and last node, one lane per node
// copies its subtree, one lane per id its id.

#include "rcdc_trparse.h"

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

// g after f, both TrTileSum
__device__ __forceinline__ TrTileSum compose(const TrTileSum &f, const TrTileSum &g) {
    TrTileSum r;
    r.q = f.q ^ g.q;
    r.d0 = f.d0 + (f.q ? g.d1 : g.d0);
    r.d1 = f.d1 + (f.q ? g.d0 : g.d1);
    return r;
}

__device__ __forceinline__ TrTileSum wave_incl_compose(TrTileSum v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        TrTileSum o;
        o.d0 = __shfl_up(v.d0, d, 64);
        o.d1 = __shfl_up(v.d1, d, 64);
        o.q = __shfl_up(v.q, d, 64);
        if (lane >= d) v = compose(o, v);
    }
    return v;
}

__device__ __forceinline__ TrTileIn apply(const TrTileIn &s, const TrTileSum &f) {
    TrTileIn r;
    r.instr = s.instr ^ f.q;
    r.depth = s.depth + (s.instr ? f.d1 : f.d0);
    return r;
}

// ---- a tile's bytes ------------------------------------------------------------

// The blob of tile t (uniform over the wave): the last b with tile_first[b] <= t.
__device__ __forceinline__ uint32_t blob_of_tile(const TrArgs &a, uint32_t t) {
    uint32_t lo = 0, hi = a.n_blobs;  // tile_first[lo] <= t < tile_first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

struct Chunk {
    uint8_t b[16];
    uint32_t valid;   // bit j: byte j belongs to the blob
    uint64_t pos;     // arena offset of byte 0 (may wrap below 0 for the arena's first chunk)
};

// The 16 bytes of this lane in row `row` of tile `k` of the blob [lo, hi).
// Chunks are 16-byte aligned addresses; one that lies wholly in the arena is
// one dword x4 load, the arena's ragged first and last chunk go byte by byte.
// Bytes outside the blob read as spaces.
__device__ __forceinline__ Chunk load_chunk(const TrArgs &a, uint64_t lo, uint64_t hi, uint32_t k,
                                            uint32_t row) {
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;
    const uint64_t v0 = (lo + mis) & ~15ull;  // in "arena offset + mis": aligned when a multiple of 16
    const uint64_t v = v0 + (uint64_t)k * kTrTile + (uint64_t)row * kTrRow + lane_id() * 16u;
    Chunk c;
    c.pos = v - mis;
    c.valid = 0;
    // the chunk's bytes [from, to) are the blob's
    const int64_t s = (int64_t)v - (int64_t)mis;
    const int64_t from = (int64_t)lo > s ? (int64_t)lo - s : 0;
    const int64_t to = (int64_t)hi - s < 16 ? (int64_t)hi - s : 16;
    if (to <= from) {
#pragma unroll
        for (int j = 0; j < 16; j++) c.b[j] = ' ';
        return c;
    }
    c.valid = ((1u << to) - 1u) & ~((1u << from) - 1u);
    if (s >= 0 && (uint64_t)s + 16u <= a.text_len) {
        const u32x4v w = *reinterpret_cast<const u32x4v *>(a.text + s);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 16; j++)
            c.b[j] = ((c.valid >> j) & 1u) ? (uint8_t)(ws[j >> 2] >> ((j & 3) * 8)) : (uint8_t)' ';
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            c.b[j] = ((c.valid >> j) & 1u) ? a.text[s + j] : (uint8_t)' ';
    }
    return c;
}

// Whether the first byte of tile k (k >= 1) of the blob [lo, hi) is escaped:
// the parity of the backslash run before it.  *too_long: the run has more
// than kTrTile bytes.  Uniform over the wave.
__device__ __forceinline__ uint32_t tile_esc(const TrArgs &a, uint64_t lo, uint32_t k,
                                             bool *too_long) {
    *too_long = false;
    if (k == 0) return 0u;
    const uint64_t mis = (uint64_t)(uintptr_t)a.text & 15u;
    const uint64_t p = ((lo + mis) & ~15ull) + (uint64_t)k * kTrTile - mis;  // > lo
    uint32_t run = 0;
    while (run <= kTrTile && p - run > lo && a.text[p - 1 - run] == '\\') run++;
    *too_long = run > kTrTile;
    return run & 1u;
}

// Whether this lane's chunk starts escaped, given that for the row's first
// byte (row_in); *row_out: the same for the byte after the row.
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

__device__ __forceinline__ int bracket(uint8_t c) {
    return (c == '{' || c == '[') ? 1 : (c == '}' || c == ']') ? -1 : 0;
}

__device__ __forceinline__ TrTileSum chunk_sum(const Chunk &c, uint32_t esc) {
    TrTileSum s = {0, 0, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        const uint8_t ch = c.b[j];
        if (esc) {
            esc = 0u;
        } else if (ch == '\\') {
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

// The state at this lane's chunk, given the state `in` at the row's first
// byte; *total: the row as a function.
__device__ __forceinline__ TrTileIn lane_state(const TrTileIn &in, const TrTileSum &mine,
                                               TrTileSum *total) {
    const TrTileSum inc = wave_incl_compose(mine);
    TrTileSum ex;
    ex.d0 = __shfl_up(inc.d0, 1, 64);
    ex.d1 = __shfl_up(inc.d1, 1, 64);
    ex.q = __shfl_up(inc.q, 1, 64);
    if (lane_id() == 0) ex = TrTileSum{0, 0, 0u};
    total->d0 = __shfl(inc.d0, 63, 64);
    total->d1 = __shfl(inc.d1, 63, 64);
    total->q = __shfl(inc.q, 63, 64);
    return apply(in, ex);
}

// kinds of event: 0 node open, 1 id open, 2 ']' at depth 4, 3 ']' at depth 2; -1 none.
// ch is a byte that counts, outside a string.
__device__ __forceinline__ int event_of(uint8_t ch, int32_t depth) {
    if (ch == '{') return depth == 2 ? 0 : -1;
    if (ch == '"') return depth == 4 ? 1 : -1;
    if (ch == ']') return depth == 4 ? 2 : depth == 2 ? 3 : -1;
    return -1;
}

__device__ __forceinline__ void chunk_counts(const Chunk &c, uint32_t esc, TrTileIn s,
                                             uint32_t n[4]) {
    n[0] = n[1] = n[2] = n[3] = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (!((c.valid >> j) & 1u)) continue;
        const uint8_t ch = c.b[j];
        if (esc) {
            esc = 0u;
        } else if (ch == '\\') {
            esc = 1u;
        } else if (s.instr) {
            if (ch == '"') s.instr = 0u;
        } else {
            const int e = event_of(ch, s.depth);
            if (e >= 0) n[e]++;
            if (ch == '"') s.instr = 1u;
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

// an integer of G_T of at most `max`; what follows it is the caller's to check
__device__ bool parse_uint(Cur &c, uint64_t max) {
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
    return true;
}

// n continuation bytes, the first of them in [lo, hi]
__device__ __forceinline__ bool utf8_tail(Cur &c, int n, int lo, int hi) {
    for (int i = 0; i < n; i++) {
        const int ch = c.peek();
        if (ch < (i ? 0x80 : lo) || ch > (i ? 0xBF : hi)) return false;
        c.pos++;
    }
    return true;
}

// a string of G_T: 0 where it is none, else kStrOk, with kStrEsc where it
// holds a backslash
constexpr uint32_t kStrOk = 1u, kStrEsc = 2u;
__device__ uint32_t parse_string(Cur &c) {
    if (!c.eat('"')) return 0u;
    uint32_t found = kStrOk;
    for (;;) {
        const int ch = c.peek();
        if (ch < 0x20) return 0u;  // a control byte, or the end of the blob
        c.pos++;
        if (ch == '"') return found;
        if (ch == '\\') {
            found |= kStrEsc;
            const int e = c.peek();
            c.pos++;
            if (e == 'u') {
                if (c.end - c.pos < 4 || c.pos > c.end) return 0u;
                int v = 0;
                for (int i = 0; i < 4; i++) {
                    const int h = hexval(c.j[c.pos + i]);
                    if (h < 0) return 0u;
                    v = v * 16 + h;
                }
                if (v >= 0xD800 && v <= 0xDFFF) return 0u;
                c.pos += 4;
            } else if (e != '"' && e != '\\' && e != '/' && e != 'b' && e != 'f' && e != 'n' &&
                       e != 'r' && e != 't') {
                return 0u;
            }
        } else if (ch >= 0x80) {
            bool ok;
            if (ch >= 0xC2 && ch <= 0xDF) ok = utf8_tail(c, 1, 0x80, 0xBF);
            else if (ch == 0xE0) ok = utf8_tail(c, 2, 0xA0, 0xBF);
            else if (ch == 0xED) ok = utf8_tail(c, 2, 0x80, 0x9F);
            else if (ch >= 0xE1 && ch <= 0xEF) ok = utf8_tail(c, 2, 0x80, 0xBF);
            else if (ch == 0xF0) ok = utf8_tail(c, 3, 0x90, 0xBF);
            else if (ch >= 0xF1 && ch <= 0xF3) ok = utf8_tail(c, 3, 0x80, 0xBF);
            else if (ch == 0xF4) ok = utf8_tail(c, 3, 0x80, 0x8F);
            else ok = false;
            if (!ok) return 0u;
        }
    }
}

__device__ __forceinline__ bool parse_null_or_string(Cur &c) {
    return c.lit("null", 4) || parse_string(c);
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

// after an element of an array: ws, then ',' ws and the next element's first
// byte `open` (left to its own lane), or the array's ']' (left to the lane
// that owns it)
__device__ __forceinline__ bool after_element(Cur &c, int open) {
    c.ws();
    if (c.eat(',')) {
        c.ws();
        return c.peek() == open;
    }
    return c.peek() == ']';
}

// At the '[' of an array whose elements begin with `open` and have lanes of
// their own, and whose ']' the structural pass recorded as cl[k] (of the same
// blob): '[' ws, then the first element's first byte or the ']' itself; the
// cursor goes on after the ']'.
__device__ bool skip_array(Cur &c, int open, const TrClose *cl, uint32_t k, uint32_t n,
                           uint32_t blob, uint32_t *rank) {
    if (!c.eat('[')) return false;
    c.ws();
    const int ch = c.peek();
    if (ch != open && ch != ']') return false;
    if (k >= n) return false;
    const TrClose r = cl[k];
    if (r.blob != blob || r.pos < c.pos || r.pos >= c.end) return false;
    *rank = r.rank;
    c.pos = r.pos + 1;
    return true;
}

// {"name": string, "value": null | string}
__device__ bool parse_xattr(Cur &c) {
    if (!c.eat('{')) return false;
    c.ws();
    uint32_t seen = 0;
    for (bool more = true; more;) {
        if (!c.eat('"')) return false;
        uint32_t k;
        if (c.lit("name\"", 5)) k = 0;
        else if (c.lit("value\"", 6)) k = 1;
        else return false;
        if ((seen >> k) & 1u) return false;
        seen |= 1u << k;
        c.ws();
        if (!c.eat(':')) return false;
        c.ws();
        if (!(k == 0 ? parse_string(c) : parse_null_or_string(c))) return false;
        if (!after_value(c, &more)) return false;
    }
    return (seen & 1u) != 0u;
}

enum NodeKey : uint32_t {
    K_NAME, K_TYPE, K_MODE, K_UID, K_GID, K_MTIME, K_ATIME, K_CTIME, K_USER, K_GROUP, K_INODE,
    K_DEVICE_ID, K_SIZE, K_LINKS, K_DEVICE, K_LINKTARGET, K_LINKTARGET_RAW, K_CONTENT, K_SUBTREE,
    K_XATTRS, K_NONE
};

// the key after its opening quote, the closing quote included
__device__ uint32_t parse_node_key(Cur &c) {
#define TR_KEY(text, k) if (c.lit(text "\"", sizeof(text))) return k
    switch (c.peek()) {
    case 'n': TR_KEY("name", K_NAME); break;
    case 't': TR_KEY("type", K_TYPE); break;
    case 'm': TR_KEY("mode", K_MODE); TR_KEY("mtime", K_MTIME); break;
    case 'u': TR_KEY("uid", K_UID); TR_KEY("user", K_USER); break;
    case 'g': TR_KEY("gid", K_GID); TR_KEY("group", K_GROUP); break;
    case 'a': TR_KEY("atime", K_ATIME); break;
    case 'c': TR_KEY("content", K_CONTENT); TR_KEY("ctime", K_CTIME); break;
    case 'i': TR_KEY("inode", K_INODE); break;
    case 'd': TR_KEY("device_id", K_DEVICE_ID); TR_KEY("device", K_DEVICE); break;
    case 's': TR_KEY("size", K_SIZE); TR_KEY("subtree", K_SUBTREE); break;
    case 'l':
        TR_KEY("links", K_LINKS); TR_KEY("linktarget", K_LINKTARGET);
        TR_KEY("linktarget_raw", K_LINKTARGET_RAW);
        break;
    case 'e': TR_KEY("extended_attributes", K_XATTRS); break;
    default: break;
    }
#undef TR_KEY
    return K_NONE;
}

__device__ bool parse_node(const TrArgs &a, Cur &c, const TrNodeOpen &r, TrNodeTmp *o) {
    if (!c.eat('{')) return false;
    c.ws();
    uint32_t seen = 0, type = 0;
    uint32_t c4 = r.c4_rank;  // the next ']' at depth 4 of this node
    bool symlink = false;
    for (bool more = true; more;) {
        if (!c.eat('"')) return false;
        const uint32_t k = parse_node_key(c);
        if (k == K_NONE || ((seen >> k) & 1u)) return false;
        seen |= 1u << k;
        c.ws();
        if (!c.eat(':')) return false;
        c.ws();
        bool ok;
        switch (k) {
        case K_NAME: case K_LINKTARGET: {
            const uint64_t quote = c.pos;
            const uint32_t str = parse_string(c);
            ok = str != 0u;
            if (ok && k == K_NAME) {
                o->name_pos = quote + 1;
                o->name_len = (uint32_t)(c.pos - quote - 2);
                if (str & kStrEsc) o->flags |= kTrNodeNameEsc;
            }
            break;
        }
        case K_TYPE:  // the index in NODE_TYPES
            ok = true;
            if (c.lit("\"file\"", 6)) type = kTrNodeFile;
            else if (c.lit("\"dir\"", 5)) type = kTrNodeDir | (1u << kTrNodeTypeShift);
            else if (c.lit("\"symlink\"", 9)) symlink = true, type = 2u << kTrNodeTypeShift;
            else if (c.lit("\"dev\"", 5)) type = 3u << kTrNodeTypeShift;
            else if (c.lit("\"chardev\"", 9)) type = 4u << kTrNodeTypeShift;
            else if (c.lit("\"fifo\"", 6)) type = 5u << kTrNodeTypeShift;
            else if (c.lit("\"socket\"", 8)) type = 6u << kTrNodeTypeShift;
            else ok = false;
            break;
        case K_MODE: case K_UID: case K_GID:
            ok = c.lit("null", 4) || parse_uint(c, 0xFFFFFFFFull);
            break;
        case K_MTIME: case K_ATIME: case K_CTIME: case K_USER: case K_GROUP: case K_LINKTARGET_RAW:
            ok = parse_null_or_string(c);
            break;
        case K_INODE: case K_DEVICE_ID: case K_SIZE: case K_LINKS: case K_DEVICE:
            ok = parse_uint(c, ~0ull);
            break;
        case K_CONTENT:
            ok = true;
            if (!c.lit("null", 4)) {
                uint32_t rank = 0;
                ok = skip_array(c, '"', a.c4, c4++, a.total.c4, r.blob, &rank) && rank >= r.id_rank;
                o->id0 = r.id_rank;
                o->nids = ok ? rank - r.id_rank : 0u;
                o->flags |= kTrNodeContent;
            }
            break;
        case K_SUBTREE:
            ok = true;
            if (!c.lit("null", 4)) {
                ok = parse_id(c, o->subtree);
                o->flags |= kTrNodeSubtree;
            }
            break;
        default:  // K_XATTRS
            ok = c.eat('[');
            c.ws();
            if (ok && !c.eat(']')) {
                for (;;) {
                    if (!parse_xattr(c)) return false;
                    c.ws();
                    if (c.eat(']')) break;
                    if (!c.eat(',')) return false;
                    c.ws();
                }
            }
            c4++;  // its ']' is one of the blob's at depth 4
            break;
        }
        if (!ok || !after_value(c, &more)) return false;
    }
    o->flags |= type;
    if ((seen & 3u) != 3u) return false;
    if (symlink && !((seen >> K_LINKTARGET) & 1u)) return false;
    // G_T leaves a dir without a subtree to the host; G_N records it
    if ((type & kTrNodeDir) && !(o->flags & kTrNodeSubtree) && !a.gn) return false;
    return after_element(c, '{');
}

// the root object and what surrounds it
__device__ bool parse_root(const TrArgs &a, Cur &c, uint32_t b) {
    const TrCounts fb = a.counts[a.tile_first[b]], fe = a.counts[a.tile_first[b + 1]];
    c.ws();
    if (!c.eat('{')) return false;
    c.ws();
    if (!c.lit("\"nodes\"", 7)) return false;
    c.ws();
    if (!c.eat(':')) return false;
    c.ws();
    if (!c.lit("null", 4)) {
        uint32_t rank = 0;
        if (!skip_array(c, '{', a.c2, fb.c2, fe.c2, b, &rank)) return false;
    }
    c.ws();
    if (!c.eat('}')) return false;
    c.ws();
    return c.pos == c.end;
}

}  // namespace

// ---- the structural pass ------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_tr_tile_sum_kernel(TrArgs a) {
    const uint32_t t = blockIdx.x * (kTrBlock / 64) + threadIdx.x / 64;
    if (t >= a.n_tiles) return;
    const uint32_t b = blob_of_tile(a, t);
    const uint64_t lo = a.refs[b].off, hi = lo + a.refs[b].len;
    bool too_long;
    uint32_t esc = tile_esc(a, lo, t - a.tile_first[b], &too_long);
    if (lane_id() == 0) {
        a.esc[t] = (uint8_t)esc;
        if (too_long) a.blob_bad[b] = 1u;
    }
    TrTileSum tile = {0, 0, 0u};
    for (uint32_t row = 0; row < kTrRows; row++) {
        const Chunk c = load_chunk(a, lo, hi, t - a.tile_first[b], row);
        uint32_t next;
        const uint32_t mine = lane_esc(c, esc, &next);
        TrTileSum total;
        (void)lane_state(TrTileIn{0u, 0}, chunk_sum(c, mine), &total);
        tile = compose(tile, total);
        esc = next;
    }
    if (lane_id() == 0) a.sums[t] = tile;
}

// one wave per blob: the state at the first byte of each of its tiles
__global__ __launch_bounds__(64) void rcdc_tr_tile_state_kernel(TrArgs a) {
    const uint32_t b = blockIdx.x;
    const uint32_t t0 = a.tile_first[b], t1 = a.tile_first[b + 1];
    TrTileIn carry = {0u, 0};
    for (uint32_t base = t0; base < t1; base += 64) {
        const uint32_t t = base + lane_id();
        TrTileSum mine = {0, 0, 0u};
        if (t < t1) mine = a.sums[t];
        TrTileSum total;
        const TrTileIn in = lane_state(carry, mine, &total);
        if (t < t1) a.ins[t] = in;
        carry = apply(carry, total);
    }
}

__global__ __launch_bounds__(256) void rcdc_tr_tile_count_kernel(TrArgs a) {
    const uint32_t t = blockIdx.x * (kTrBlock / 64) + threadIdx.x / 64;
    if (t >= a.n_tiles) return;
    const uint32_t b = blob_of_tile(a, t);
    const uint64_t lo = a.refs[b].off, hi = lo + a.refs[b].len;
    TrTileIn in = a.ins[t];
    uint32_t esc = a.esc[t];
    uint32_t sum[4] = {0, 0, 0, 0};
    for (uint32_t row = 0; row < kTrRows; row++) {
        const Chunk c = load_chunk(a, lo, hi, t - a.tile_first[b], row);
        uint32_t next;
        const uint32_t mine = lane_esc(c, esc, &next);
        TrTileSum total;
        const TrTileIn s = lane_state(in, chunk_sum(c, mine), &total);
        uint32_t n[4];
        chunk_counts(c, mine, s, n);
        for (int e = 0; e < 4; e++) sum[e] += n[e];
        in = apply(in, total);
        esc = next;
    }
    for (int e = 0; e < 4; e++) sum[e] = __shfl(wave_incl_add(sum[e]), 63, 64);
    if (lane_id() == 0) a.counts[t] = TrCounts{sum[0], sum[1], sum[2], sum[3]};
}

// One workgroup of 1024, a record of four uint32 per thread: the sum of the
// records of the threads before this one, and *all: of all 1024.
__device__ u32x4v block_excl4(u32x4v x, u32x4v *lds /* 16 */, u32x4v *all) {
    const uint32_t lane = lane_id(), wave = threadIdx.x / 64;
    u32x4v inc;
    inc.x = wave_incl_add(x.x);
    inc.y = wave_incl_add(x.y);
    inc.z = wave_incl_add(x.z);
    inc.w = wave_incl_add(x.w);
    __syncthreads();  // a call before this one has read lds
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    u32x4v before = {0u, 0u, 0u, 0u}, sum = {0u, 0u, 0u, 0u};
    for (uint32_t w = 0; w < 16; w++) {
        const u32x4v s = lds[w];
        if (w < wave) before += s;
        sum += s;
    }
    *all = sum;
    return before + inc - x;
}

// Exclusive scan of n records of four uint32 in place, the totals to v[n]:
// one workgroup of 1024, a chunk of 1024 records per pass.
__device__ void block_scan4(u32x4v *v, uint32_t n, u32x4v *lds /* 16 */) {
    u32x4v carry = {0u, 0u, 0u, 0u};
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        u32x4v x = {0u, 0u, 0u, 0u};
        if (i < n) x = v[i];
        u32x4v all;
        const u32x4v before = block_excl4(x, lds, &all);
        if (i < n) v[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) v[n] = carry;
}

__global__ __launch_bounds__(1024) void rcdc_tr_count_scan_kernel(TrArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.counts), a.n_tiles, lds);
}

__global__ __launch_bounds__(256) void rcdc_tr_tile_emit_kernel(TrArgs a) {
    const uint32_t t = blockIdx.x * (kTrBlock / 64) + threadIdx.x / 64;
    if (t >= a.n_tiles) return;
    const uint32_t b = blob_of_tile(a, t);
    const uint64_t lo = a.refs[b].off, hi = lo + a.refs[b].len;
    TrTileIn in = a.ins[t];
    uint32_t esc = a.esc[t];
    const TrCounts before = a.counts[t];
    uint32_t at[4] = {before.nodes, before.ids, before.c4, before.c2};  // before this row
    const uint32_t cap[4] = {a.total.nodes, a.total.ids, a.total.c4, a.total.c2};
    for (uint32_t row = 0; row < kTrRows; row++) {
        const Chunk c = load_chunk(a, lo, hi, t - a.tile_first[b], row);
        uint32_t next;
        uint32_t mine = lane_esc(c, esc, &next);
        TrTileSum total;
        TrTileIn s = lane_state(in, chunk_sum(c, mine), &total);
        uint32_t n[4], my[4];
        chunk_counts(c, mine, s, n);
        for (int e = 0; e < 4; e++) {
            const uint32_t inc = wave_incl_add(n[e]);
            my[e] = at[e] + inc - n[e];
            at[e] += __shfl(inc, 63, 64);
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (!((c.valid >> j) & 1u)) continue;
            const uint8_t ch = c.b[j];
            if (mine) {
                mine = 0u;
            } else if (ch == '\\') {
                mine = 1u;
            } else if (s.instr) {
                if (ch == '"') s.instr = 0u;
            } else {
                const int e = event_of(ch, s.depth);
                const uint64_t pos = c.pos + (uint64_t)j;
                if (e >= 0 && my[e] < cap[e]) {  // the counts of the pass before: always within
                    if (e == 0) a.node_open[my[0]] = TrNodeOpen{pos, b, my[1], my[2], 0u};
                    else if (e == 1) a.id_open[my[1]] = TrIdOpen{pos, b, 0u};
                    else if (e == 2) a.c4[my[2]] = TrClose{pos, b, my[1]};
                    else a.c2[my[3]] = TrClose{pos, b, my[0]};
                }
                if (e >= 0) my[e]++;
                if (ch == '"') s.instr = 1u;
                s.depth += bracket(ch);
            }
        }
        in = apply(in, total);
        esc = next;
    }
}

// ---- the strict lanes ------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_tr_id_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.ids) return;
    const TrIdOpen r = a.id_open[i];
    const rcdc_trparse_ref ref = a.refs[r.blob];
    Cur c = {a.text, r.pos, ref.off + ref.len};
    uint32_t id[8];
    if (!parse_id(c, id) || !after_element(c, '"')) {
        a.blob_bad[r.blob] = 1u;
        return;
    }
    u32x4v *d = reinterpret_cast<u32x4v *>(a.tmp_ids + (uint64_t)i * 32u);
    d[0] = u32x4v{id[0], id[1], id[2], id[3]};
    d[1] = u32x4v{id[4], id[5], id[6], id[7]};
}

__global__ __launch_bounds__(256) void rcdc_tr_node_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.nodes) return;
    const TrNodeOpen r = a.node_open[i];
    const rcdc_trparse_ref ref = a.refs[r.blob];
    Cur c = {a.text, r.pos, ref.off + ref.len};
    TrNodeTmp o = {};
    o.blob = r.blob;
    if (parse_node(a, c, r, &o)) {
        o.flags |= kTrNodeOk;
    } else {
        o.flags = 0u;
        o.nids = 0u;
        a.blob_bad[r.blob] = 1u;
    }
    a.tmp_nodes[i] = o;
}

// the blob lane; the id and node kernels have ended, so blob_bad is final and
// blob_ok becomes the blob's verdict
__global__ __launch_bounds__(256) void rcdc_tr_root_kernel(TrArgs a) {
    const uint32_t b = blockIdx.x * kTrBlock + threadIdx.x;
    if (b >= a.n_blobs) return;
    const rcdc_trparse_ref ref = a.refs[b];
    Cur c = {a.text, ref.off, ref.off + ref.len};
    a.blob_ok[b] = (parse_root(a, c, b) && !a.blob_bad[b]) ? 1u : 0u;
}

// ---- numbering ---------------------------------------------------------------------------

// What each node adds (content ids of a "file", a subtree, a node), scanned
// over the nodes in order, in three steps: a workgroup scans its kTrScan
// records and gives their sum, one workgroup scans the sums, and every record
// gets the sum of the workgroups before its own.
__global__ __launch_bounds__(1024) void rcdc_tr_number_kernel(TrArgs a) {
    __shared__ u32x4v lds[16];
    const uint32_t i = blockIdx.x * kTrScan + threadIdx.x;
    u32x4v x = {0u, 0u, 0u, 0u};
    if (i < a.total.nodes) {
        const TrNodeTmp *p = a.tmp_nodes + i;
        if ((p->flags & kTrNodeOk) && a.blob_ok[p->blob]) {
            x.x = (p->flags & kTrNodeFile) ? p->nids : 0u;
            x.y = (p->flags & kTrNodeSubtree) ? 1u : 0u;
            x.z = 1u;
        }
    }
    u32x4v all;
    const u32x4v before = block_excl4(x, lds, &all);
    if (i < a.total.nodes) reinterpret_cast<u32x4v *>(a.adds)[i] = before;
    if (threadIdx.x == 0) reinterpret_cast<u32x4v *>(a.add_sums)[blockIdx.x] = all;
}

__global__ __launch_bounds__(1024) void rcdc_tr_number_scan_kernel(TrArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.add_sums), (a.total.nodes + kTrScan - 1) / kTrScan, lds);
}

// also adds[n]: the totals
__global__ __launch_bounds__(1024) void rcdc_tr_number_apply_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrScan + threadIdx.x;
    u32x4v *adds = reinterpret_cast<u32x4v *>(a.adds);
    const u32x4v *sums = reinterpret_cast<const u32x4v *>(a.add_sums);
    if (i < a.total.nodes) adds[i] += sums[blockIdx.x];
    if (i == 0) adds[a.total.nodes] = sums[(a.total.nodes + kTrScan - 1) / kTrScan];
}

__global__ __launch_bounds__(256) void rcdc_tr_blob_kernel(TrArgs a) {
    const uint32_t b = blockIdx.x * kTrBlock + threadIdx.x;
    if (b >= a.n_blobs) return;
    const u32x4v *adds = reinterpret_cast<const u32x4v *>(a.adds);
    const u32x4v x0 = adds[a.counts[a.tile_first[b]].nodes];
    const u32x4v x1 = adds[a.counts[a.tile_first[b + 1]].nodes];
    rcdc_trparse_blob r = {};
    r.status = a.blob_ok[b] ? RCDC_TRPARSE_OK : RCDC_TRPARSE_NOT_PARSED;
    r.nodes = x1.z - x0.z;
    r.data_ids = x1.x - x0.x;
    r.tree_ids = x1.y - x0.y;
    r.data_start = x0.x;
    r.tree_start = x0.y;
    a.blobs[b] = r;
    if (a.node_start) a.node_start[b] = x0.z;
}

// rcdc_tree_nodes: one lane per node writes its record; the record's index is
// the count of nodes of OK blobs before it, which the numbering scanned
__global__ __launch_bounds__(256) void rcdc_tr_record_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.nodes) return;
    const TrNodeTmp *p = a.tmp_nodes + i;
    if (!(p->flags & kTrNodeOk) || !a.blob_ok[p->blob]) return;
    const u32x4v x = reinterpret_cast<const u32x4v *>(a.adds)[i];
    if (x.z >= a.cap_nodes) return;  // the bound: never
    uint32_t flags = 0;
    if (p->flags & kTrNodeContent) flags |= RCDC_TRNODE_CONTENT;
    if (p->flags & kTrNodeSubtree) flags |= RCDC_TRNODE_SUBTREE;
    if (p->flags & kTrNodeNameEsc) flags |= RCDC_TRNODE_NAME_ESC;
    const uint32_t type = (p->flags >> kTrNodeTypeShift) & 7u;
    u32x4v *d = reinterpret_cast<u32x4v *>(a.nodes + x.z);
    d[0] = u32x4v{(uint32_t)p->name_pos, (uint32_t)(p->name_pos >> 32), p->name_len, p->blob};
    d[1] = u32x4v{x.x, (p->flags & kTrNodeContent) ? p->nids : 0u, x.y, type | (flags << 8)};
}

__global__ __launch_bounds__(256) void rcdc_tr_subtree_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.nodes) return;
    const TrNodeTmp *p = a.tmp_nodes + i;
    if ((p->flags & (kTrNodeOk | kTrNodeSubtree)) != (kTrNodeOk | kTrNodeSubtree) ||
        !a.blob_ok[p->blob])
        return;
    const uint64_t dst = reinterpret_cast<const u32x4v *>(a.adds)[i].y;
    if (dst >= a.cap_tree_ids) return;  // the bound: never
    if (a.tree_ids) {
        u32x4v *d = reinterpret_cast<u32x4v *>(a.tree_ids + dst * 32u);
        d[0] = u32x4v{p->subtree[0], p->subtree[1], p->subtree[2], p->subtree[3]};
        d[1] = u32x4v{p->subtree[4], p->subtree[5], p->subtree[6], p->subtree[7]};
    }
    if (a.tree_is_dir) a.tree_is_dir[dst] = (p->flags & kTrNodeDir) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void rcdc_tr_scatter_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.ids) return;
    // the node of id i: the last node opened with id_rank <= i (nodes before
    // it with the same rank hold no id)
    uint32_t lo = 0, hi = a.total.nodes;
    if (hi == 0 || a.node_open[0].id_rank > i) return;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.node_open[mid].id_rank <= i) lo = mid; else hi = mid;
    }
    const TrNodeTmp *p = a.tmp_nodes + lo;
    if ((p->flags & (kTrNodeOk | kTrNodeFile)) != (kTrNodeOk | kTrNodeFile) ||
        i - p->id0 >= p->nids || !a.blob_ok[p->blob])
        return;
    const uint64_t dst = (uint64_t)reinterpret_cast<const u32x4v *>(a.adds)[lo].x + (i - p->id0);
    if (dst >= a.cap_data_ids) return;  // the bound: never
    const u32x4v *s = reinterpret_cast<const u32x4v *>(a.tmp_ids + (uint64_t)i * 32u);
    u32x4v *d = reinterpret_cast<u32x4v *>(a.data_ids + dst * 32u);
    d[0] = s[0];
    d[1] = s[1];
}

namespace rcdc {

static inline uint32_t tr_blocks(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

#define TR_LAUNCH(kernel, grid, block, ...)                                        \
    do {                                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);   \
        if (hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return e_;        \
    } while (0)

hipError_t launch_tr_structure(const TrArgs &a, hipStream_t st) {
    if (a.n_tiles) {
        TR_LAUNCH(rcdc_tr_tile_sum_kernel, tr_blocks(a.n_tiles, kTrBlock / 64), kTrBlock, a);
        TR_LAUNCH(rcdc_tr_tile_state_kernel, a.n_blobs, 64, a);
        TR_LAUNCH(rcdc_tr_tile_count_kernel, tr_blocks(a.n_tiles, kTrBlock / 64), kTrBlock, a);
    }
    TR_LAUNCH(rcdc_tr_count_scan_kernel, 1, 1024, a);
    return hipSuccess;
}

hipError_t launch_tr_parse(const TrArgs &a, hipStream_t st) {
    if (a.n_tiles)
        TR_LAUNCH(rcdc_tr_tile_emit_kernel, tr_blocks(a.n_tiles, kTrBlock / 64), kTrBlock, a);
    if (a.total.ids) TR_LAUNCH(rcdc_tr_id_kernel, tr_blocks(a.total.ids, kTrBlock), kTrBlock, a);
    if (a.total.nodes) TR_LAUNCH(rcdc_tr_node_kernel, tr_blocks(a.total.nodes, kTrBlock), kTrBlock, a);
    TR_LAUNCH(rcdc_tr_root_kernel, tr_blocks(a.n_blobs, kTrBlock), kTrBlock, a);
    const uint32_t scans = tr_blocks(a.total.nodes, kTrScan);
    if (scans) TR_LAUNCH(rcdc_tr_number_kernel, scans, kTrScan, a);
    TR_LAUNCH(rcdc_tr_number_scan_kernel, 1, 1024, a);
    TR_LAUNCH(rcdc_tr_number_apply_kernel, scans ? scans : 1u, kTrScan, a);
    TR_LAUNCH(rcdc_tr_blob_kernel, tr_blocks(a.n_blobs, kTrBlock), kTrBlock, a);
    if (a.total.nodes)
        TR_LAUNCH(rcdc_tr_subtree_kernel, tr_blocks(a.total.nodes, kTrBlock), kTrBlock, a);
    if (a.total.ids && a.data_ids)
        TR_LAUNCH(rcdc_tr_scatter_kernel, tr_blocks(a.total.ids, kTrBlock), kTrBlock, a);
    if (a.total.nodes && a.nodes)
        TR_LAUNCH(rcdc_tr_record_kernel, tr_blocks(a.total.nodes, kTrBlock), kTrBlock, a);
    return hipSuccess;
}

}  // namespace rcdc
