// rcdc_tree_parse (include/rcdc.h): tree blobs as JSON text in HBM -> the ids
// find_used_blobs and TreeStreamerOnce read out of them (commands/prune.rs:
// 1582-1632, blob/tree.rs:618-800).  gfx950, wave64.  The plan is
// rcdc_ixparse.hip's; what is new is that strings hold backslashes.
// rcdc_tree_nodes is the same kernels with TrArgs::gn set (the grammar G_N)
// and one more at the end, which writes a record per node.
//
// The structural pass is rcdc_json_tiles.h's with ESC true.  The four kinds
// of byte it records: '{' at depth 2 (a node), '"' opening a string at depth 4
// (an element of "content"), ']' at depth 4 (ends "content" or
// "extended_attributes"), ']' at depth 2 (ends "nodes").
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
// the same quotes and brackets as the structural pass.  Any lane that fails
// marks its blob, and a marked blob is NOT_PARSED: nothing of it is written.
//
// Numbering.  The node records (content ids of "file" nodes, subtrees, nodes;
// zero for a blob that is not OK) are scanned into positions, a workgroup per
// kTrScan records and one workgroup over their sums; one lane per blob writes
// its record from the scan at its first and last node, one lane per node
// copies its subtree, one lane per id its id.

#include "rcdc_trparse.h"

namespace {

using namespace rcdc;
using namespace rcdc::jt;

static_assert(kTrBlock == kTileBlock, "the structural kernels run kTileBlock threads");

__device__ __forceinline__ Tiles<rcdc_trparse_ref> tiles(const TrArgs &a) {
    return {a.text, a.text_len, a.refs, a.tile_first, a.n_blobs, a.n_tiles,
            kTrTile, a.sums,    a.ins,  a.counts,     a.esc,     a.blob_bad};
}

// ---- strict parsers ----------------------------------------------------------

// an integer of G_T of at most `max`: only that it is one
__device__ __forceinline__ bool parse_uint_to(Cur &c, uint64_t max) {
    uint64_t v;
    return parse_uint(c, max, &v);
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
    uint32_t c4 = r.rank_b;  // the next ']' at depth 4 of this node
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
            ok = c.lit("null", 4) || parse_uint_to(c, 0xFFFFFFFFull);
            break;
        case K_MTIME: case K_ATIME: case K_CTIME: case K_USER: case K_GROUP: case K_LINKTARGET_RAW:
            ok = parse_null_or_string(c);
            break;
        case K_INODE: case K_DEVICE_ID: case K_SIZE: case K_LINKS: case K_DEVICE:
            ok = parse_uint_to(c, ~0ull);
            break;
        case K_CONTENT:
            ok = true;
            if (!c.lit("null", 4)) {
                uint32_t rank = 0;
                ok = skip_array(c, '"', a.c4, c4++, a.total.n[kTrC4], r.ref, &rank) &&
                     rank >= r.rank_a;
                o->id0 = r.rank_a;
                o->nids = ok ? rank - r.rank_a : 0u;
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
        if (!skip_array(c, '{', a.c2, fb.n[kTrC2], fe.n[kTrC2], b, &rank)) return false;
    }
    c.ws();
    if (!c.eat('}')) return false;
    c.ws();
    return c.pos == c.end;
}

}  // namespace

// ---- the structural pass ------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_tr_tile_sum_kernel(TrArgs a) {
    tile_sum<true, TrGrammar>(tiles(a));
}

__global__ __launch_bounds__(64) void rcdc_tr_tile_state_kernel(TrArgs a) { tile_state(tiles(a)); }

__global__ __launch_bounds__(256) void rcdc_tr_tile_count_kernel(TrArgs a) {
    tile_count<true, TrGrammar>(tiles(a));
}

__global__ __launch_bounds__(1024) void rcdc_tr_count_scan_kernel(TrArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.counts), a.n_tiles, lds);
}

__global__ __launch_bounds__(256) void rcdc_tr_tile_emit_kernel(TrArgs a) {
    tile_emit<true, TrGrammar>(tiles(a), a.total,
                               [&](int e, uint64_t pos, uint32_t b, const uint32_t *my) {
        if (e == kTrNode) a.node_open[my[kTrNode]] = TrNodeOpen{pos, b, my[kTrId], my[kTrC4], 0u};
        else if (e == kTrId) a.id_open[my[kTrId]] = TrIdOpen{pos, b, 0u};
        else if (e == kTrC4) a.c4[my[kTrC4]] = TrClose{pos, b, my[kTrId]};
        else a.c2[my[kTrC2]] = TrClose{pos, b, my[kTrNode]};
    });
}

// ---- the strict lanes ------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_tr_id_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.n[kTrId]) return;
    const TrIdOpen r = a.id_open[i];
    const rcdc_trparse_ref ref = a.refs[r.ref];
    Cur c = {a.text, r.pos, ref.off + ref.len};
    uint32_t id[8];
    if (!parse_id(c, id) || !after_element(c, '"')) {
        a.blob_bad[r.ref] = 1u;
        return;
    }
    u32x4v *d = reinterpret_cast<u32x4v *>(a.tmp_ids + (uint64_t)i * 32u);
    d[0] = u32x4v{id[0], id[1], id[2], id[3]};
    d[1] = u32x4v{id[4], id[5], id[6], id[7]};
}

__global__ __launch_bounds__(256) void rcdc_tr_node_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrBlock + threadIdx.x;
    if (i >= a.total.n[kTrNode]) return;
    const TrNodeOpen r = a.node_open[i];
    const rcdc_trparse_ref ref = a.refs[r.ref];
    Cur c = {a.text, r.pos, ref.off + ref.len};
    TrNodeTmp o = {};
    o.blob = r.ref;
    if (parse_node(a, c, r, &o)) {
        o.flags |= kTrNodeOk;
    } else {
        o.flags = 0u;
        o.nids = 0u;
        a.blob_bad[r.ref] = 1u;
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
    if (i < a.total.n[kTrNode]) {
        const TrNodeTmp *p = a.tmp_nodes + i;
        if ((p->flags & kTrNodeOk) && a.blob_ok[p->blob]) {
            x.x = (p->flags & kTrNodeFile) ? p->nids : 0u;
            x.y = (p->flags & kTrNodeSubtree) ? 1u : 0u;
            x.z = 1u;
        }
    }
    u32x4v all;
    const u32x4v before = block_excl4(x, lds, &all);
    if (i < a.total.n[kTrNode]) reinterpret_cast<u32x4v *>(a.adds)[i] = before;
    if (threadIdx.x == 0) reinterpret_cast<u32x4v *>(a.add_sums)[blockIdx.x] = all;
}

__global__ __launch_bounds__(1024) void rcdc_tr_number_scan_kernel(TrArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.add_sums), (a.total.n[kTrNode] + kTrScan - 1) / kTrScan,
                lds);
}

// also adds[n]: the totals
__global__ __launch_bounds__(1024) void rcdc_tr_number_apply_kernel(TrArgs a) {
    const uint32_t i = blockIdx.x * kTrScan + threadIdx.x;
    u32x4v *adds = reinterpret_cast<u32x4v *>(a.adds);
    const u32x4v *sums = reinterpret_cast<const u32x4v *>(a.add_sums);
    if (i < a.total.n[kTrNode]) adds[i] += sums[blockIdx.x];
    if (i == 0) adds[a.total.n[kTrNode]] = sums[(a.total.n[kTrNode] + kTrScan - 1) / kTrScan];
}

__global__ __launch_bounds__(256) void rcdc_tr_blob_kernel(TrArgs a) {
    const uint32_t b = blockIdx.x * kTrBlock + threadIdx.x;
    if (b >= a.n_blobs) return;
    const u32x4v *adds = reinterpret_cast<const u32x4v *>(a.adds);
    const u32x4v x0 = adds[a.counts[a.tile_first[b]].n[kTrNode]];
    const u32x4v x1 = adds[a.counts[a.tile_first[b + 1]].n[kTrNode]];
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
    if (i >= a.total.n[kTrNode]) return;
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
    if (i >= a.total.n[kTrNode]) return;
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
    if (i >= a.total.n[kTrId]) return;
    // the node of id i: the last node opened with id_rank <= i (nodes before
    // it with the same rank hold no id)
    uint32_t lo = 0, hi = a.total.n[kTrNode];
    if (hi == 0 || a.node_open[0].rank_a > i) return;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.node_open[mid].rank_a <= i) lo = mid; else hi = mid;
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

hipError_t launch_tr_structure(const TrArgs &a, hipStream_t st) {
    if (a.n_tiles) {
        RCDC_LAUNCH(rcdc_tr_tile_sum_kernel, blocks(a.n_tiles, kTrBlock / 64), kTrBlock, a);
        RCDC_LAUNCH(rcdc_tr_tile_state_kernel, a.n_blobs, 64, a);
        RCDC_LAUNCH(rcdc_tr_tile_count_kernel, blocks(a.n_tiles, kTrBlock / 64), kTrBlock, a);
    }
    RCDC_LAUNCH(rcdc_tr_count_scan_kernel, 1, 1024, a);
    return hipSuccess;
}

hipError_t launch_tr_parse(const TrArgs &a, hipStream_t st) {
    const uint32_t n_ids = a.total.n[kTrId], n_nodes = a.total.n[kTrNode];
    if (a.n_tiles)
        RCDC_LAUNCH(rcdc_tr_tile_emit_kernel, blocks(a.n_tiles, kTrBlock / 64), kTrBlock, a);
    if (n_ids) RCDC_LAUNCH(rcdc_tr_id_kernel, blocks(n_ids, kTrBlock), kTrBlock, a);
    if (n_nodes) RCDC_LAUNCH(rcdc_tr_node_kernel, blocks(n_nodes, kTrBlock), kTrBlock, a);
    RCDC_LAUNCH(rcdc_tr_root_kernel, blocks(a.n_blobs, kTrBlock), kTrBlock, a);
    const uint32_t scans = blocks(n_nodes, kTrScan);
    if (scans) RCDC_LAUNCH(rcdc_tr_number_kernel, scans, kTrScan, a);
    RCDC_LAUNCH(rcdc_tr_number_scan_kernel, 1, 1024, a);
    RCDC_LAUNCH(rcdc_tr_number_apply_kernel, scans ? scans : 1u, kTrScan, a);
    RCDC_LAUNCH(rcdc_tr_blob_kernel, blocks(a.n_blobs, kTrBlock), kTrBlock, a);
    if (n_nodes)
        RCDC_LAUNCH(rcdc_tr_subtree_kernel, blocks(n_nodes, kTrBlock), kTrBlock, a);
    if (n_ids && a.data_ids)
        RCDC_LAUNCH(rcdc_tr_scatter_kernel, blocks(n_ids, kTrBlock), kTrBlock, a);
    if (n_nodes && a.nodes)
        RCDC_LAUNCH(rcdc_tr_record_kernel, blocks(n_nodes, kTrBlock), kTrBlock, a);
    return hipSuccess;
}

}  // namespace rcdc
