// rcdc_pack_header_parse (include/rcdc.h): opened pack headers in HBM -> the
// entries PackHeader::from_binary reads out of them (packfile.rs:88-242), in
// the arrays of rcdc_index_parse.  gfx950, wave64.  The plan is
// rcdc_trparse.hip's, "a tile as a function of the state at its first byte".
//
// The chain.  Entries follow each other and each is 37 or 41 bytes by its
// type byte, so where an entry starts depends on every entry before it: the
// only serial thing in the format.  A tile (kPhTile bytes, one wave) needs of
// all that came before one number, its PHASE: the distance from its first
// byte to the first entry start at or after it, 0..40.
//
// Pass 1.  One lane per (tile, phase) walks the entries that start in the
// tile from that phase -- at most ceil(kPhTile / 37) = 56 -- out of LDS,
// where the wave has staged the tile and a halo of 48 bytes (an entry that
// starts in the tile's last byte ends 40 bytes behind it) with 16-byte loads.
// It leaves a PhWalk: the exit phase, the entries started, the sum of their
// lengths in 64 bits, how many are tree entries, and the first type byte
// above 3 or entry cut short it met.  40 of the 41 walks of a tile are off
// the true chain: they read ids as type bytes and mostly end in "bad type"
// at once.  Nothing of them is used.  A header's first tile has a known
// phase, so one lane walks it.
//
// LDS.  The 41 walkers start on consecutive bytes and advance by 37 or 41, so
// at any step they stand within 40 + 4 * (entries walked) bytes of each other:
// while that is under 128 bytes they read distinct banks or the same dword
// (a broadcast), later some pairs meet on a bank, 2-way at worst.  The loads
// are single bytes (an entry is at no alignment), 4 waves of 2096 bytes per
// workgroup: LDS does not bound the occupancy.
//
// Chaining.  One wave per header, 64 tiles at a time: the wave stages the
// exit phases of those tiles (41 bytes each) in LDS, lane 0 follows the true
// chain through them (one LDS lookup per TILE, never per entry), then lane l
// reads tile l's PhWalk at its phase and three wave scans give every tile the
// entries and the offset before it (PhTileIn).  The first error on the chain
// in header order is the header's status; the tiles behind it are not looked
// at.  Without one, a sum of lengths above 2^32 - 1 is OVERFLOW: offsets only
// grow, so the running offset exceeds that after some entry exactly when the
// last one does.
//
// Numbering.  What each header adds (a pack and its entries, under the type
// of its first entry; nothing unless OK) is scanned over the headers as in
// rcdc_trparse.hip: a workgroup per kPhScan headers, one workgroup over their
// sums, and the sums added back.
//
// Pass 2.  A tile of an OK header is staged again; lane 0 re-walks it from
// its now known phase and leaves the entry starts in LDS; then lane e takes
// entry e: a wave scan of the lengths gives its offset, and the wave writes
// the locs 16 bytes per lane and the ids 16 bytes per lane (two lanes per id),
// both to consecutive addresses.

#include "rcdc_pkhdr.h"
#include "rcdc_wave.h"

namespace {

using namespace rcdc;

// The header of tile t (uniform over the wave): the last h with tile_first[h] <= t.
__device__ __forceinline__ uint32_t header_of_tile(const PhArgs &a, uint32_t t) {
    uint32_t lo = 0, hi = a.n_headers;  // tile_first[lo] <= t < tile_first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// Arena offset of the first byte of tile k of the header that starts at lo:
// tiles count from the 16-byte boundary at or before the header's first byte,
// so for the arena's first header it may lie up to 15 bytes below 0.
__device__ __forceinline__ int64_t tile_start(const PhArgs &a, uint64_t lo, uint32_t k) {
    const uint64_t mis = (uint64_t)(uintptr_t)a.plain & 15u;
    return (int64_t)(((lo + mis) & ~15ull) + (uint64_t)k * kPhTile) - (int64_t)mis;
}

// The wave stages the kPhTile + kPhHalo bytes from arena offset s0 into lds
// (16-byte aligned): a chunk that lies wholly in the arena is one dword x4
// load, the arena's ragged first and last chunk go byte by byte, and bytes
// outside the arena read as 0.
__device__ __forceinline__ void stage_tile(const PhArgs &a, int64_t s0, uint8_t *lds) {
    for (uint32_t c = lane_id(); c < (kPhTile + kPhHalo) / 16; c += 64) {
        const int64_t s = s0 + (int64_t)c * 16;
        u32x4v w = {0u, 0u, 0u, 0u};
        if (s >= 0 && (uint64_t)s + 16u <= a.plain_len) {
            w = *reinterpret_cast<const u32x4v *>(a.plain + s);
        } else {
            uint32_t ws[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < 16; j++)
                if (s + j >= 0 && (uint64_t)(s + j) < a.plain_len)
                    ws[j >> 2] |= (uint32_t)a.plain[s + j] << ((j & 3) * 8);
            w = u32x4v{ws[0], ws[1], ws[2], ws[3]};
        }
        *reinterpret_cast<u32x4v *>(lds + c * 16u) = w;
    }
}

__device__ __forceinline__ uint32_t lds_u32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ uint32_t pack_walk(uint32_t exit, uint32_t n, uint32_t tree, uint32_t err,
                                              uint32_t pos) {
    return exit | (n << 6) | (tree << 12) | (err << 18) | (pos << 20);
}
__device__ __forceinline__ uint32_t walk_exit(uint32_t p) { return p & 63u; }
__device__ __forceinline__ uint32_t walk_n(uint32_t p) { return (p >> 6) & 63u; }
__device__ __forceinline__ uint32_t walk_tree(uint32_t p) { return (p >> 12) & 63u; }
__device__ __forceinline__ uint32_t walk_err(uint32_t p) { return (p >> 18) & 3u; }
__device__ __forceinline__ uint32_t walk_pos(uint32_t p) { return (p >> 20) & 2047u; }

}  // namespace

// ---- pass 1 -------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ph_walk_kernel(PhArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_all[kPhBlock / 64][kPhTile + kPhHalo];
    const uint32_t t = blockIdx.x * (kPhBlock / 64) + threadIdx.x / 64;
    const bool live = t < a.n_tiles;
    uint8_t *lds = lds_all[threadIdx.x / 64];
    uint32_t h = 0, k = 0;
    uint64_t lo = 0, hi = 0;
    int64_t s0 = 0;
    if (live) {
        h = header_of_tile(a, t);
        k = t - a.tile_first[h];
        lo = a.refs[h].off;
        hi = lo + a.refs[h].len;
        s0 = tile_start(a, lo, k);
        stage_tile(a, s0, lds);
    }
    __syncthreads();
    if (!live) return;
    const uint32_t d = lane_id();
    if (d >= kPhPhases) return;
    if (k == 0 && d != (uint32_t)((int64_t)lo - s0)) return;  // the first tile's phase is known
    // the header's end in tile positions: above 0 (the tile holds a byte of it)
    const int64_t end = (int64_t)hi - s0;
    const uint32_t stop = end < (int64_t)kPhTile ? (uint32_t)end : kPhTile;
    uint32_t p = d, n = 0, tree = 0, err = 0, pos = 0;
    uint64_t sum = 0;
    while (p < stop) {
        const uint32_t type = lds[p];
        if (type > 3u) {
            err = RCDC_PKHDR_BAD_TYPE;
            pos = p;
            break;
        }
        const uint32_t size = type >= 2u ? 41u : 37u;
        if ((int64_t)(p + size) > end) {
            err = RCDC_PKHDR_CUT_SHORT;
            pos = p;
            break;
        }
        sum += lds_u32(lds + p + 1);
        tree += type & 1u;
        n++;
        p += size;
    }
    const uint32_t exit = (err || p < kPhTile) ? 0u : p - kPhTile;  // at most 40
    const uint64_t at = (uint64_t)t * kPhPhases + d;
    a.walks[at] = PhWalk{sum, pack_walk(exit, n, tree, err, pos), 0u};
    a.exits[at] = (uint8_t)exit;
}

// ---- chaining ---------------------------------------------------------------------------

// one wave per header
__global__ __launch_bounds__(64) void rcdc_ph_chain_kernel(PhArgs a) {
    __shared__ uint8_t ex[64 * kPhPhases];
    __shared__ uint8_t ph[64 + 1];
    const uint32_t h = blockIdx.x, lane = lane_id();
    const uint32_t t0 = a.tile_first[h], t1 = a.tile_first[h + 1];
    const uint64_t lo = a.refs[h].off, len = a.refs[h].len;
    uint32_t phase = (uint32_t)((int64_t)lo - tile_start(a, lo, 0));
    uint32_t count = 0, tree = 0, status = RCDC_PKHDR_OK, err_entry = 0;
    uint64_t sum = 0, err_pos = 0;
    for (uint32_t base = t0; base < t1 && status == RCDC_PKHDR_OK; base += 64) {
        const uint32_t cnt = t1 - base < 64u ? t1 - base : 64u;
        __syncthreads();  // the round before has read ex and ph
        for (uint32_t i = lane; i < cnt * kPhPhases; i += 64)
            ex[i] = a.exits[(uint64_t)base * kPhPhases + i];
        __syncthreads();
        if (lane == 0) {
            // a header's first tile has one walk, at its phase: what the other
            // bytes of ex hold is never looked up
            uint32_t q = phase;
            for (uint32_t i = 0; i < cnt; i++) {
                ph[i] = (uint8_t)q;
                q = ex[i * kPhPhases + q];
                if (q >= kPhPhases) q = 0;  // behind an error on the chain: not used
            }
            ph[cnt] = (uint8_t)q;
        }
        __syncthreads();
        uint32_t mine = 0, packed = 0;
        uint64_t s = 0;
        if (lane < cnt) {
            mine = ph[lane];
            const PhWalk w = a.walks[(uint64_t)(base + lane) * kPhPhases + mine];
            packed = w.packed;
            s = w.sum;
        }
        phase = ph[cnt];
        const uint64_t bad = __ballot(lane < cnt && walk_err(packed) != 0u);
        const uint32_t first = bad ? (uint32_t)__builtin_ctzll(bad) : 64u;
        // tiles behind the first error add nothing
        const uint32_t n = lane <= first ? walk_n(packed) : 0u;
        const uint32_t tr = lane <= first ? walk_tree(packed) : 0u;
        if (lane > first) s = 0;
        const uint32_t n_inc = wave_incl_add(n), tr_inc = wave_incl_add(tr);
        const uint64_t s_inc = wave_incl_add64(s);
        if (lane < cnt && lane <= first)
            a.ins[base + lane] = PhTileIn{mine, count + n_inc - n, sum + s_inc - s};
        if (bad) {
            status = walk_err(__shfl(packed, first, 64));
            err_entry = count + __shfl(n_inc, first, 64);
            const uint32_t k = base - t0 + first;
            err_pos = (uint64_t)(tile_start(a, lo, k) + (int64_t)walk_pos(__shfl(packed, first, 64)) -
                                 (int64_t)lo);
        }
        count += __shfl(n_inc, 63, 64);
        tree += __shfl(tr_inc, 63, 64);
        sum += shfl64(s_inc, 63);
    }
    if (lane != 0) return;
    if (status == RCDC_PKHDR_OK && sum > 0xFFFFFFFFull) status = RCDC_PKHDR_OVERFLOW;
    PhHeaderTmp o = {};
    o.status = status;
    o.err_entry = err_entry;
    o.err_pos = err_pos;
    if (status == RCDC_PKHDR_OK) {
        o.sum = sum;
        o.count = count;
        o.tree = tree;
        o.type = len ? (uint32_t)a.plain[lo] & 1u : 0u;
    }
    a.tmp[h] = o;
}

// ---- numbering ---------------------------------------------------------------------------

__global__ __launch_bounds__(1024) void rcdc_ph_number_kernel(PhArgs a) {
    __shared__ u32x4v lds[16];
    const uint32_t i = blockIdx.x * kPhScan + threadIdx.x;
    u32x4v x = {0u, 0u, 0u, 0u};
    if (i < a.n_headers) {
        const PhHeaderTmp *p = a.tmp + i;
        if (p->status == RCDC_PKHDR_OK) {
            if (p->type) {
                x.y = 1u;
                x.w = p->count;
            } else {
                x.x = 1u;
                x.z = p->count;
            }
        }
    }
    u32x4v all;
    const u32x4v before = block_excl4(x, lds, &all);
    if (i < a.n_headers) reinterpret_cast<u32x4v *>(a.adds)[i] = before;
    if (threadIdx.x == 0) reinterpret_cast<u32x4v *>(a.add_sums)[blockIdx.x] = all;
}

// exclusive scan of the workgroups' sums in place, the totals behind them
__global__ __launch_bounds__(1024) void rcdc_ph_number_scan_kernel(PhArgs a) {
    __shared__ u32x4v lds[16];
    block_scan4(reinterpret_cast<u32x4v *>(a.add_sums), (a.n_headers + kPhScan - 1) / kPhScan, lds);
}

// the sums added back, adds[n_headers] (the totals), and the headers' records
__global__ __launch_bounds__(1024) void rcdc_ph_number_apply_kernel(PhArgs a) {
    const uint32_t i = blockIdx.x * kPhScan + threadIdx.x;
    u32x4v *adds = reinterpret_cast<u32x4v *>(a.adds);
    const u32x4v *sums = reinterpret_cast<const u32x4v *>(a.add_sums);
    if (i == 0) adds[a.n_headers] = sums[(a.n_headers + kPhScan - 1) / kPhScan];
    if (i >= a.n_headers) return;
    const u32x4v before = adds[i] + sums[blockIdx.x];
    adds[i] = before;
    const PhHeaderTmp *p = a.tmp + i;
    rcdc_pkhdr_header r = {};
    r.status = p->status;
    r.err_entry = p->err_entry;
    r.err_pos = p->err_pos;
    if (p->status == RCDC_PKHDR_OK) {
        const uint64_t len = a.refs[i].len;  // the entries' bytes
        r.type = p->type;
        r.number = a.pack_base[p->type] + (p->type ? before.y : before.x);
        r.count = p->count;
        r.first = p->type ? before.w : before.z;
        r.data = p->count - p->tree;
        r.tree = p->tree;
        r.size = 32u + len;
        r.pack_size = 36u + p->sum + len;
    }
    a.headers[i] = r;
}

// ---- pass 2 -------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rcdc_ph_emit_kernel(PhArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_all[kPhBlock / 64][kPhTile + kPhHalo];
    __shared__ uint16_t starts_all[kPhBlock / 64][64];
    const uint32_t wave = threadIdx.x / 64, lane = lane_id();
    const uint32_t t = blockIdx.x * (kPhBlock / 64) + wave;
    uint8_t *lds = lds_all[wave];
    uint16_t *starts = starts_all[wave];
    bool live = t < a.n_tiles;
    uint32_t h = 0, n = 0;
    PhTileIn in = {};
    if (live) {
        h = header_of_tile(a, t);
        live = a.tmp[h].status == RCDC_PKHDR_OK;
    }
    if (live) {
        in = a.ins[t];
        const uint32_t k = t - a.tile_first[h];
        n = walk_n(a.walks[(uint64_t)t * kPhPhases + in.phase].packed);
        stage_tile(a, tile_start(a, a.refs[h].off, k), lds);
    }
    __syncthreads();
    if (live && lane == 0) {
        // the entries are whole and their types known good: pass 1 walked them
        uint32_t p = in.phase;
        for (uint32_t e = 0; e < n; e++) {
            starts[e] = (uint16_t)p;
            p += lds[p] >= 2u ? 41u : 37u;
        }
    }
    __syncthreads();
    if (!live || n == 0) return;
    const uint32_t type = a.tmp[h].type;
    const u32x4v before = reinterpret_cast<const u32x4v *>(a.adds)[h];
    const uint32_t number = a.pack_base[type] + (type ? before.y : before.x);
    const uint64_t dst0 = (uint64_t)(type ? before.w : before.z) + in.entry;
    if (dst0 + n > a.cap_entries) return;  // the bound: never
    uint32_t length = 0, ulen = 0;
    if (lane < n) {
        const uint8_t *e = lds + starts[lane];
        length = lds_u32(e + 1);
        if (e[0] >= 2u) ulen = lds_u32(e + 5);
    }
    // an OK header: every offset is below 2^32
    const uint32_t offset = (uint32_t)in.offset + wave_incl_add(length) - length;
    if (a.locs[type] && lane < n)
        *reinterpret_cast<u32x4v *>(a.locs[type] + dst0 + lane) = u32x4v{number, offset, length, ulen};
    if (a.ids[type]) {
        for (uint32_t c = lane; c < 2u * n; c += 64) {
            const uint32_t p = starts[c >> 1];
            const uint8_t *s = lds + p + (lds[p] >= 2u ? 9u : 5u) + (c & 1u) * 16u;
            const u32x4v w = {lds_u32(s), lds_u32(s + 4), lds_u32(s + 8), lds_u32(s + 12)};
            *reinterpret_cast<u32x4v *>(a.ids[type] + dst0 * 32u + (uint64_t)c * 16u) = w;
        }
    }
}

namespace rcdc {

hipError_t launch_ph_parse(const PhArgs &a, hipStream_t st) {
    if (a.n_tiles)
        RCDC_LAUNCH(rcdc_ph_walk_kernel, blocks(a.n_tiles, kPhBlock / 64), kPhBlock, a);
    RCDC_LAUNCH(rcdc_ph_chain_kernel, a.n_headers, 64, a);
    const uint32_t scans = blocks(a.n_headers, kPhScan);
    RCDC_LAUNCH(rcdc_ph_number_kernel, scans, kPhScan, a);
    RCDC_LAUNCH(rcdc_ph_number_scan_kernel, 1, 1024, a);
    RCDC_LAUNCH(rcdc_ph_number_apply_kernel, scans, kPhScan, a);
    if (a.n_tiles)
        RCDC_LAUNCH(rcdc_ph_emit_kernel, blocks(a.n_tiles, kPhBlock / 64), kPhBlock, a);
    return hipSuccess;
}

}  // namespace rcdc
