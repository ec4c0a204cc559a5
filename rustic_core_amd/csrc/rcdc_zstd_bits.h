// rcdc_zstd_bits.h -- the device-side zstd decoder helpers (RFC 8878) that the
// frame checker (rcdc_zstd_dec.hip) and the decompressor (rcdc_zstd_dx.hip)
// share, in one copy: the predefined tables and length baselines, the FSE and
// Huffman table entries and the per-wave LDS layout, the loads at any
// alignment, both backward bit readers, the table readers and builders, the
// Huffman stream decoder, the section parsers (literals-section header,
// sequence count, the Huffman literals step, the sequence-table step), the
// frame-header parse and XXH64.
//
// Everything is in an anonymous namespace: each translation unit compiles its
// own instance with the callers it has, so whether a function that is not
// __forceinline__ gets inlined is decided per unit, as before.  The text is
// hardened against corrupt input (indices masked or clamped, positions
// checked) so that a frame's bytes never decide whether a table access stays
// inside its table; build_huf and huf_stream take their extra checks as a
// template parameter, which the checker turns off for speed (DESIGN.md
// 3g-bis).  The section steps are plain __device__ functions on purpose:
// forced inlining cost the checker a third of its raw-block rate.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t kBlockMax = 128u << 10;

// Predefined distributions (RFC 8878 3.1.1.3.2.2) and code -> (baseline,
// extra bits) of literal and match lengths (3.1.1.3.2.1.1).
__constant__ int16_t kLLNorm[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                    2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ int16_t kMLNorm[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ int16_t kOFNorm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
__constant__ uint32_t kLLBase[36] = {0,  1,  2,  3,  4,  5,   6,   7,   8,    9,    10,   11,
                                     12, 13, 14, 15, 16, 18,  20,  22,  24,   28,   32,   40,
                                     48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
__constant__ uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,  1,  1,
                                    1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__constant__ uint32_t kMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,
                                     17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30,
                                     31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83,
                                     99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
__constant__ uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1,
                                    2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

struct FseD {  // FSE decoding entry (FSE_decode_t)
    uint8_t sym, nb;
    uint16_t next;
};
struct HufD {
    uint8_t sym, nb;
};

// LDS of one wave (workgroup = one wave).  The Huffman tables live only
// through a block's literals section (the checker decodes its literals to
// scratch memory, the decompressor to the block's slot of the workspace) and
// the LL / ML extras only through its sequences section, so the two share
// bytes: 9984 B per wave, 16 waves per CU by LDS (14464 B and 11 waves
// before).  A treeless literals section rebuilds the Huffman table from the
// weights kept in w.
struct ZstdLds {
    FseD ll[512], ml[512], of[256];
    union {
        struct {
            FseD hw[64];  // FSE table of Huffman weights (log <= 6)
            HufD huf[2048];
        } h;
        // per LL / ML state: the code's baseline | extra bits << 24 (as
        // zstd's ZSTD_seqSymbol), so a sequence's lengths need one LDS read
        // each and no dependent constant-table lookup
        struct {
            uint32_t llx[512], mlx[512];
        } x;
    } u;
    int16_t norm[64];  // (read_ncount's capacity: kNormCap)
    uint16_t nxt[64];  // per symbol: <= 53 (ML), <= 64 by kNormCap
    uint8_t w[256];    // Huffman weights (kept for treeless literals)
    uint32_t pf[8];    // the sequence reader's next group, loaded straight to LDS
};
constexpr uint32_t kNormCap = 64;

__device__ __forceinline__ uint32_t highbit32(uint32_t v) { return 31u - (uint32_t)__clz(v); }

__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
}

// Frames, blobs, the literal scratch and the workspace are global memory:
// loads through a global-address-space pointer are global_load (counted by
// vmcnt only).  A generic pointer gives flat_load, which also counts in
// lgkmcnt, so every LDS wait of the sequence loop (its table reads) also
// waited for the bitstream's prefetch loads in flight (r5zpmc ISA: 24 flat
// loads in the decode loop).
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T *gptr(const T *p) {
    return (const __attribute__((address_space(1))) T *)p;
}

// 4 bytes at any alignment from the aligned dwords that hold them (a dword
// holding a readable byte is readable: allocations are 4-byte granular).
__device__ __forceinline__ uint32_t ld4u(const uint8_t *p) {
    const uint32_t b = (uint32_t)(uintptr_t)p & 3u;
    const auto *w = gptr((const uint32_t *)(p - b));
    const uint32_t lo = w[0];
    const uint32_t hi = w[b ? 1 : 0];
    return __builtin_amdgcn_alignbit(hi, lo, b * 8u);
}
__device__ __forceinline__ uint64_t ld8u(const uint8_t *p) {
    return (uint64_t)ld4u(p) | (uint64_t)ld4u(p + 4) << 32;
}

// 8 little-endian bytes at p; bytes outside [lo, hi) read as 0.
__device__ uint64_t ld8b(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
    if (p >= lo && p + 8 <= hi) return ld8u(p);
    uint64_t v = 0;
    for (int i = 0; i < 8; i++)
        if (p + i >= lo && p + i < hi) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

// ---- backward bitstreams (RFC 8878 4.1) ---------------------------------------
// Bits [0, pos) unread, read from the top; bits below 0 read as zeros (a read
// that goes below 0 is an overflow).
struct BRev {
    const uint8_t *base;
    int64_t len;
    int64_t pos;
    int64_t cb;  // cache holds bits [cb, cb + 64)
    uint64_t cache;
};

__device__ __forceinline__ void brev_fill(BRev &r) {
    r.cb = ((r.pos - 57) >> 3) << 3;  // arithmetic shift: floor
    r.cache = ld8b(r.base + (r.cb >> 3), r.base, r.base + r.len);
}

// false: empty stream or no end mark
__device__ bool brev_init(BRev &r, const uint8_t *p, int64_t len) {
    r.base = p;
    r.len = len;
    if (len <= 0) return false;
    const uint32_t last = p[len - 1];
    if (last == 0) return false;
    r.pos = 8 * (len - 1) + (int64_t)highbit32(last);
    brev_fill(r);
    return true;
}

__device__ __forceinline__ uint64_t brev_bits(BRev &r, uint32_t n) {
    uint64_t v = 0;
    if (n) {
        const int64_t lo = r.pos - (int64_t)n;
        if (lo < r.cb) {
            r.pos = lo + n;
            brev_fill(r);
        }
        v = (r.cache >> (uint32_t)(lo - r.cb)) & ((1ull << n) - 1ull);
    }
    r.pos -= n;
    return v;
}

// The same bitstream read through a 64-bit window that slides down 32 bits
// at a time, with the next 4-8 dwords (two 16-byte groups) already loaded or
// in flight: a refill never waits on memory.  Reads are at most 32 bits.
// Invariant: the window holds bits [B, B + 64) and B <= pos (pos - B < 64);
// g0.w is the dword of bits [B - 32, B), then g0.z, g0.y, g0.x, g1.w, ...
struct BRevQ {  // 32-bit positions: the scalar unit has no 64-bit signed compare
    const uint8_t *base;
    int32_t len;
    int32_t pos;
    int32_t B;
    uint64_t acc;
    uint4 g0, g1;
    uint32_t used;  // dwords of the original g0 shifted in (0..3)
    // LDS prefetch (the wave-uniform sequence reader): the group after g0,
    // bytes [nbyte, nbyte + 16), loaded by the global_load_lds of lanes 0-4
    // into pf when g0 was taken and read 4 slides later.  With the dwords
    // loaded into registers and aligned at once, every 4th slide waited for
    // a memory round trip; keeping them in VGPRs spilled (128 VGPRs).
    __attribute__((address_space(3))) uint32_t *pf;
    int32_t nbyte;
};

// A wave-uniform value in a scalar register: the serial sequence decode then
// runs on the scalar unit (a wave64 VALU op takes 4 cycles for one useful
// lane; r5j: 0.7 us per sequence, VALU-issue bound).
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    return (uint64_t)rfl((uint32_t)v) | (uint64_t)rfl((uint32_t)(v >> 32)) << 32;
}

// 4 bytes at base + byte (any alignment), bytes outside [0, len) as 0; U:
// the reader is wave-uniform (every lane reads the same stream)
template <bool U = false>
__device__ __forceinline__ uint32_t brq_ld4(const uint8_t *base, int64_t len, int64_t byte) {
    uint32_t v = 0;
    if (byte >= 0 && byte + 4 <= len) {
        v = ld4u(base + byte);
    } else {
        for (int i = 0; i < 4; i++)
            if (byte + i >= 0 && byte + i < len) v |= (uint32_t)gptr(base)[byte + i] << (8 * i);
    }
    return U ? rfl(v) : v;
}

// the 16 bytes [byte, byte + 16) as dwords x (lowest) .. w
template <bool U = false>
__device__ __forceinline__ uint4 brq_ld16(const uint8_t *base, int64_t len, int64_t byte) {
    return make_uint4(brq_ld4<U>(base, len, byte), brq_ld4<U>(base, len, byte + 4),
                      brq_ld4<U>(base, len, byte + 8), brq_ld4<U>(base, len, byte + 12));
}

// issue the next group's load into LDS (lanes 0-4, one dword each; no wait)
__device__ __forceinline__ void brq_fetch_lds(BRevQ &r, int32_t byte) {
    r.nbyte = byte;
    if (byte < 4 || byte + 20 > r.len) return;  // (the stream's ends: slow path)
    const uint8_t *a = r.base + byte;
    const uint32_t *w = (const uint32_t *)(a - ((uintptr_t)a & 3u));
    const uint32_t lane = __lane_id();
    if (lane < 5)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void *)(w + lane), r.pf, 4, 0, 0);
}

// the fetched group, wave-uniform (x lowest)
__device__ __forceinline__ uint4 brq_take_lds(BRevQ &r) {
    if (r.nbyte < 4 || r.nbyte + 20 > r.len) return brq_ld16<true>(r.base, r.len, r.nbyte);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the wave's LDS load has landed
    const uint32_t sh = (uint32_t)((uintptr_t)(r.base + r.nbyte) & 3u) * 8u;
    const uint32_t w0 = r.pf[0], w1 = r.pf[1], w2 = r.pf[2], w3 = r.pf[3], w4 = r.pf[4];
    return make_uint4(rfl(__builtin_amdgcn_alignbit(w1, w0, sh)), rfl(__builtin_amdgcn_alignbit(w2, w1, sh)),
                      rfl(__builtin_amdgcn_alignbit(w3, w2, sh)), rfl(__builtin_amdgcn_alignbit(w4, w3, sh)));
}

template <bool U = false>
__device__ __forceinline__ bool brq_init(BRevQ &r, const uint8_t *p, int64_t len64) {
    if (len64 <= 0 || len64 > (int64_t)kBlockMax) return false;  // streams of one block
    int32_t len = (int32_t)len64;
    if (U) {
        p = reinterpret_cast<const uint8_t *>(rfl64(reinterpret_cast<uintptr_t>(p)));
        len = (int32_t)rfl((uint32_t)len);
    }
    r.base = p;
    r.len = len;
    const uint32_t last = U ? rfl(p[len - 1]) : p[len - 1];
    if (last == 0) return false;
    r.pos = 8 * (len - 1) + (int32_t)highbit32(last);
    r.B = ((r.pos >> 5) << 5) - 32;  // arithmetic shifts: floor
    const int32_t by = r.B >> 3;
    r.acc = (uint64_t)brq_ld4<U>(p, len, by) | (uint64_t)brq_ld4<U>(p, len, by + 4) << 32;
    r.g0 = brq_ld16<U>(p, len, by - 16);
    if (U && r.pf)
        brq_fetch_lds(r, by - 32);
    else
        r.g1 = brq_ld16<U>(p, len, by - 32);
    r.used = 0;
    return true;
}

template <bool U = false>
__device__ __forceinline__ void brq_slide(BRevQ &r) {
    r.acc = (r.acc << 32) | r.g0.w;
    r.B -= 32;
    r.g0.w = r.g0.z;
    r.g0.z = r.g0.y;
    r.g0.y = r.g0.x;
    if (++r.used == 4) {
        if (U && r.pf) {
            r.g0 = brq_take_lds(r);
            brq_fetch_lds(r, (r.B >> 3) - 32);
        } else {
            r.g0 = r.g1;
            r.g1 = brq_ld16<U>(r.base, r.len, (r.B >> 3) - 32);
        }
        r.used = 0;
    }
}

template <bool U = false>
__device__ __forceinline__ uint32_t brq_peek(BRevQ &r, uint32_t n) {
    if (n == 0) return 0;
    const int32_t lo = r.pos - (int32_t)n;
    if (lo < r.B) brq_slide<U>(r);
    return (uint32_t)((r.acc >> (uint32_t)(lo - r.B)) & ((1ull << n) - 1ull));
}

template <bool U = false>
__device__ __forceinline__ uint32_t brq_bits(BRevQ &r, uint32_t n) {
    const uint32_t v = brq_peek<U>(r, n);
    r.pos -= n;
    return v;
}

// ---- FSE ---------------------------------------------------------------------

// FSE_readNCount: a table description at p (at most `avail` bytes);
// returns its byte length, or -1.  norm[0..*nsym) and *al are set.
__device__ int read_ncount(const uint8_t *p, int64_t avail, uint32_t max_sym, uint32_t max_al,
                           int16_t *norm, uint32_t *nsym, uint32_t *al) {
    if (avail < 1) return -1;
    const uint8_t *end = p + avail;
    int64_t bitpos = 0;  // from p
    auto rd32 = [&](int64_t bp) -> uint32_t {
        const uint64_t v = ld8b(p + (bp >> 3), p, end);
        return (uint32_t)(v >> (bp & 7));
    };
    uint32_t bs = rd32(0);
    int nb = (int)(bs & 0xF) + 5;
    if ((uint32_t)nb > max_al) return -1;
    *al = (uint32_t)nb;
    bitpos = 4;
    int remaining = (1 << nb) + 1;
    int threshold = 1 << nb;
    nb++;
    uint32_t s = 0;
    bool prev0 = false;
    while (remaining > 1 && s <= max_sym) {
        if (bitpos > 8 * avail) return -1;
        bs = rd32(bitpos);
        if (prev0) {
            uint32_t n0 = s;
            while ((bs & 0xFFFF) == 0xFFFF) {
                n0 += 24;
                bitpos += 16;
                if (bitpos > 8 * avail) return -1;
                bs = rd32(bitpos);
            }
            while ((bs & 3) == 3) {
                n0 += 3;
                bs >>= 2;
                bitpos += 2;
            }
            n0 += bs & 3;
            bitpos += 2;
            if (n0 > max_sym + 1 || n0 > kNormCap) return -1;
            while (s < n0) norm[s++] = 0;
            if (s > max_sym) break;
            bs = rd32(bitpos);
        }
        const int mx = (2 * threshold - 1) - remaining;
        int count;
        if ((int)(bs & (uint32_t)(threshold - 1)) < mx) {
            count = (int)(bs & (uint32_t)(threshold - 1));
            bitpos += nb - 1;
        } else {
            count = (int)(bs & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= mx;
            bitpos += nb;
        }
        count--;
        remaining -= count < 0 ? -count : count;
        if (s >= kNormCap) return -1;  // (a symbol this table cannot have)
        norm[s++] = (int16_t)count;
        prev0 = count == 0;
        while (remaining < threshold) {
            nb--;
            threshold >>= 1;
        }
        if (bitpos > 8 * avail) return -1;
    }
    if (remaining != 1 || s > max_sym + 1) return -1;
    *nsym = s;
    const int64_t used = (bitpos + 7) >> 3;
    return used > avail ? -1 : (int)used;
}

// FSE_buildDTable from norm[0..nsym) (accuracy al <= 9) into t (1 << al
// entries); false if the counts do not fill the table.  Uniform code; lane 0
// writes.
__device__ bool build_fse(FseD *t, const int16_t *norm, uint32_t nsym, uint32_t al, uint16_t *nxt,
                          uint32_t lane) {
    const uint32_t size = 1u << al, mask = size - 1;
    uint32_t high = size - 1;
    int total = 0;
    for (uint32_t s = 0; s < nsym; s++) total += norm[s] < 0 ? 1 : norm[s];
    if ((uint32_t)total != size) return false;
    for (uint32_t s = 0; s < nsym; s++) {
        if (norm[s] == -1) {
            if (lane == 0) t[high & mask].sym = (uint8_t)s;
            high--;
            if (lane == 0) nxt[s] = 1;
        } else if (lane == 0) {
            nxt[s] = (uint16_t)(norm[s] < 0 ? 0 : norm[s]);
        }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        for (int i = 0; i < norm[s]; i++) {
            if (lane == 0) t[pos].sym = (uint8_t)s;
            do {
                pos = (pos + step) & mask;
            } while (pos > high);
        }
    }
    if (pos != 0) return false;
    wsync();
    if (lane == 0) {
        for (uint32_t u = 0; u < size; u++) {
            const uint32_t s = t[u].sym & (kNormCap - 1u);
            const uint32_t ns = nxt[s]++;
            const uint32_t nb = al - highbit32(ns | 1u);
            t[u].nb = (uint8_t)nb;
            t[u].next = (uint16_t)((ns << nb) - size);
        }
    }
    wsync();
    return true;
}

__device__ bool build_predefined(FseD *t, const int16_t *src, uint32_t nsym, uint32_t al,
                                 int16_t *norm, uint16_t *nxt, uint32_t lane) {
    if (lane < nsym) norm[lane] = src[lane];
    wsync();
    return build_fse(t, norm, nsym, al, nxt, lane);
}

// ---- Huffman -----------------------------------------------------------------

// Huffman weights (HUF_readStats) at p (avail bytes) -> L.w[0..*nw), the
// implied last weight appended; returns the description's length or -1.
__device__ int read_huf_weights(const uint8_t *p, int64_t avail, ZstdLds &L, uint32_t *nw,
                                uint32_t lane) {
    if (avail < 1) return -1;
    const uint32_t hb = p[0];
    uint32_t n = 0;
    int used;
    if (hb >= 128) {
        n = hb - 127;
        used = 1 + (int)((n + 1) / 2);
        if (used > avail) return -1;
        if (lane < n) {
            const uint32_t byte = p[1 + lane / 2];
            L.w[lane] = (uint8_t)((lane & 1) ? (byte & 15u) : (byte >> 4));
        }
        if (lane + 64 < n) {
            const uint32_t k = lane + 64, byte = p[1 + k / 2];
            L.w[k] = (uint8_t)((k & 1) ? (byte & 15u) : (byte >> 4));
        }
        wsync();
    } else {
        // FSE-compressed weights: NCount (log <= 6), then two interleaved
        // states over a backward bitstream (FSE_decompress_usingDTable);
        // the states masked to the 64 entries of hw
        used = 1 + (int)hb;
        if (used > avail || hb == 0) return -1;
        uint32_t nsym = 0, al = 0;
        const int nc = read_ncount(p + 1, hb, 255, 6, L.norm, &nsym, &al);
        if (nc < 0) return -1;
        wsync();
        if (!build_fse(L.u.h.hw, L.norm, nsym, al, L.nxt, lane)) return -1;
        BRev r;
        if (!brev_init(r, p + 1 + nc, (int64_t)hb - nc)) return -1;
        uint32_t s1 = (uint32_t)brev_bits(r, al) & 63u, s2 = (uint32_t)brev_bits(r, al) & 63u;
        for (;;) {
            if (n >= 255) return -1;
            FseD e = L.u.h.hw[s1];
            if (lane == 0) L.w[n] = e.sym;
            n++;
            s1 = (e.next + (uint32_t)brev_bits(r, e.nb)) & 63u;
            if (r.pos < 0) {
                if (n >= 255) return -1;
                if (lane == 0) L.w[n] = L.u.h.hw[s2].sym;
                n++;
                break;
            }
            if (n >= 255) return -1;
            e = L.u.h.hw[s2];
            if (lane == 0) L.w[n] = e.sym;
            n++;
            s2 = (e.next + (uint32_t)brev_bits(r, e.nb)) & 63u;
            if (r.pos < 0) {
                if (n >= 255) return -1;
                if (lane == 0) L.w[n] = L.u.h.hw[s1].sym;
                n++;
                break;
            }
        }
        wsync();
    }
    // the last weight is implied: the weights fill a power of two
    uint32_t total = 0, ones = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t wi = L.w[i];
        if (wi > 11) return -1;
        total += wi ? (1u << (wi - 1)) : 0u;
        ones += wi == 1u;
    }
    if (total == 0) return -1;
    const uint32_t tl = highbit32(total) + 1;
    if (tl > 11) return -1;
    const uint32_t rest = (1u << tl) - total;
    if (rest & (rest - 1)) return -1;
    // HUF_readStats' tree check: an even number, at least 2, of weight-1
    // symbols (codes of the full table log), the implied last one included.
    // Without it a table whose codes are all shorter than its log decodes,
    // but libzstd calls it corrupt (r6 checker soak, seed 5627)
    ones += rest == 1u;
    if (ones < 2 || (ones & 1u)) return -1;
    wsync();
    if (lane == 0) L.w[n] = (uint8_t)(highbit32(rest) + 1);
    *nw = n + 1;
    wsync();
    return used;
}

// HUF_readDTableX1 from L.w[0..nw) (checked by read_huf_weights: weights
// <= 11 that fill 2^tl <= 2048 entries) -> L.u.h.huf; returns the table log.
// Hard: hold that again here (weights clamped, stores guarded), whatever L.w
// holds; the decompressor's choice.  The checker relies on read_huf_weights
// alone: the extra checks cost it scratch and with that speed (DESIGN.md
// 3g-bis).
template <bool Hard>
__device__ uint32_t build_huf(ZstdLds &L, uint32_t nw, uint32_t lane) {
    uint32_t cnt[13] = {0};
    uint32_t total = 0;
    for (uint32_t s = 0; s < nw; s++) {
        const uint32_t wi = Hard && L.w[s] >= 12 ? 0u : L.w[s];
        cnt[wi]++;
        total += wi ? (1u << (wi - 1)) : 0u;
    }
    const uint32_t tl = highbit32(Hard ? total | 1u : total);  // total is a power of two now
    uint32_t start[13];
    uint32_t nx = 0;
    for (uint32_t wi = 1; wi <= (Hard ? 12u : tl); wi++) {
        start[wi] = nx;
        nx += cnt[wi] << (wi - 1);
    }
    // symbols of weight wi fill 2^(wi-1) entries each, in symbol order: lane l
    // writes the entries of symbol s with l in the range (all lanes stride)
    for (uint32_t s = 0; s < nw; s++) {
        const uint32_t wi = Hard && L.w[s] >= 12 ? 0u : L.w[s];
        if (!wi) continue;
        const uint32_t len = 1u << (wi - 1), b = start[wi];
        start[wi] += len;
        for (uint32_t k = lane; k < len; k += 64) {
            if (!Hard || b + k < 2048u) {
                L.u.h.huf[b + k].sym = (uint8_t)s;
                L.u.h.huf[b + k].nb = (uint8_t)(tl + 1 - wi);
            }
        }
    }
    wsync();
    return tl;
}

// One Huffman stream [p, p + len) -> n symbols at out (one lane; out[0, n) is
// inside a span the caller took).  Hard: a stream that has run out of bits
// ends the loop at once, not at its n-th symbol (the decompressor's choice;
// the verdict is the same, and the reader gives zeros below the stream's
// start either way).
template <bool Hard>
__device__ bool huf_stream(const ZstdLds &L, uint32_t tl, const uint8_t *p, int64_t len, uint8_t *out,
                           uint32_t n) {
    BRevQ r;
    r.pf = nullptr;  // (per-lane streams: no LDS prefetch)
    if (n == 0) return len == 0 || (brq_init(r, p, len) && r.pos == 0);
    if (!brq_init(r, p, len)) return false;
    uint32_t i = 0;
    // four symbols per dword store once aligned
    while (i < n && ((uintptr_t)(out + i) & 3u)) {
        const HufD e = L.u.h.huf[brq_peek(r, tl)];
        out[i++] = e.sym;
        r.pos -= e.nb;
    }
    for (; i + 4 <= n; i += 4) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const HufD e = L.u.h.huf[brq_peek(r, tl)];
            v |= (uint32_t)e.sym << (8 * k);
            r.pos -= e.nb;
        }
        *reinterpret_cast<uint32_t *>(out + i) = v;
        if (Hard && r.pos < 0) return false;  // (also keeps a corrupt stream's reads near it)
    }
    for (; i < n; i++) {
        const HufD e = L.u.h.huf[brq_peek(r, tl)];
        out[i] = e.sym;
        r.pos -= e.nb;
    }
    return r.pos == 0;
}

// ---- a compressed block's sections ---------------------------------------------

// Literals_Section_Header (3.1.1.3.1.1) of a block [p, p + bs), bs >= 3:
// false if it does not fit the block.
struct LitHdr {
    uint32_t ltype, regen, csize, hdr, nstreams;
};
__device__ bool lit_header(const uint8_t *p, uint32_t bs, LitHdr &h) {
    const uint32_t b0 = p[0];
    const uint32_t sf = (b0 >> 2) & 3u;
    h.ltype = b0 & 3u;
    h.csize = 0;
    h.nstreams = 1;
    if (h.ltype < 2) {
        if (sf == 0 || sf == 2) {
            h.regen = b0 >> 3;
            h.hdr = 1;
        } else if (sf == 1) {
            h.regen = (b0 >> 4) | ((uint32_t)p[1] << 4);
            h.hdr = 2;
        } else {
            h.regen = (b0 >> 4) | ((uint32_t)p[1] << 4) | ((uint32_t)p[2] << 12);
            h.hdr = 3;
        }
    } else {
        h.nstreams = sf == 0 ? 1u : 4u;
        if (sf < 2) {
            const uint32_t v = b0 | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            h.regen = (v >> 4) & 0x3FFu;
            h.csize = (v >> 14) & 0x3FFu;
            h.hdr = 3;
        } else if (sf == 2) {
            if (bs < 4) return false;
            const uint32_t v = b0 | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) |
                               ((uint32_t)p[3] << 24);
            h.regen = (v >> 4) & 0x3FFFu;
            h.csize = v >> 18;
            h.hdr = 4;
        } else {
            if (bs < 5) return false;
            const uint64_t v = b0 | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) |
                               ((uint64_t)p[3] << 24) | ((uint64_t)p[4] << 32);
            h.regen = (uint32_t)((v >> 4) & 0x3FFFFu);
            h.csize = (uint32_t)((v >> 22) & 0x3FFFFu);
            h.hdr = 5;
        }
    }
    if (h.regen > kBlockMax) return false;
    // the section's bytes, then at least the sequence count's first byte
    const uint64_t body = h.ltype == 0 ? h.regen : h.ltype == 1 ? 1u : h.csize;
    return (uint64_t)h.hdr + body < bs;
}

// Number_of_Sequences (3.1.1.3.2.1) at q (< end); returns the bytes it takes,
// 0 if cut off.
__device__ uint32_t seq_count(const uint8_t *q, const uint8_t *end, uint32_t *nseq) {
    const uint32_t b = q[0];
    if (b < 128) {
        *nseq = b;
        return 1;
    }
    if (b < 255) {
        if (q + 2 > end) return 0;
        *nseq = ((b - 128) << 8) + q[1];
        return 2;
    }
    if (q + 3 > end) return 0;
    *nseq = q[1] + ((uint32_t)q[2] << 8) + 0x7F00u;
    return 3;
}

// The entropy tables a block may take over from the block before it (the
// tables themselves stay in the wave's LDS).  A frame starts with none; so
// does every block of a pass that takes blocks out of order.
struct Tables {
    uint32_t huf_log;  // 0: no Huffman table yet
    uint32_t huf_nw;   // its weights in L.w[0 .. huf_nw)
    uint32_t al_ll, al_of, al_ml;  // 255: no table yet
};
__device__ __forceinline__ void tables_reset(Tables &S) {
    S.huf_log = 0;
    S.huf_nw = 0;
    S.al_ll = S.al_of = S.al_ml = 255u;
}

// What a section step found: done, malformed, or a treeless literals section
// or repeat-mode table with no earlier table in S (the caller knows whether
// that is the frame's fault or its own pass's).
constexpr uint32_t kSecOk = 0, kSecBad = 1, kSecNeedsTable = 2;

// The streams of a Huffman literals section [cs, cs + clen) after its tree
// description -> regen bytes at out, with the table of log tl in L: one
// stream on lane 0 or four on lanes 0-3.
template <bool Hard>
__device__ uint32_t huf_streams(const ZstdLds &L, uint32_t tl, uint32_t nstreams,
                                                const uint8_t *cs, int64_t clen, uint8_t *out,
                                                uint32_t regen, uint32_t lane) {
    bool ok = true;
    if (nstreams == 1) {
        if (lane == 0) ok = huf_stream<Hard>(L, tl, cs, clen, out, regen);
    } else {
        if (clen < 6) return kSecBad;
        const int64_t s1 = cs[0] | (cs[1] << 8), s2 = cs[2] | (cs[3] << 8), s3 = cs[4] | (cs[5] << 8);
        const int64_t s4 = clen - 6 - s1 - s2 - s3;
        const uint32_t seg = (regen + 3) / 4;
        if (s4 < 0 || 3 * seg > regen) return kSecBad;
        if (lane < 4) {
            const int64_t off = 6 + (lane > 0 ? s1 : 0) + (lane > 1 ? s2 : 0) + (lane > 2 ? s3 : 0);
            const int64_t ln = lane == 0 ? s1 : lane == 1 ? s2 : lane == 2 ? s3 : s4;
            const uint32_t nn = lane < 3 ? seg : regen - 3 * seg;
            ok = huf_stream<Hard>(L, tl, cs + off, ln, out + lane * seg, nn);
        }
    }
    if (__builtin_amdgcn_ballot_w64(!ok)) return kSecBad;
    wsync();
    return kSecOk;
}

// The Huffman literals step of a block whose header is h (ltype 2 or 3): the
// section's csize bytes at cs -> h.regen bytes at out.  Its tree, or for a
// treeless section the table of S rebuilt from the weights still in L.w (the
// table's bytes held LL / ML extras since).  Hard: as build_huf and
// huf_stream.
template <bool Hard>
__device__ uint32_t huf_literals(ZstdLds &L, Tables &S, const LitHdr &h,
                                                 const uint8_t *cs, uint8_t *out, uint32_t lane) {
    int64_t clen = h.csize;
    if (h.ltype == 2) {
        uint32_t nw = 0;
        const int tu = read_huf_weights(cs, clen, L, &nw, lane);
        if (tu < 0) return kSecBad;
        S.huf_log = build_huf<Hard>(L, nw, lane);
        S.huf_nw = nw;
        cs += tu;
        clen -= tu;
    } else if (S.huf_log == 0) {  // treeless: the previous block's table
        return kSecNeedsTable;
    } else {
        build_huf<Hard>(L, S.huf_nw, lane);
    }
    return huf_streams<Hard>(L, S.huf_log, h.nstreams, cs, clen, out, h.regen, lane);
}

// The sequence-table step: the modes byte at q (Symbol_Compression_Modes,
// 3.1.1.3.2.1) and the tables it announces into L.ll / L.of / L.ml, then the
// LL / ML extras per state.  q moves past the table descriptions, to the
// sequences' bitstream.
__device__ uint32_t seq_tables(ZstdLds &L, Tables &S, const uint8_t *&q,
                                               const uint8_t *end, uint32_t lane) {
    if (q >= end) return kSecBad;
    const uint32_t modes = *q++;
    // reserved bits 1-0 must be zero (RFC 8878 3.1.1.3.2.1; libzstd 1.5,
    // the reference's, rejects them, 1.4.8 decodes)
    if (modes & 3u) return kSecBad;
    // tables in the order LL, OF, ML
    for (int k = 0; k < 3; k++) {
        const uint32_t mode = (modes >> (6 - 2 * k)) & 3u;
        FseD *t = k == 0 ? L.ll : k == 1 ? L.of : L.ml;
        uint32_t &al = k == 0 ? S.al_ll : k == 1 ? S.al_of : S.al_ml;
        const uint32_t max_sym = k == 0 ? 35u : k == 1 ? 31u : 52u;
        const uint32_t max_al = k == 0 ? 9u : k == 1 ? 8u : 9u;
        if (mode == 0) {
            const int16_t *nrm = k == 0 ? kLLNorm : k == 1 ? kOFNorm : kMLNorm;
            const uint32_t ns = k == 0 ? 36u : k == 1 ? 29u : 53u;
            const uint32_t a = k == 1 ? 5u : 6u;
            if (!build_predefined(t, nrm, ns, a, L.norm, L.nxt, lane)) return kSecBad;
            al = a;
        } else if (mode == 1) {
            if (q >= end) return kSecBad;
            const uint32_t s = *q++;
            if (s > max_sym) return kSecBad;
            if (lane == 0) {
                t[0].sym = (uint8_t)s;
                t[0].nb = 0;
                t[0].next = 0;
            }
            wsync();
            al = 0;
        } else if (mode == 2) {
            uint32_t ns = 0, a = 0;
            const int u = read_ncount(q, end - q, max_sym, max_al, L.norm, &ns, &a);
            if (u < 0) return kSecBad;
            wsync();
            if (!build_fse(t, L.norm, ns, a, L.nxt, lane)) return kSecBad;
            al = a;
            q += u;
        } else if (al == 255u) {  // repeat: needs an earlier table
            return kSecNeedsTable;
        }
    }
    for (uint32_t u = lane; u < (1u << S.al_ll); u += 64) {
        const uint32_t c = L.ll[u].sym < 36 ? L.ll[u].sym : 0u;
        L.u.x.llx[u] = kLLBase[c] | (uint32_t)kLLBits[c] << 24;
    }
    for (uint32_t u = lane; u < (1u << S.al_ml); u += 64) {
        const uint32_t c = L.ml[u].sym < 53 ? L.ml[u].sym : 0u;
        L.u.x.mlx[u] = kMLBase[c] | (uint32_t)kMLBits[c] << 24;
    }
    wsync();
    return kSecOk;
}

// ---- the frame header ----------------------------------------------------------

// The window a frame asks its decoder for (RFC 8878 3.1.1.1.2; a
// single-segment frame's is its content size).
__device__ __forceinline__ uint64_t window_size(uint32_t single, uint32_t wd, uint64_t fcs) {
    if (single) return fcs;
    const uint64_t base = 1ull << (10u + (wd >> 3));
    return base + (base >> 3) * (wd & 7u);
}

// decode_all (decrypt.rs:71-95) reads the decoder through io::copy into a
// Vec, whose first read offers 8 KiB of output (DEFAULT_BUF_SIZE).  A frame
// whose content size is known and fits takes libzstd's one-pass shortcut
// (ZSTD_decompressStream -> ZSTD_decompress_usingDDict): no window limit,
// and an empty compressed block is corrupt.  Other frames go through the
// stage machine: the window limit applies and empty blocks of any type are
// skipped.  The stage machine also holds every block to Block_Maximum_Size =
// min(window, 128 KiB) (size field and regenerated bytes, RFC 8878 3.1.1.2.3)
// and reaches back at most one window (3.1.1.1.2); the one-pass path has the
// whole output before it and checks neither.  Both decoders follow the path
// decode_all would take.
constexpr uint64_t kDecodeAllFirstOut = 8192;

struct FrameHdr {
    uint32_t single, cksum;  // Single_Segment_Flag, Content_Checksum_Flag
    uint32_t fcs_len;        // bytes of Frame_Content_Size, 0: none
    uint64_t fcs;
    bool shortcut;           // decode_all's one-pass path
    uint64_t W;              // the window
    uint32_t bmax;           // Block_Maximum_Size
    uint32_t wlim;           // largest match offset: the window (~0u: no limit)
    uint32_t len;            // the header's bytes: the first block header follows
};

// The frame header at f (len bytes of frame): magic, reserved bit, dictionary
// id, content size, the one-pass rule, window and Block_Maximum_Size.  False:
// malformed, or a feature these readers lack (dictionaries, skippable
// frames), or a window past the limit of rustic's decode_all: the zstd
// crate's streaming decoder keeps libzstd's default, windows up to 2^27 + 1
// bytes (ZSTD_WINDOWLOG_LIMIT_DEFAULT; larger ones fail with "Frame requires
// too much memory for decoding").
__device__ bool frame_header(const uint8_t *f, uint64_t len, FrameHdr &H) {
    if (len < 6) return false;
    const uint32_t magic = f[0] | (f[1] << 8) | (f[2] << 16) | ((uint32_t)f[3] << 24);
    const uint32_t fhd = f[4];
    if (magic != 0xFD2FB528u || (fhd & 8u)) return false;  // (bit 3: reserved)
    const uint32_t fcs_flag = fhd >> 6, did_flag = fhd & 3u;
    H.single = (fhd >> 5) & 1u;
    H.cksum = (fhd >> 2) & 1u;
    const uint8_t *q = f + 5 + (H.single ? 0 : 1);  // window descriptor
    const uint32_t did_len = did_flag == 0 ? 0 : did_flag == 1 ? 1 : did_flag == 2 ? 2 : 4;
    H.fcs_len = fcs_flag == 0 ? (H.single ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
    if (q + did_len + H.fcs_len > f + len) return false;
    uint32_t did = 0;
    for (uint32_t j = 0; j < did_len; j++) did |= (uint32_t)q[j] << (8 * j);
    if (did) return false;  // dictionaries: not supported
    q += did_len;
    uint64_t fcs = 0;
    for (uint32_t j = 0; j < H.fcs_len; j++) fcs |= (uint64_t)q[j] << (8 * j);
    if (H.fcs_len == 2) fcs += 256;
    q += H.fcs_len;
    H.fcs = fcs;
    H.shortcut = H.fcs_len && fcs <= kDecodeAllFirstOut;
    H.W = window_size(H.single, H.single ? 0u : f[5], fcs);
    if (!H.shortcut && H.W > (1ull << 27) + 1ull) return false;
    // Block_Maximum_Size and the reach of a match (the window fits 32 bits)
    H.bmax = H.shortcut ? kBlockMax : (uint32_t)min(H.W, (uint64_t)kBlockMax);
    H.wlim = H.shortcut ? ~0u : (uint32_t)H.W;
    H.len = (uint32_t)(q - f);
    return true;
}

// ---- XXH64 -------------------------------------------------------------------
// XXH64 (seed 0) of data[0, n), its low 32 bits: a frame's Content_Checksum
// (RFC 8878 3.1.1).  The four accumulators of the 32-byte stripes are
// independent: lanes 0-3 take one 8-byte word of each stripe; the merge and
// the tail of < 32 bytes are uniform code.  Only frames that carry a checksum
// come here (this library's encoder writes none), after their last block: a
// call, so that nothing of it is live in the sequence loop.
constexpr uint64_t kXP1 = 0x9E3779B185EBCA87ull, kXP2 = 0xC2B2AE3D27D4EB4Full,
                   kXP3 = 0x165667B19E3779F9ull, kXP4 = 0x85EBCA77C2B2AE63ull,
                   kXP5 = 0x27D4EB2F165667C5ull;
__device__ __forceinline__ uint64_t xrotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t in) {
    return xrotl(acc + in * kXP2, 31) * kXP1;
}
__device__ __forceinline__ uint64_t xmerge(uint64_t h, uint64_t v) {
    return (h ^ xround(0, v)) * kXP1 + kXP4;
}
__device__ __noinline__ uint32_t xxh64_low32(const uint8_t *data, uint64_t n, uint32_t lane) {
    uint64_t h;
    const uint64_t stripes = n / 32;
    if (stripes) {
        const uint32_t k = lane & 3u;  // (lanes above 3 repeat lanes 0-3: in bounds, unused)
        uint64_t acc = k == 0 ? kXP1 + kXP2 : k == 1 ? kXP2 : k == 2 ? 0ull : 0ull - kXP1;
        const uint8_t *p = data + 8u * k;
        uint64_t s = 0;
        for (; s + 4 <= stripes; s += 4, p += 128) {  // four loads in flight
            const uint64_t a = ld8u(p), b = ld8u(p + 32), c = ld8u(p + 64), d = ld8u(p + 96);
            acc = xround(xround(xround(xround(acc, a), b), c), d);
        }
        for (; s < stripes; s++, p += 32) acc = xround(acc, ld8u(p));
        const uint64_t v1 = __shfl(acc, 0), v2 = __shfl(acc, 1), v3 = __shfl(acc, 2),
                       v4 = __shfl(acc, 3);
        h = xrotl(v1, 1) + xrotl(v2, 7) + xrotl(v3, 12) + xrotl(v4, 18);
        h = xmerge(xmerge(xmerge(xmerge(h, v1), v2), v3), v4);
    } else {
        h = kXP5;
    }
    h += n;
    const auto *t = gptr(data);
    uint64_t i = stripes * 32;
    auto le = [&](uint64_t at, uint32_t nb) {  // nb bytes, each inside [0, n)
        uint64_t v = 0;
        for (uint32_t j = 0; j < nb; j++) v |= (uint64_t)t[at + j] << (8u * j);
        return v;
    };
    for (; i + 8 <= n; i += 8) h = xrotl(h ^ xround(0, le(i, 8)), 27) * kXP1 + kXP4;
    if (i + 4 <= n) {
        h = xrotl(h ^ le(i, 4) * kXP1, 23) * kXP2 + kXP3;
        i += 4;
    }
    for (; i < n; i++) h = xrotl(h ^ (uint64_t)t[i] * kXP5, 11) * kXP1;
    h ^= h >> 33;
    h *= kXP2;
    h ^= h >> 29;
    h *= kXP3;
    h ^= h >> 32;
    return (uint32_t)h;
}

}  // namespace
