// rcdc_zstd_dx.hip -- zstd frames decompressed on the device: decode_all of
// rustic's read path (backend/decrypt.rs:71-97 read_encrypted_from_partial,
// commands/check.rs:718-814 check_pack) for frames in HBM.
//
// Three kernels, no waiting between workgroups anywhere:
//   rcdc_zdx_blocks_kernel   a thread per frame walks the frame header, every
//                            block header and, for compressed blocks, the
//                            literals-section header, the sequence count and
//                            the modes byte (ZdxFrame, ZdxBlk).
//   rcdc_zdx_entropy_kernel  a wave per compressed block, from a queue: the
//                            literals and the sequences decoded into the
//                            block's slot of the workspace (the parallel
//                            stage).  rcdc_zdx_inorder_kernel runs the same
//                            device function a wave per frame, blocks in
//                            order with the tables carried along, for frames
//                            with repeat-mode tables.
//   rcdc_zdx_copy_kernel     a wave per frame, blocks in order: repeat
//                            offsets resolved, literals and matches copied to
//                            the output.  The only kernel that writes d_out.
// Status per frame: 0 decoded, 1 valid so far but the output does not fit
// out_cap, 2 malformed or not readable here -- the frame-level rules are the
// checker's (rcdc_zstd_dec.hip), of which this unit keeps its own copies of
// the bit readers, table builders, predefined tables and XXH64: the checker's
// translation unit stays as it is.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rcdc_internal.h"

using namespace rcdc;

namespace {

constexpr uint32_t kDxOk = 0, kDxFull = 1, kDxBad = 2;
constexpr uint32_t kBlockMax = 128u << 10;
// every match is at least 3 bytes: more sequences cannot stay within a block
constexpr uint32_t kSeqMax = kBlockMax / 3u;

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

struct FseD {
    uint8_t sym, nb;
    uint16_t next;
};
struct HufD {
    uint8_t sym, nb;
};

// LDS of one entropy wave (workgroup = one wave): the checker's layout, 9984 B,
// 16 waves per CU.  The Huffman table lives through a block's literals, the
// LL / ML extras through its sequences.
struct DxLds {
    FseD ll[512], ml[512], of[256];
    union {
        struct {
            FseD hw[64];
            HufD huf[2048];
        } h;
        struct {
            uint32_t llx[512], mlx[512];  // baseline | extra bits << 24 per state
        } x;
    } u;
    int16_t norm[64];
    uint16_t nxt[64];
    uint8_t w[256];  // Huffman weights (kept for treeless literals, in-order pass)
    uint32_t pf[8];  // the sequence reader's next group
};
constexpr uint32_t kNormCap = 64;

__device__ __forceinline__ uint32_t highbit32(uint32_t v) { return 31u - (uint32_t)__clz(v); }

__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
}

// ---- bounded regions ---------------------------------------------------------
// Every store to d_out and to the workspace goes to a pointer span_at gave:
// [off, off + n) of a region, or nullptr when that leaves it (the caller
// turns it into status 2, or 1 for the output's capacity).
struct Span {
    uint8_t *base;
    uint64_t cap;
};
__device__ __forceinline__ uint8_t *span_at(const Span &s, uint64_t off, uint64_t n) {
    return (off <= s.cap && n <= s.cap - off) ? s.base + off : nullptr;
}
__device__ __forceinline__ Span region(uint8_t *ws, uint64_t off, uint64_t cap) {
    Span s;
    s.base = ws + off;
    s.cap = cap;
    return s;
}

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
struct BRev {
    const uint8_t *base;
    int64_t len;
    int64_t pos;
    int64_t cb;
    uint64_t cache;
};

__device__ __forceinline__ void brev_fill(BRev &r) {
    r.cb = ((r.pos - 57) >> 3) << 3;
    r.cache = ld8b(r.base + (r.cb >> 3), r.base, r.base + r.len);
}

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

// The same stream through a 64-bit window that slides down 32 bits at a time
// with the next groups of 16 bytes loaded ahead; 32-bit positions (scalar
// compares); U: wave-uniform reader, the next group prefetched through LDS.
struct BRevQ {
    const uint8_t *base;
    int32_t len;
    int32_t pos;
    int32_t B;
    uint64_t acc;
    uint4 g0, g1;
    uint32_t used;
    __attribute__((address_space(3))) uint32_t *pf;
    int32_t nbyte;
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    return (uint64_t)rfl((uint32_t)v) | (uint64_t)rfl((uint32_t)(v >> 32)) << 32;
}

// 4 bytes at base + byte, bytes outside [0, len) as 0
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
    r.B = ((r.pos >> 5) << 5) - 32;
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

// FSE_readNCount: returns the description's byte length, or -1.
__device__ int read_ncount(const uint8_t *p, int64_t avail, uint32_t max_sym, uint32_t max_al,
                           int16_t *norm, uint32_t *nsym, uint32_t *al) {
    if (avail < 1) return -1;
    const uint8_t *end = p + avail;
    int64_t bitpos = 0;
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
        if (s >= kNormCap) return -1;
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
// entries); uniform code, lane 0 writes.
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

// HUF_readStats at p (avail bytes) -> L.w[0..*nw), the implied last weight
// appended; returns the description's length or -1.
__device__ int read_huf_weights(const uint8_t *p, int64_t avail, DxLds &L, uint32_t *nw,
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
    // HUF_readStats' tree check: an even number, at least 2, of weight-1 symbols
    ones += rest == 1u;
    if (ones < 2 || (ones & 1u)) return -1;
    wsync();
    if (lane == 0) L.w[n] = (uint8_t)(highbit32(rest) + 1);
    *nw = n + 1;
    wsync();
    return used;
}

// HUF_readDTableX1 from L.w[0..nw) (checked by read_huf_weights: the weights
// fill 2^tl <= 2048 entries) -> L.u.h.huf; returns the table log.
__device__ uint32_t build_huf(DxLds &L, uint32_t nw, uint32_t lane) {
    uint32_t cnt[13] = {0};
    uint32_t total = 0;
    for (uint32_t s = 0; s < nw; s++) {
        const uint32_t wi = L.w[s] < 12 ? L.w[s] : 0u;
        cnt[wi]++;
        total += wi ? (1u << (wi - 1)) : 0u;
    }
    const uint32_t tl = highbit32(total | 1u);
    uint32_t start[13];
    uint32_t nx = 0;
    for (uint32_t wi = 1; wi <= 12; wi++) {
        start[wi] = nx;
        nx += cnt[wi] << (wi - 1);
    }
    for (uint32_t s = 0; s < nw; s++) {
        const uint32_t wi = L.w[s] < 12 ? L.w[s] : 0u;
        if (!wi) continue;
        const uint32_t len = 1u << (wi - 1), b = start[wi];
        start[wi] += len;
        for (uint32_t k = lane; k < len; k += 64) {
            if (b + k < 2048u) {
                L.u.h.huf[b + k].sym = (uint8_t)s;
                L.u.h.huf[b + k].nb = (uint8_t)(tl + 1 - wi);
            }
        }
    }
    wsync();
    return tl;
}

// One Huffman stream [p, p + len) -> n symbols at out (one lane; out[0, n) is
// inside a span the caller took).
__device__ bool huf_stream(const DxLds &L, uint32_t tl, const uint8_t *p, int64_t len, uint8_t *out,
                           uint32_t n) {
    BRevQ r;
    r.pf = nullptr;
    if (n == 0) return len == 0 || (brq_init(r, p, len) && r.pos == 0);
    if (!brq_init(r, p, len)) return false;
    uint32_t i = 0;
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
        if (r.pos < 0) return false;  // (also keeps a corrupt stream's reads near it)
    }
    for (; i < n; i++) {
        const HufD e = L.u.h.huf[brq_peek(r, tl)];
        out[i] = e.sym;
        r.pos -= e.nb;
    }
    return r.pos == 0;
}

// ---- copies by the whole wave -------------------------------------------------

// dst[0, n) = src[0, n); the ranges do not overlap (or src == dst side by side
// without a shared byte); dst[0, n) is inside a span the caller took.  The
// 4-aligned body of dst in dword stores of bytes loaded at any alignment.
__device__ void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t lane) {
    uint64_t head = (4u - ((uintptr_t)dst & 3u)) & 3u;
    if (head > n) head = n;
    if (lane < head) dst[lane] = gptr(src)[lane];
    const uint64_t nd = (n - head) / 4;
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst + head);
    const uint8_t *s = src + head;
    for (uint64_t k = lane; k < nd; k += 64) d4[k] = ld4u(s + 4 * k);
    const uint64_t done = head + 4 * nd;
    if (lane < n - done) dst[done + lane] = gptr(src)[done + lane];
}

__device__ void wave_fill(uint8_t *dst, uint32_t v, uint64_t n, uint32_t lane) {
    uint64_t head = (4u - ((uintptr_t)dst & 3u)) & 3u;
    if (head > n) head = n;
    if (lane < head) dst[lane] = (uint8_t)v;
    const uint64_t nd = (n - head) / 4;
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint64_t k = lane; k < nd; k += 64) d4[k] = v * 0x01010101u;
    const uint64_t done = head + 4 * nd;
    if (lane < n - done) dst[done + lane] = (uint8_t)v;
}

// A match by the whole wave: dst[i] = dst[i - off], i in [0, n); the off
// bytes before dst are complete.  off >= n is a plain copy.  Otherwise the
// bytes before dst + done are periodic with period off, so each phase copies
// as many as a whole number of periods gives, from the start of that region:
// the copied length doubles (offset 1, 128 KiB: 17 phases).
__device__ void wave_match(uint8_t *dst, uint64_t off, uint64_t n, uint32_t lane) {
    const uint8_t *src = dst - off;
    if (off >= n) {
        wave_copy(dst, src, n, lane);
        return;
    }
    uint64_t done = 0;
    while (done < n) {
        const uint64_t ph = done % off;
        uint64_t c = off + done - ph;  // src + ph + c == dst + done
        if (c > n - done) c = n - done;
        wave_copy(dst + done, src + ph, c, lane);
        done += c;
        wsync();
    }
}

// ---- the header walk -----------------------------------------------------------

__device__ __forceinline__ uint64_t window_size(uint32_t single, uint32_t wd, uint64_t fcs) {
    if (single) return fcs;
    const uint64_t base = 1ull << (10u + (wd >> 3));
    return base + (base >> 3) * (wd & 7u);
}
// decode_all's one-pass path: a declared content size within its first 8 KiB read
constexpr uint64_t kDecodeAllFirstOut = 8192;

// Literals_Section_Header of a block [p, p + bs), bs >= 3: false if it does
// not fit the block.
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

// Number_of_Sequences at q (< end); returns the bytes it takes, 0 if cut off.
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

}  // namespace

// refs: frame_off, frame_len, out_off, out_cap (rcdc_zstd_dec_ref).  write 0:
// count (frm only); 1: also one ZdxBlk per block at place[i].
__global__ __launch_bounds__(256) void rcdc_zdx_blocks_kernel(
    const uint8_t *__restrict__ frames, const ulonglong4 *__restrict__ refs, uint32_t n,
    uint32_t write, uint32_t all_in_order, const ZdxPlace *__restrict__ place, ZdxLayout lay,
    uint8_t *ws, ZdxFrame *__restrict__ frm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ulonglong4 r = refs[i];
    const uint8_t *f = frames + r.x, *end = f + r.y;
    const Span blks = region(ws, lay.blk_off, lay.blk_cap);
    ZdxPlace pl;
    pl.blk0 = pl.data0 = 0;
    if (write) pl = place[i];
    ZdxFrame F;
    memset(&F, 0, sizeof F);
    uint32_t st = kDxOk;
    do {
        if (r.y < 6) { st = kDxBad; break; }
        const uint32_t magic = f[0] | (f[1] << 8) | (f[2] << 16) | ((uint32_t)f[3] << 24);
        const uint32_t fhd = f[4];
        if (magic != 0xFD2FB528u || (fhd & 8u)) { st = kDxBad; break; }
        const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, cksum = (fhd >> 2) & 1u,
                       did_flag = fhd & 3u;
        const uint8_t *q = f + 5 + (single ? 0 : 1);
        const uint32_t did_len = did_flag == 0 ? 0 : did_flag == 1 ? 1 : did_flag == 2 ? 2 : 4;
        const uint32_t fcs_len = fcs_flag == 0 ? (single ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
        if (q + did_len + fcs_len > end) { st = kDxBad; break; }
        uint32_t did = 0;
        for (uint32_t j = 0; j < did_len; j++) did |= (uint32_t)q[j] << (8 * j);
        if (did) { st = kDxBad; break; }  // dictionaries: not supported
        q += did_len;
        uint64_t fcs = 0;
        for (uint32_t j = 0; j < fcs_len; j++) fcs |= (uint64_t)q[j] << (8 * j);
        if (fcs_len == 2) fcs += 256;
        q += fcs_len;
        const bool shortcut = fcs_len && fcs <= kDecodeAllFirstOut;
        const uint64_t W = window_size(single, single ? 0u : f[5], fcs);
        if (!shortcut && W > (1ull << 27) + 1ull) { st = kDxBad; break; }
        F.fcs = fcs;
        F.flags = (fcs_len ? kZdxHasFcs : 0u) | (cksum ? kZdxChecksum : 0u) |
                  (all_in_order ? kZdxInOrder : 0u);
        if (fcs_len && fcs > r.w) { st = kDxFull; break; }
        F.bmax = shortcut ? kBlockMax : (uint32_t)min(W, (uint64_t)kBlockMax);
        F.wlim = shortcut ? ~0u : (uint32_t)W;
        uint32_t tree = kZdxNoTree;
        uint64_t k = 0, cursor = 0;
        for (;;) {
            if (q + 3 > end) { st = kDxBad; break; }
            const uint32_t bh = q[0] | (q[1] << 8) | ((uint32_t)q[2] << 16);
            q += 3;
            const uint32_t last = bh & 1u, btype = (bh >> 1) & 3u, bsize = bh >> 3;
            const uint64_t csz = btype == 1 ? 1u : bsize;
            if (btype == 3 || bsize > F.bmax || q + csz > end) { st = kDxBad; break; }
            ZdxBlk d;
            memset(&d, 0, sizeof d);
            d.content = r.x + (uint64_t)(q - f);
            d.size = bsize;
            d.type = btype;
            d.tree = kZdxNoTree;
            d.frame = i;
            if (btype == 2 && bsize == 0 && !shortcut) {
                // the stage machine skips empty blocks of any type; the
                // one-pass path calls an empty compressed block corrupt
                d.type = 0;
            } else if (btype == 2) {
                if (bsize < 3) { st = kDxBad; break; }  // libzstd's MIN_CBLOCK_SIZE
                LitHdr h;
                if (!lit_header(q, bsize, h)) { st = kDxBad; break; }
                const uint8_t *bend = q + bsize;
                const uint8_t *s = q + h.hdr + (h.ltype == 0 ? h.regen : h.ltype == 1 ? 1u : h.csize);
                uint32_t nseq = 0;
                const uint32_t cb = seq_count(s, bend, &nseq);
                if (!cb || nseq > kSeqMax) { st = kDxBad; break; }
                s += cb;
                if (nseq) {
                    if (s >= bend) { st = kDxBad; break; }
                    const uint32_t modes = s[0];
                    if (modes & 3u) { st = kDxBad; break; }  // reserved bits (RFC 8878 3.1.1.3.2.1)
                    if ((modes >> 6) == 3u || ((modes >> 4) & 3u) == 3u || ((modes >> 2) & 3u) == 3u)
                        F.flags |= kZdxInOrder;  // a repeat-mode table
                }
                if (h.ltype == 3) {
                    if (tree == kZdxNoTree) {
                        F.flags |= kZdxInOrder;  // (which calls it corrupt)
                    } else {
                        d.tree = tree;
                        F.ntreeless++;
                    }
                } else if (h.ltype == 2) {
                    tree = (uint32_t)(pl.blk0 + k);
                }
                d.regen = h.regen;
                d.nseq = nseq;
                d.lit_off = pl.data0 + cursor;
                d.seq_off = d.lit_off + ((h.regen + 15u) & ~15u);
                cursor += ((h.regen + 15u) & ~15u) + 8ull * nseq;
                F.ncomp++;
            }
            if (write) {
                uint8_t *slot = span_at(blks, (pl.blk0 + k) * sizeof(ZdxBlk), sizeof(ZdxBlk));
                if (!slot) { st = kDxBad; break; }
                *reinterpret_cast<ZdxBlk *>(slot) = d;
            }
            q += csz;
            k++;
            if (k >= 0xFFFFFFFFull) { st = kDxBad; break; }
            if (last) break;
        }
        F.nblk = (uint32_t)k;
        F.need = cursor;
        if (st) break;
        if (cksum) q += 4;
        if (q != end) st = kDxBad;  // cut off, a second frame or trailing bytes
    } while (false);
    F.status = st;
    frm[i] = F;
}

namespace {

// ---- the entropy stage ---------------------------------------------------------

// What the in-order pass carries from block to block (the tables themselves
// stay in the wave's LDS); the parallel pass starts every block with none.
struct EState {
    uint32_t huf_log;  // 0: no Huffman table yet
    uint32_t huf_nw;   // its weights in L.w[0 .. huf_nw)
    uint32_t al_ll, al_of, al_ml;  // 255: no table yet
};
__device__ __forceinline__ void estate_reset(EState &S) {
    S.huf_log = 0;
    S.huf_nw = 0;
    S.al_ll = S.al_of = S.al_ml = 255u;
}

// Compressed block b: its literals and sequence records into its slot of the
// data region, its verdict into res.  Returns the status (0 or 2).
__device__ uint32_t entropy_block(DxLds &L, EState &S, const uint8_t *frames, const ZdxBlk &b,
                                  const Span &blks, const Span &data, uint32_t bmax, ZdxRes *res,
                                  uint32_t lane) {
    const uint8_t *p = frames + b.content;
    const uint32_t bs = b.size;
    const uint8_t *end = p + bs;
    LitHdr h;
    // (the header walk accepted it: the same bytes give the same answer)
    if (bs < 3 || !lit_header(p, bs, h) || h.regen != b.regen) return kDxBad;
    const uint32_t regen = h.regen;
    uint8_t *lits = span_at(data, b.lit_off, (regen + 15u) & ~15u);
    uint64_t *recs = reinterpret_cast<uint64_t *>(span_at(data, b.seq_off, 8ull * b.nseq));
    if (!lits || !recs || (b.seq_off & 7u)) return kDxBad;
    const uint8_t *q = p + h.hdr;
    if (h.ltype == 0) {
        wave_copy(lits, q, regen, lane);
        q += regen;
    } else if (h.ltype == 1) {
        wave_fill(lits, q[0], regen, lane);
        q += 1;
    } else {
        const uint8_t *cs = q;
        int64_t clen = h.csize;
        if (h.ltype == 2) {
            uint32_t nw = 0;
            const int tu = read_huf_weights(cs, clen, L, &nw, lane);
            if (tu < 0) return kDxBad;
            S.huf_log = build_huf(L, nw, lane);
            S.huf_nw = nw;
            cs += tu;
            clen -= tu;
        } else if (S.huf_log != 0) {  // treeless, in order: the weights are still in L.w
            build_huf(L, S.huf_nw, lane);
        } else {
            // treeless, on its own: the tree of the block the header walk
            // recorded, read from that block's bytes
            if (b.tree == kZdxNoTree) return kDxBad;
            const uint8_t *ts = span_at(blks, (uint64_t)b.tree * sizeof(ZdxBlk), sizeof(ZdxBlk));
            if (!ts) return kDxBad;
            const ZdxBlk tb = *reinterpret_cast<const ZdxBlk *>(ts);
            LitHdr th;
            if (tb.type != 2 || tb.frame != b.frame || tb.size < 3 ||
                !lit_header(frames + tb.content, tb.size, th) || th.ltype != 2)
                return kDxBad;
            uint32_t nw = 0;
            if (read_huf_weights(frames + tb.content + th.hdr, th.csize, L, &nw, lane) < 0) return kDxBad;
            S.huf_log = build_huf(L, nw, lane);
            S.huf_nw = nw;
        }
        const uint32_t tl = S.huf_log;
        bool ok = true;
        if (h.nstreams == 1) {
            if (lane == 0) ok = huf_stream(L, tl, cs, clen, lits, regen);
        } else {
            if (clen < 6) return kDxBad;
            const int64_t s1 = cs[0] | (cs[1] << 8), s2 = cs[2] | (cs[3] << 8), s3 = cs[4] | (cs[5] << 8);
            const int64_t s4 = clen - 6 - s1 - s2 - s3;
            const uint32_t seg = (regen + 3) / 4;
            if (s4 < 0 || 3 * seg > regen) return kDxBad;
            if (lane < 4) {
                const int64_t off = 6 + (lane > 0 ? s1 : 0) + (lane > 1 ? s2 : 0) + (lane > 2 ? s3 : 0);
                const int64_t ln = lane == 0 ? s1 : lane == 1 ? s2 : lane == 2 ? s3 : s4;
                const uint32_t nn = lane < 3 ? seg : regen - 3 * seg;
                ok = huf_stream(L, tl, cs + off, ln, lits + lane * seg, nn);
            }
        }
        if (__builtin_amdgcn_ballot_w64(!ok)) return kDxBad;
        wsync();
        q += h.csize;
    }
    // -- sequences section
    if (q >= end) return kDxBad;
    uint32_t nseq = 0;
    const uint32_t cb = seq_count(q, end, &nseq);
    if (!cb || nseq != b.nseq) return kDxBad;
    q += cb;
    nseq = rfl(nseq);
    uint32_t sum_ll = 0, sum_ml = 0;  // per lane, over its sequences
    if (nseq) {
        if (q >= end) return kDxBad;
        const uint32_t modes = *q++;
        if (modes & 3u) return kDxBad;
        for (int k = 0; k < 3; k++) {  // tables in the order LL, OF, ML
            const uint32_t mode = (modes >> (6 - 2 * k)) & 3u;
            FseD *t = k == 0 ? L.ll : k == 1 ? L.of : L.ml;
            uint32_t &al = k == 0 ? S.al_ll : k == 1 ? S.al_of : S.al_ml;
            const uint32_t max_sym = k == 0 ? 35u : k == 1 ? 31u : 52u;
            const uint32_t max_al = k == 0 ? 9u : k == 1 ? 8u : 9u;
            if (mode == 0) {
                const int16_t *nrm = k == 0 ? kLLNorm : k == 1 ? kOFNorm : kMLNorm;
                const uint32_t ns = k == 0 ? 36u : k == 1 ? 29u : 53u;
                const uint32_t a = k == 1 ? 5u : 6u;
                if (!build_predefined(t, nrm, ns, a, L.norm, L.nxt, lane)) return kDxBad;
                al = a;
            } else if (mode == 1) {
                if (q >= end) return kDxBad;
                const uint32_t s = *q++;
                if (s > max_sym) return kDxBad;
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
                if (u < 0) return kDxBad;
                wsync();
                if (!build_fse(t, L.norm, ns, a, L.nxt, lane)) return kDxBad;
                al = a;
                q += u;
            } else if (al == 255u) {  // repeat: needs an earlier table
                return kDxBad;
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
        BRevQ r;
        r.pf = (__attribute__((address_space(3))) uint32_t *)L.pf;
        if (!brq_init<true>(r, q, end - q)) return kDxBad;
        const uint32_t al_ll = rfl(S.al_ll), al_of = rfl(S.al_of), al_ml = rfl(S.al_ml);
        // (states masked to their tables: a table's entries keep every state
        // inside it, the masks make that independent of the frame's bytes)
        const uint32_t mll = (1u << al_ll) - 1u, mof = (1u << al_of) - 1u, mml = (1u << al_ml) - 1u;
        uint32_t sll = brq_bits<true>(r, al_ll);
        uint32_t sof = brq_bits<true>(r, al_of);
        uint32_t sml = brq_bits<true>(r, al_ml);
        for (uint32_t s0 = 0; s0 < nseq; s0 += 64) {
            const uint32_t nb = min(64u, nseq - s0);
            uint32_t myll = 0, myml = 3, myofv = 0;
            // the decode state is wave-uniform: say so each round
            r.pos = (int32_t)rfl((uint32_t)r.pos);
            r.B = (int32_t)rfl((uint32_t)r.B);
            r.acc = rfl64(r.acc);
            r.used = rfl(r.used);
            r.len = (int32_t)rfl((uint32_t)r.len);
            r.base = reinterpret_cast<const uint8_t *>(rfl64(reinterpret_cast<uintptr_t>(r.base)));
            r.g0 = make_uint4(rfl(r.g0.x), rfl(r.g0.y), rfl(r.g0.z), rfl(r.g0.w));
            r.nbyte = (int32_t)rfl((uint32_t)r.nbyte);
            sll = rfl(sll);
            sof = rfl(sof);
            sml = rfl(sml);
            for (uint32_t j = 0; j < nb; j++) {
                const uint32_t veo = reinterpret_cast<const uint32_t *>(L.of)[sof & mof];
                const uint32_t vel = reinterpret_cast<const uint32_t *>(L.ll)[sll & mll];
                const uint32_t vem = reinterpret_cast<const uint32_t *>(L.ml)[sml & mml];
                const uint32_t vxl = L.u.x.llx[sll & mll], vxm = L.u.x.mlx[sml & mml];
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t eo = rfl(veo), el = rfl(vel), em = rfl(vem);
                const uint32_t xl = rfl(vxl), xm = rfl(vxm);
                const uint32_t ofc = eo & 31u;
                const uint64_t ofv = (1ull << ofc) + brq_bits<true>(r, ofc);
                const uint32_t nm = xm >> 24, nl = xl >> 24;  // <= 16 each
                const uint32_t vx = brq_bits<true>(r, nm + nl);
                const uint32_t ml = (xm & 0xFFFFFFu) + (uint32_t)((uint64_t)vx >> nl);
                const uint32_t ll = (xl & 0xFFFFFFu) + (vx & (uint32_t)((1ull << nl) - 1ull));
                if (s0 + j + 1 < nseq) {
                    // the three state updates (<= 9 + 9 + 8 bits) in one read
                    const uint32_t bl = (el >> 8) & 15u, bm = (em >> 8) & 15u, bo = (eo >> 8) & 15u;
                    const uint32_t v = brq_bits<true>(r, min(bl + bm + bo, 32u));
                    sll = (el >> 16) + (uint32_t)((uint64_t)v >> (bm + bo));
                    sml = (em >> 16) + ((v >> bo) & ((1u << bm) - 1u));
                    sof = (eo >> 16) + (v & ((1u << bo) - 1u));
                }
                const bool me = lane == j;
                myll = me ? ll : myll;
                myml = me ? ml : myml;
                myofv = me ? (uint32_t)min(ofv, (uint64_t)kZdxOfvMax) : myofv;
            }
            if (r.pos < 0) return kDxBad;
            if (lane < nb) {
                // ll <= 131071, ml - 3 <= 131071: 17 bits each
                recs[s0 + lane] = (uint64_t)(myll & 0x1FFFFu) |
                                  (uint64_t)((myml - 3u) & 0x1FFFFu) << kZdxRecMlShift |
                                  (uint64_t)myofv << kZdxRecOfShift;
                sum_ll += myll;
                sum_ml += myml;
            }
        }
        if (r.pos != 0) return kDxBad;  // bits left over (the RFC; libzstd 1.4.8 is lax)
    } else if (q != end) {
        return kDxBad;
    }
    // per lane at most 683 sequences of < 2^18 each: the sums fit 32 bits;
    // the wave's totals in 64
    uint64_t tl_ = sum_ll, tm_ = sum_ml;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        tl_ += __shfl_xor(tl_, d);
        tm_ += __shfl_xor(tm_, d);
    }
    if (tl_ > regen || regen + tm_ > bmax) return kDxBad;
    if (lane == 0) {
        res->lit_used = (uint32_t)tl_;
        res->regen = (uint32_t)(regen + tm_);
    }
    return kDxOk;
}

}  // namespace

// The parallel stage: a wave per compressed block of the frames the header
// walk passed and did not flag, from the queue counter ctr (zeroed by the host).
template <int OCC>
__global__ __launch_bounds__(64, OCC) void rcdc_zdx_entropy_kernel(
    const uint8_t *__restrict__ frames, const ZdxFrame *__restrict__ frm, ZdxLayout lay, uint8_t *ws,
    uint64_t nblk, uint32_t *ctr) {
    __shared__ DxLds L;
    const uint32_t lane = threadIdx.x;
    const Span blks = region(ws, lay.blk_off, lay.blk_cap);
    const Span ress = region(ws, lay.res_off, lay.res_cap);
    const Span data = region(ws, lay.data_off, lay.data_cap);
    for (;;) {
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(ctr, 1u);
        k = rfl(__shfl(k, 0));
        if (k >= nblk) break;
        const uint8_t *bp = span_at(blks, (uint64_t)k * sizeof(ZdxBlk), sizeof(ZdxBlk));
        uint8_t *rp = span_at(ress, (uint64_t)k * sizeof(ZdxRes), sizeof(ZdxRes));
        if (!bp || !rp) break;
        const ZdxBlk b = *reinterpret_cast<const ZdxBlk *>(bp);
        if (b.type != 2) continue;
        const ZdxFrame F = frm[b.frame];
        if (F.status != kDxOk || (F.flags & kZdxInOrder)) continue;
        EState S;
        estate_reset(S);
        ZdxRes *res = reinterpret_cast<ZdxRes *>(rp);
        const uint32_t st = entropy_block(L, S, frames, b, blks, data, F.bmax, res, lane);
        if (lane == 0) res->status = st;
        __syncthreads();  // LDS tables are rebuilt by the next block
    }
}

// The in-order entropy pass: a wave per flagged frame of list[0, nlist).
template <int OCC>
__global__ __launch_bounds__(64, OCC) void rcdc_zdx_inorder_kernel(
    const uint8_t *__restrict__ frames, const ZdxFrame *__restrict__ frm,
    const ZdxPlace *__restrict__ place, const uint32_t *__restrict__ list, uint32_t nlist,
    ZdxLayout lay, uint8_t *ws, uint32_t *ctr) {
    __shared__ DxLds L;
    const uint32_t lane = threadIdx.x;
    const Span blks = region(ws, lay.blk_off, lay.blk_cap);
    const Span ress = region(ws, lay.res_off, lay.res_cap);
    const Span data = region(ws, lay.data_off, lay.data_cap);
    for (;;) {
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(ctr, 1u);
        k = rfl(__shfl(k, 0));
        if (k >= nlist) break;
        const uint32_t i = list[k];
        const ZdxFrame F = frm[i];
        if (F.status != kDxOk) continue;
        const uint64_t b0 = place[i].blk0;
        EState S;
        estate_reset(S);
        for (uint32_t j = 0; j < F.nblk; j++) {
            const uint8_t *bp = span_at(blks, (b0 + j) * sizeof(ZdxBlk), sizeof(ZdxBlk));
            uint8_t *rp = span_at(ress, (b0 + j) * sizeof(ZdxRes), sizeof(ZdxRes));
            if (!bp || !rp) break;
            const ZdxBlk b = *reinterpret_cast<const ZdxBlk *>(bp);
            if (b.type != 2) continue;
            ZdxRes *res = reinterpret_cast<ZdxRes *>(rp);
            const uint32_t st = entropy_block(L, S, frames, b, blks, data, F.bmax, res, lane);
            if (lane == 0) res->status = st;
            __syncthreads();
            if (st != kDxOk) break;  // (the copy stops at this block too)
        }
        __syncthreads();
    }
}

namespace {

// ---- XXH64 (a frame's Content_Checksum: its low 32 bits, seed 0) -------------
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
        for (; s + 4 <= stripes; s += 4, p += 128) {
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
    auto le = [&](uint64_t at, uint32_t nb) {
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

// ---- the copy stage ------------------------------------------------------------

constexpr uint32_t kShort = 32;  // a lane copies up to this many bytes itself

struct CopyLds {
    uint32_t ms[64], me[64];  // the batch's matches: start and end, from the batch's start
};

// number of v[0, 64) (ascending) that are < x (strict) or <= x
__device__ __forceinline__ uint32_t count_below(const uint32_t *v, uint32_t x, bool strict) {
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1) {
        const uint32_t y = v[lo + step - 1];
        if (strict ? y < x : y <= x) lo += step;
    }
    const uint32_t y = v[lo < 64 ? lo : 63];
    if (lo < 64 && (strict ? y < x : y <= x)) lo++;
    return lo;
}

// One frame's copy state.
struct Cp {
    Span out;        // [out_off, out_off + out_cap) of d_out
    uint64_t pos;    // bytes written
    uint64_t fcs;    // declared content size, ~0: none
    uint32_t wlim, bmax;
    uint32_t r0, r1, r2;
};

// Room for n more bytes: 0, or the status that ends the frame (past the
// declared size: malformed; past out_cap: 1).
__device__ __forceinline__ uint32_t room(const Cp &C, uint64_t n) {
    if (C.pos + n > C.fcs) return kDxBad;
    if (C.pos + n > C.out.cap) return kDxFull;
    return kDxOk;
}

// The sequences of compressed block b executed at C.pos.
__device__ uint32_t copy_compressed(Cp &C, CopyLds &M, const ZdxBlk &b, const ZdxRes &res,
                                    const Span &data, uint32_t lane) {
    if (res.status != kDxOk) return kDxBad;
    if (res.lit_used > b.regen || res.regen > C.bmax) return kDxBad;
    const uint8_t *lits = span_at(data, b.lit_off, (b.regen + 15u) & ~15u);
    const uint64_t *recs = reinterpret_cast<const uint64_t *>(span_at(data, b.seq_off, 8ull * b.nseq));
    if (!lits || !recs) return kDxBad;
    const uint64_t pos0 = C.pos;
    const uint32_t nseq = rfl(b.nseq);  // (wave-uniform: every lane loaded the same descriptor)
    uint64_t litpos = 0;
    for (uint32_t s0 = 0; s0 < nseq; s0 += 64) {
        const uint32_t nb = min(64u, nseq - s0);
        const bool mine = lane < nb;
        uint32_t ll = 0, ml = 0, ofv = 4;
        if (mine) {
            const uint64_t rec = recs[s0 + lane];
            ll = (uint32_t)rec & 0x1FFFFu;
            ml = ((uint32_t)(rec >> kZdxRecMlShift) & 0x1FFFFu) + 3u;
            ofv = (uint32_t)(rec >> kZdxRecOfShift);
        }
        // -- repeat offsets, in order (RFC 8878 3.1.1.5)
        uint32_t off = ofv - 3u;
        uint32_t r0 = rfl(C.r0), r1 = rfl(C.r1), r2 = rfl(C.r2);
        const bool anyrep = __builtin_amdgcn_ballot_w64(mine && ofv <= 3u) != 0;
        bool zero = false;
        if (!anyrep && nb >= 3) {
            r0 = (uint32_t)__shfl((int)off, (int)nb - 1);
            r1 = (uint32_t)__shfl((int)off, (int)nb - 2);
            r2 = (uint32_t)__shfl((int)off, (int)nb - 3);
        } else {
            for (uint32_t j = 0; j < nb; j++) {
                const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)ofv, (int)j);
                const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)ll, (int)j);
                const bool lr = v <= 3u;  // a repeat code
                const uint32_t idx = v - 1u + (l == 0 ? 1u : 0u);
                const uint32_t rsel = idx == 1 ? r1 : idx == 2 ? r2 : idx == 0 ? r0 : r0 - 1u;
                const uint32_t o = lr ? rsel : v - 3u;
                const bool k1 = lr && idx == 0, k2 = lr && idx <= 1;  // r1 / r2 kept
                const uint32_t n2 = k2 ? r2 : r1, n1 = k1 ? r1 : r0;
                r2 = n2;
                r1 = n1;
                r0 = o;
                zero |= o == 0;
                off = lane == j ? o : off;
            }
        }
        if (zero) return kDxBad;  // rep[0] - 1 == 0
        C.r0 = r0;
        C.r1 = r1;
        C.r2 = r2;
        // -- place the batch
        uint64_t incl_l = ll, incl_o = (uint64_t)ll + ml;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t a = __shfl_up(incl_l, d), c = __shfl_up(incl_o, d);
            if (lane >= d) {
                incl_l += a;
                incl_o += c;
            }
        }
        const uint64_t tot_l = __shfl(incl_l, (int)nb - 1), tot_o = __shfl(incl_o, (int)nb - 1);
        if (litpos + tot_l > b.regen) return kDxBad;                  // more literals than decoded
        if (C.pos - pos0 + tot_o > C.bmax) return kDxBad;             // Block_Maximum_Size
        if (const uint32_t st = room(C, tot_o)) return st;
        uint8_t *base = span_at(C.out, C.pos, tot_o);
        if (!base) return kDxFull;
        const uint64_t lp = litpos + incl_l - ll;        // my literals
        const uint64_t rel = incl_o - ll - ml;           // my literals' place in the batch
        const uint64_t mp = C.pos + rel + ll;            // my match: bytes regenerated before it
        if (__builtin_amdgcn_ballot_w64(mine && (off == 0 || off > mp || off > C.wlim))) return kDxBad;
        // -- literals: from the workspace, no order
        if (mine && ll <= kShort) {
            uint8_t *d = base + rel;
            const auto *s = gptr(lits + lp);
            for (uint32_t i = 0; i < ll; i++) d[i] = s[i];
        }
        uint64_t longs = __builtin_amdgcn_ballot_w64(mine && ll > kShort);
        while (longs) {
            const int j = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint64_t r_ = __shfl(rel, j), l_ = __shfl(lp, j);
            const uint32_t n_ = (uint32_t)__shfl((int)ll, j);
            wave_copy(base + r_, lits + l_, n_, lane);
        }
        wsync();
        // -- matches, in dependency order.  A match's source [a, e) (its first
        // min(off, ml) bytes: the rest repeats them) may hold bytes that
        // earlier matches of this batch write; those matches are a run of
        // lanes [lo, hi), found in the batch's sorted match ranges.
        M.ms[lane] = mine ? (uint32_t)(rel + ll) : 0xFFFFFFFFu;
        M.me[lane] = mine ? (uint32_t)(rel + ll + ml) : 0xFFFFFFFFu;
        wsync();
        uint64_t dep = 0;
        if (mine) {
            const int64_t a = (int64_t)(rel + ll) - (int64_t)off;
            const int64_t e = a + (int64_t)min(off, ml);
            if (e > 0) {
                const uint32_t lo = count_below(M.me, (uint32_t)max(a, (int64_t)0), false);
                const uint32_t hi = min(count_below(M.ms, (uint32_t)e, true), lane);
                if (hi > lo) dep = ((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
            }
        }
        uint64_t done = nb == 64 ? 0ull : ~0ull << nb;
        for (uint32_t round = 0; round < 64 && done != ~0ull; round++) {
            const bool ready = !((done >> lane) & 1ull) && (dep & ~done) == 0;
            uint8_t *d = base + rel + ll;
            if (ready && ml <= kShort) {
                const auto *s = gptr((const uint8_t *)d - off);
                uint32_t ph = 0;
                for (uint32_t i = 0; i < ml; i++) {
                    d[i] = s[ph];
                    ph = ph + 1 == off ? 0 : ph + 1;
                }
            }
            uint64_t lm = __builtin_amdgcn_ballot_w64(ready && ml > kShort);
            while (lm) {
                const int j = __builtin_ctzll(lm);
                lm &= lm - 1;
                const uint64_t d_ = __shfl(rel + ll, j);
                const uint32_t o_ = (uint32_t)__shfl((int)off, j), n_ = (uint32_t)__shfl((int)ml, j);
                wave_match(base + d_, o_, n_, lane);
            }
            done |= __builtin_amdgcn_ballot_w64(ready);
            wsync();
        }
        if (done != ~0ull) return kDxBad;  // (cannot happen: the lowest open lane is always ready)
        litpos += tot_l;
        C.pos += tot_o;
    }
    // the remaining literals
    const uint64_t rest = b.regen - litpos;
    if (C.pos - pos0 + rest > C.bmax) return kDxBad;
    if (const uint32_t st = room(C, rest)) return st;
    uint8_t *d = span_at(C.out, C.pos, rest);
    if (!d) return kDxFull;
    wave_copy(d, lits + litpos, rest, lane);
    C.pos += rest;
    wsync();
    return kDxOk;
}

}  // namespace

// A wave per frame of order[0, nlist) (longest first), blocks in order.
__global__ __launch_bounds__(64) void rcdc_zdx_copy_kernel(
    const uint8_t *__restrict__ frames, const ulonglong4 *__restrict__ refs,
    const ZdxFrame *__restrict__ frm, const ZdxPlace *__restrict__ place,
    const uint32_t *__restrict__ order, uint32_t nlist, ZdxLayout lay, uint8_t *ws, uint8_t *d_out,
    uint64_t *__restrict__ out_lens, uint32_t *__restrict__ status, uint32_t *ctr) {
    __shared__ CopyLds M;
    const uint32_t lane = threadIdx.x;
    const Span blks = region(ws, lay.blk_off, lay.blk_cap);
    const Span ress = region(ws, lay.res_off, lay.res_cap);
    const Span data = region(ws, lay.data_off, lay.data_cap);
    for (;;) {
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(ctr, 1u);
        k = rfl(__shfl(k, 0));
        if (k >= nlist) break;
        const uint32_t i = order[k];
        const ulonglong4 r = refs[i];
        const ZdxFrame F = frm[i];
        uint32_t st = F.status;
        Cp C;
        C.out.base = d_out + r.z;
        C.out.cap = r.w;
        C.pos = 0;
        C.fcs = (F.flags & kZdxHasFcs) ? F.fcs : ~0ull;
        C.wlim = F.wlim;
        C.bmax = F.bmax;
        C.r0 = 1;
        C.r1 = 4;
        C.r2 = 8;
        const uint64_t b0 = place[i].blk0;
        const uint32_t nblk = rfl(F.nblk);
        for (uint32_t j = 0; st == kDxOk && j < nblk; j++) {
            const uint8_t *bp = span_at(blks, (b0 + j) * sizeof(ZdxBlk), sizeof(ZdxBlk));
            const uint8_t *rp = span_at(ress, (b0 + j) * sizeof(ZdxRes), sizeof(ZdxRes));
            if (!bp || !rp) { st = kDxBad; break; }
            const ZdxBlk b = *reinterpret_cast<const ZdxBlk *>(bp);
            if (b.type == 2) {
                const ZdxRes res = *reinterpret_cast<const ZdxRes *>(rp);
                st = copy_compressed(C, M, b, res, data, lane);
            } else if (b.size) {
                // (the header walk held size to Block_Maximum_Size and, for a
                // raw block, its bytes to the frame)
                if ((st = room(C, b.size)) != kDxOk) break;
                uint8_t *d = span_at(C.out, C.pos, b.size);
                if (!d) { st = kDxFull; break; }
                if (b.type == 0)
                    wave_copy(d, frames + b.content, b.size, lane);
                else
                    wave_fill(d, frames[b.content], b.size, lane);
                C.pos += b.size;
                wsync();
            }
        }
        if (st == kDxOk && C.fcs != ~0ull && C.pos != C.fcs) st = kDxBad;
        if (st == kDxOk && (F.flags & kZdxChecksum)) {
            const uint8_t *c = frames + r.x + r.y - 4;  // (the walk: the frame ends with it)
            const uint32_t want = c[0] | (c[1] << 8) | (c[2] << 16) | ((uint32_t)c[3] << 24);
            if (xxh64_low32(C.out.base, C.pos, lane) != want) st = kDxBad;
        }
        if (lane == 0) {
            status[i] = st;
            out_lens[i] = st == kDxOk ? C.pos : 0;
        }
        __syncthreads();
    }
}

namespace rcdc {

// waves per CU the entropy grids are sized for (128 VGPRs, 9984 B of LDS)
uint32_t zdx_waves_per_cu() { return 16u; }

hipError_t launch_zdx_blocks(const uint8_t *frames, const void *refs, uint32_t n, bool write,
                             bool all_in_order, const ZdxPlace *place, const ZdxLayout &lay,
                             uint8_t *ws, ZdxFrame *frm, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rcdc_zdx_blocks_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, frames,
                       (const ulonglong4 *)refs, n, write ? 1u : 0u, all_in_order ? 1u : 0u, place,
                       lay, ws, frm);
    return hipGetLastError();
}

hipError_t launch_zdx_entropy(const uint8_t *frames, const ZdxFrame *frm, const ZdxLayout &lay,
                              uint8_t *ws, uint64_t nblk, uint32_t grid, uint32_t *ctr,
                              hipStream_t stream) {
    if (nblk == 0) return hipSuccess;
    const uint32_t g = nblk < grid ? (uint32_t)nblk : grid;
    hipLaunchKernelGGL(rcdc_zdx_entropy_kernel<4>, dim3(g), dim3(64), 0, stream, frames, frm, lay, ws,
                       nblk, ctr);
    return hipGetLastError();
}

hipError_t launch_zdx_inorder(const uint8_t *frames, const ZdxFrame *frm, const ZdxPlace *place,
                              const uint32_t *list, uint32_t nlist, const ZdxLayout &lay, uint8_t *ws,
                              uint32_t grid, uint32_t *ctr, hipStream_t stream) {
    if (nlist == 0) return hipSuccess;
    const uint32_t g = nlist < grid ? nlist : grid;
    hipLaunchKernelGGL(rcdc_zdx_inorder_kernel<4>, dim3(g), dim3(64), 0, stream, frames, frm, place,
                       list, nlist, lay, ws, ctr);
    return hipGetLastError();
}

hipError_t launch_zdx_copy(const uint8_t *frames, const void *refs, const ZdxFrame *frm,
                           const ZdxPlace *place, const uint32_t *order, uint32_t nlist,
                           const ZdxLayout &lay, uint8_t *ws, uint8_t *d_out, uint64_t *out_lens,
                           uint32_t *status, uint32_t grid, uint32_t *ctr, hipStream_t stream) {
    if (nlist == 0) return hipSuccess;
    const uint32_t g = nlist < grid ? nlist : grid;
    hipLaunchKernelGGL(rcdc_zdx_copy_kernel, dim3(g), dim3(64), 0, stream, frames,
                       (const ulonglong4 *)refs, frm, place, order, nlist, lay, ws, d_out, out_lens,
                       status, ctr);
    return hipGetLastError();
}

}  // namespace rcdc
