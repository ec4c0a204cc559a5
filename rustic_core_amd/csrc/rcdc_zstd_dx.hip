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
// checker's (rcdc_zstd_dec.hip).  From rcdc_zstd_bits.h, shared with the
// checker: the predefined tables, the LDS layout, the loads and bit readers,
// the FSE / Huffman table readers and builders, huf_stream, the section steps
// (lit_header, seq_count, huf_literals / huf_streams, seq_tables), frame_header
// and xxh64_low32.  Here: the bounded regions, the wave copies, the sequence
// decode loop that writes records, and the copy stage.  The two stay separate
// translation units.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rcdc_internal.h"
#include "rcdc_launch.h"
#include "rcdc_zstd_bits.h"

using namespace rcdc;

namespace {

constexpr uint32_t kDxOk = 0, kDxFull = 1, kDxBad = 2;
// every match is at least 3 bytes: more sequences cannot stay within a block
constexpr uint32_t kSeqMax = kBlockMax / 3u;

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
        FrameHdr H;
        if (!frame_header(f, r.y, H)) { st = kDxBad; break; }
        F.fcs = H.fcs;
        F.flags = (H.fcs_len ? kZdxHasFcs : 0u) | (H.cksum ? kZdxChecksum : 0u) |
                  (all_in_order ? kZdxInOrder : 0u);
        if (H.fcs_len && H.fcs > r.w) { st = kDxFull; break; }
        F.bmax = H.bmax;
        F.wlim = H.wlim;
        const uint8_t *q = f + H.len;
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
            if (btype == 2 && bsize == 0 && !H.shortcut) {
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
        if (H.cksum) q += 4;
        if (q != end) st = kDxBad;  // cut off, a second frame or trailing bytes
    } while (false);
    F.status = st;
    frm[i] = F;
}

namespace {

// ---- the entropy stage ---------------------------------------------------------

// (Tables: what the in-order pass carries from block to block; the parallel
// pass starts every block with none.)

// Compressed block b: its literals and sequence records into its slot of the
// data region, its verdict into res.  Returns the status (0 or 2).
__device__ uint32_t entropy_block(ZstdLds &L, Tables &S, const uint8_t *frames, const ZdxBlk &b,
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
        uint32_t st = huf_literals<true>(L, S, h, q, lits, lane);
        if (st == kSecNeedsTable) {
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
            S.huf_log = build_huf<true>(L, nw, lane);
            S.huf_nw = nw;
            st = huf_streams<true>(L, S.huf_log, h.nstreams, q, h.csize, lits, regen, lane);
        }
        if (st != kSecOk) return kDxBad;
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
        if (seq_tables(L, S, q, end, lane) != kSecOk) return kDxBad;  // (no table to repeat: bad)
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
    __shared__ ZstdLds L;
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
        Tables S;
        tables_reset(S);
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
    __shared__ ZstdLds L;
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
        Tables S;
        tables_reset(S);
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
