"""A strict RFC 8878 decoder that records structure -- test infrastructure,
plain Python, no GPU and no librcdc.so.

`dissect(frame)` decodes one frame and returns what it is made of: the header
form, every block's type and sizes, a compressed block's literals section
(type, header size class, Huffman weights and how they were coded, the four
stream sizes) and sequences section (the count and the byte form of its
header, the modes byte, every adaptive table's normalized counts and accuracy
log, the decoded (ll, ml, offset_value) list and the resolved offsets).  The
content is regenerated with tests/zstd_frames.py's `Content` history rules.

It is strict where libzstd 1.4.8 is lax: every Huffman and FSE bitstream must
be consumed exactly down to its end mark (the FSE-coded Huffman weights end by
running out, as the format defines), reserved bits must be 0, and a violation
raises DissectError naming the block and the field.  tests/
test_zstd_dissect_host.py holds it to the hand-built cases, libzstd's own
frames and tests/zstd_model.py's; tests/test_gpu_zstd_features.py dissects
what the device writes.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

from tests import zstd_frames as zf
from tests import zstd_model as zm

BLOCK = 128 << 10
LL_MAX_LOG, OF_MAX_LOG, ML_MAX_LOG = 9, 8, 9
_STREAM = {"ll": (35, LL_MAX_LOG), "of": (31, OF_MAX_LOG), "ml": (52, ML_MAX_LOG)}


class DissectError(ValueError):
    pass


def _fail(where, what):
    raise DissectError(f"{where}: {what}")


# ---- bit readers -----------------------------------------------------------------

class _Fwd:
    """Little-endian bits from the front (FSE table descriptions); bits past
    the end read as zeros and are refused when the description is done."""

    def __init__(self, data, where):
        self.d, self.pos, self.where = data, 0, where

    def read(self, n):
        i = self.pos >> 3
        v = (int.from_bytes(self.d[i:i + 5], "little") >> (self.pos & 7)) & ((1 << n) - 1)
        self.pos += n
        return v

    def bytes_used(self):
        if self.pos > 8 * len(self.d):
            _fail(self.where, "table description runs past its section")
        return (self.pos + 7) >> 3


class _Back:
    """A bitstream read from its end mark down.  `pos` counts the bits left
    below the read point; it goes negative when a read runs past the start
    (the missing low bits are zeros, as libzstd and the format define)."""

    def __init__(self, data, where):
        if not data:
            _fail(where, "empty bitstream")
        if data[-1] == 0:
            _fail(where, "no end mark in the bitstream's last byte")
        self.d, self.where = data, where
        self.pos = 8 * (len(data) - 1) + data[-1].bit_length() - 1

    def read(self, n):
        self.pos -= n
        p = self.pos
        if p >= 0:
            i = p >> 3
            return (int.from_bytes(self.d[i:i + 8], "little") >> (p & 7)) & ((1 << n) - 1)
        have = n + p
        if have <= 0:
            return 0
        return (int.from_bytes(self.d[:8], "little") & ((1 << have) - 1)) << -p & ((1 << n) - 1)

    def need(self, where, field):
        if self.pos < 0:
            _fail(where, f"{field} reads {-self.pos} bits past the bitstream's start")

    def done(self, where, field):
        if self.pos != 0:
            _fail(where, f"{field}: {self.pos} bits left above the bitstream's start" if self.pos > 0
                  else f"{field} reads {-self.pos} bits past the bitstream's start")


# ---- FSE (RFC 8878 4.1) ---------------------------------------------------------

def read_ncount(data, max_sym, max_log, where):
    """FSE table description -> (normalized counts, accuracy log, bytes)."""
    r = _Fwd(data, where)
    tl = r.read(4) + 5
    if tl > max_log:
        _fail(where, f"accuracy log {tl} above {max_log}")
    remaining, norm = 1 << tl, []
    while remaining > 0:
        if len(norm) > max_sym:
            _fail(where, f"more than {max_sym + 1} symbols")
        bits = (remaining + 1).bit_length()
        low_mask = (1 << (bits - 1)) - 1
        thresh = (1 << bits) - 1 - (remaining + 1)
        v = r.read(bits)
        if v & low_mask < thresh:  # a short value: bits - 1 bits
            r.pos -= 1
            v &= low_mask
        elif v > low_mask:
            v -= thresh
        prob = v - 1
        remaining -= abs(prob)
        if remaining < 0:
            _fail(where, "counts overshoot the table")
        norm.append(prob)
        if prob == 0:
            while True:
                rep = r.read(2)
                norm += [0] * rep
                if rep != 3:
                    break
    if len(norm) > max_sym + 1:
        _fail(where, f"more than {max_sym + 1} symbols")
    return norm, tl, r.bytes_used()


def fse_dtable(norm, tl):
    """[(symbol, bits, baseline)] per state (RFC 8878 4.1.1)."""
    size = 1 << tl
    sym_of, high = [0] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym_of[high] = s
            high -= 1
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym_of[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    nxt = [abs(c) for c in norm]
    tab = []
    for u in range(size):
        s = sym_of[u]
        x = nxt[s]
        nxt[s] += 1
        nb = tl - (x.bit_length() - 1)
        tab.append((s, nb, (x << nb) - size))
    return tab


# ---- Huffman (RFC 8878 4.2) -----------------------------------------------------

def _fse_weights(data, where):
    """FSE-compressed Huffman weights: two interleaved states until the stream
    runs out (4.2.1.2)."""
    norm, tl, used = read_ncount(data, 255, 6, where + " weights table")
    if used >= len(data):
        _fail(where, "no weights bitstream after its table description")
    tab = fse_dtable(norm, tl)
    b = _Back(data[used:], where + " weights bitstream")
    s1 = b.read(tl)
    s2 = b.read(tl)
    b.need(where, "weights initial states")
    out = []
    while True:
        if len(out) > 254:
            _fail(where, "more than 255 weights")
        sym, nb, base = tab[s1]
        out.append(sym)
        s1 = base + b.read(nb)
        if b.pos < 0:
            out.append(tab[s2][0])
            break
        sym, nb, base = tab[s2]
        out.append(sym)
        s2 = base + b.read(nb)
        if b.pos < 0:
            out.append(tab[s1][0])
            break
    return out, norm, tl


def huf_table(explicit, where):
    """Explicit weights -> NS(weights (all symbols), log, dec) where dec maps
    the next `log` bits to (symbol, code length)."""
    if any(w > 11 for w in explicit):
        _fail(where, f"Huffman weight {max(explicit)} above 11")
    total = sum(1 << (w - 1) for w in explicit if w)
    if total == 0:
        _fail(where, "Huffman weights are all zero")
    log = total.bit_length()
    if log > 11:
        _fail(where, f"Huffman table log {log} above 11")
    rest = (1 << log) - total
    if rest & (rest - 1):
        _fail(where, "Huffman weights leave no power of two for the last symbol")
    w = list(explicit) + [rest.bit_length()]
    ones = sum(1 for x in w if x == 1)
    if ones < 2 or ones & 1:
        _fail(where, "Huffman table without a pair of weight-1 symbols")
    dec = []
    for x in range(1, log + 1):
        for s, ws in enumerate(w):
            if ws == x:
                dec += [(s, log + 1 - x)] * (1 << (x - 1))
    assert len(dec) == 1 << log
    return NS(weights=w, log=log, dec=dec)


def _huf_stream(data, n, tab, where):
    b = _Back(data, where)
    d, log, dec = data, tab.log, tab.dec
    mask, m56 = (1 << log) - 1, (1 << 56) - 1
    rem = b.pos  # bits below the read point not yet in acc
    out = bytearray(n)
    acc = bits = 0  # the next `bits` bits of the stream, the first one highest
    for k in range(n):
        if bits < log and rem:
            if rem >= 56:
                rem -= 56
                i = rem >> 3
                acc = acc << 56 | ((int.from_bytes(d[i:i + 8], "little") >> (rem & 7)) & m56)
                bits += 56
            else:
                acc = acc << rem | (int.from_bytes(d[:7], "little") & ((1 << rem) - 1))
                bits += rem
                rem = 0
        # (the missing low bits of the stream's last code are zeros)
        sym, nb = dec[(acc >> (bits - log)) & mask if bits >= log else (acc << (log - bits)) & mask]
        out[k] = sym
        bits -= nb
        if bits < 0:
            _fail(where, f"literal {k} of {n} reads {-bits} bits past the stream's start")
        acc &= (1 << bits) - 1
    if bits or rem:
        _fail(where, f"{bits + rem} bits left above the stream's start after {n} literals")
    return out


# ---- sections -------------------------------------------------------------------

def _literals(blk, where, prev_huf):
    """-> (NS literals section, bytes used, literals, Huffman table or prev)."""
    if not blk:
        _fail(where, "no literals section")
    b0 = blk[0]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    where = where + " literals"
    if lt < 2:
        hl = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        if len(blk) < hl:
            _fail(where, "header truncated")
        n = int.from_bytes(blk[:hl], "little") >> (3 if hl == 1 else 4)
        end = hl + (n if lt == 0 else 1)
        if end > len(blk) or n > BLOCK:
            _fail(where, f"{n} literals do not fit the block")
        lits = bytes(blk[hl:end]) if lt == 0 else bytes([blk[hl]]) * n
        sec = NS(type=lt, size_format=sf, header_size=hl, regen=n, comp=end - hl, huf=None)
        return sec, end, lits, prev_huf
    hl, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    if len(blk) < hl:
        _fail(where, "header truncated")
    h = int.from_bytes(blk[:hl], "little")
    n, comp = (h >> 4) & ((1 << bits) - 1), (h >> (4 + bits)) & ((1 << bits) - 1)
    if hl + comp > len(blk) or n > BLOCK:
        _fail(where, f"compressed size {comp} does not fit the block")
    body = blk[hl:hl + comp]
    huf = NS(direct=None, fse_norm=None, fse_log=None, tree_bytes=0, streams=None)
    if lt == 2:
        if not body:
            _fail(where, "no Huffman tree description")
        hb = body[0]
        if hb >= 128:
            nw = hb - 127
            tb = 1 + (nw + 1) // 2
            if tb > len(body):
                _fail(where, "direct weights run past the section")
            wts = []
            for k in range(nw):
                x = body[1 + k // 2]
                wts.append(x >> 4 if k % 2 == 0 else x & 15)
            huf.direct = True
        else:
            tb = 1 + hb
            if hb == 0 or tb > len(body):
                _fail(where, "FSE-coded weights run past the section")
            wts, huf.fse_norm, huf.fse_log = _fse_weights(body[1:tb], where)
            huf.direct = False
        tab = huf_table(wts, where)
        huf.tree_bytes = tb
        body = body[tb:]
    else:
        if prev_huf is None:
            _fail(where, "treeless literals without an earlier Huffman table")
        tab = prev_huf
    huf.weights, huf.log = tab.weights, tab.log
    huf.streams_at = hl + comp - len(body) + (6 if sf else 0)  # in the block's content
    if sf == 0:
        huf.streams = [len(body)]
        lits = _huf_stream(body, n, tab, where + " stream 0")
    else:
        if len(body) < 6:
            _fail(where, "no jump table")
        s = [int.from_bytes(body[2 * k:2 * k + 2], "little") for k in range(3)]
        s.append(len(body) - 6 - sum(s))
        if s[3] < 1 or min(s) < 1:
            _fail(where, f"jump table {s[:3]} does not fit {len(body) - 6} stream bytes")
        huf.streams = s
        seg = (n + 3) // 4
        lits, q = bytearray(), 6
        for k in range(4):
            cnt = seg if k < 3 else n - 3 * seg
            if cnt < 0:
                _fail(where, f"{n} literals cannot fill four streams")
            lits += _huf_stream(body[q:q + s[k]], cnt, tab, where + f" stream {k}")
            q += s[k]
    sec = NS(type=lt, size_format=sf, header_size=hl, regen=n, comp=comp, huf=huf)
    return sec, hl + comp, bytes(lits), tab


def _predef(name):
    pn, tl = zm.PREDEF_NORM[name]
    return fse_dtable(pn, tl), tl


def _sequences(blk, where, prev_tabs):
    """-> (NS sequences section, tables for a later block's repeat mode)."""
    where = where + " sequences"
    if not blk:
        _fail(where, "no sequences section")
    s0 = blk[0]
    if s0 == 0:
        if len(blk) != 1:
            _fail(where, f"{len(blk) - 1} bytes after a count of 0")
        return NS(count=0, count_bytes=1, modes=None, tables={}, seqs=[], offsets=[]), prev_tabs
    if s0 < 128:
        k, q = s0, 1
    elif s0 < 255:
        if len(blk) < 2:
            _fail(where, "count truncated")
        k, q = ((s0 - 128) << 8) + blk[1], 2
    else:
        if len(blk) < 3:
            _fail(where, "count truncated")
        k, q = blk[1] + (blk[2] << 8) + 0x7F00, 3
    nb_hdr = q
    if q >= len(blk):
        _fail(where, "no modes byte")
    modes = blk[q]
    q += 1
    if modes & 3:
        _fail(where, f"reserved bits of the modes byte {modes:#04x} are set")
    tabs, rec = {}, {}
    for name, shift in (("ll", 6), ("of", 4), ("ml", 2)):
        mode = (modes >> shift) & 3
        max_sym, max_log = _STREAM[name]
        w = f"{where} {name} table"
        if mode == 0:
            tabs[name] = _predef(name)
            rec[name] = NS(mode=0, norm=None, log=tabs[name][1])
        elif mode == 1:
            if q >= len(blk):
                _fail(w, "RLE symbol missing")
            if blk[q] > max_sym:
                _fail(w, f"RLE symbol {blk[q]} above {max_sym}")
            tabs[name] = ([(blk[q], 0, 0)], 0)
            rec[name] = NS(mode=1, norm=None, log=0, symbol=blk[q])
            q += 1
        elif mode == 2:
            norm, tl, used = read_ncount(blk[q:], max_sym, max_log, w)
            tabs[name] = (fse_dtable(norm, tl), tl)
            rec[name] = NS(mode=2, norm=norm, log=tl)
            q += used
        else:
            if not prev_tabs or name not in prev_tabs:
                _fail(w, "repeat mode without an earlier table")
            tabs[name] = prev_tabs[name]
            rec[name] = NS(mode=3, norm=None, log=tabs[name][1])
    if q >= len(blk):
        _fail(where, "no bitstream")
    b = _Back(blk[q:], where + " bitstream")
    (tll, lll), (tof, lof), (tml, lml) = tabs["ll"], tabs["of"], tabs["ml"]
    sll, sof, sml = b.read(lll), b.read(lof), b.read(lml)
    b.need(where, "initial states")
    LLB, LLX, MLB, MLX = zf.LL_BASE, zf.LL_BITS, zf.ML_BASE, zf.ML_BITS
    seqs = []
    for i in range(k):
        llc, nbl, bl = tll[sll]
        ofc, nbo, bo = tof[sof]
        mlc, nbm, bm = tml[sml]
        if ofc > 31:
            _fail(where, f"sequence {i}: offset code {ofc}")
        ofv = (1 << ofc) + b.read(ofc)
        ml = MLB[mlc] + b.read(MLX[mlc])
        ll = LLB[llc] + b.read(LLX[llc])
        seqs.append((ll, ml, ofv))
        if i + 1 < k:
            sll = bl + b.read(nbl)
            sml = bm + b.read(nbm)
            sof = bo + b.read(nbo)
        if b.pos < 0:
            b.need(where, f"sequence {i}")
    b.done(where, "bitstream")
    sec = NS(count=k, count_bytes=nb_hdr, modes=modes, tables=rec, seqs=seqs, offsets=[],
             bitstream_at=q, bitstream_size=len(blk) - q)  # within the sequences section
    return sec, tabs


# ---- frames ---------------------------------------------------------------------

def parse_header(frame):
    """The frame header: NS(descriptor, single, window, content_size, did,
    checksum, size)."""
    if frame[:4] != zf.MAGIC:
        _fail("frame header", "bad magic")
    if len(frame) < 5:
        _fail("frame header", "truncated")
    fhd = frame[4]
    if fhd & 8:
        _fail("frame header", f"reserved bit of the descriptor {fhd:#04x} is set")
    fcs_flag, single, did_flag = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    q, window = 5, None
    if not single:
        if len(frame) < 6:
            _fail("frame header", "truncated")
        wd = frame[q]
        window = (1 << (10 + (wd >> 3))) // 8 * (8 + (wd & 7))
        q += 1
    db = (0, 1, 2, 4)[did_flag]
    did = int.from_bytes(frame[q:q + db], "little")
    q += db
    fb = (1 if single else 0, 2, 4, 8)[fcs_flag]
    if len(frame) < q + fb:
        _fail("frame header", "truncated")
    size = int.from_bytes(frame[q:q + fb], "little") + (256 if fb == 2 else 0) if fb else None
    q += fb
    if single:
        window = size
    return NS(descriptor=fhd, single=bool(single), window=window, content_size=size, did=did,
              did_bytes=db, checksum=bool(fhd & 4), size=q)


def dissect(frame, max_blocks=None):
    """One frame -> NS(header, blocks, content, end).  `end` is the offset
    just past the frame (its checksum included); the caller decides whether
    bytes may follow."""
    frame = bytes(frame)
    hdr = parse_header(frame)
    if hdr.did:
        _fail("frame header", f"dictionary id {hdr.did}")
    c = zf.Content()
    out = c.out
    blocks, pos, huf, tabs = [], hdr.size, None, None
    while True:
        i = len(blocks)
        where = f"block {i}"
        if max_blocks is not None and i >= max_blocks:
            _fail(where, f"more than {max_blocks} blocks")
        if pos + 3 > len(frame):
            _fail(where, "header past the frame's end")
        h = int.from_bytes(frame[pos:pos + 3], "little")
        last, tpe, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3
        n0 = len(out)
        blk = NS(type=tpe, size=size, last=bool(last), at=pos, start=n0, regen=0, literals=None,
                 sequences=None, lits=None)
        if tpe == 3:
            _fail(where, "reserved block type 3")
        if size > BLOCK:
            _fail(where, f"size {size} above 128 KiB")
        if tpe == 1:
            if pos + 1 > len(frame):
                _fail(where, "RLE byte past the frame's end")
            out += frame[pos:pos + 1] * size
            pos += 1
        else:
            if pos + size > len(frame):
                _fail(where, "content past the frame's end")
            body = frame[pos:pos + size]
            pos += size
            if tpe == 0:
                out += body
            else:
                if size < 3:
                    _fail(where, f"compressed block of {size} bytes")
                blk.literals, used, lits, huf = _literals(body, where, huf)
                blk.sequences, tabs = _sequences(body[used:], where, tabs)
                blk.sequences.at = used  # in the block's content
                blk.lits = lits
                p = 0
                for k, (ll, ml, ofv) in enumerate(blk.sequences.seqs):
                    if p + ll > len(lits):
                        _fail(where, f"sequence {k} takes more literals than the section has")
                    out += lits[p:p + ll]
                    p += ll
                    off = c.offset(ofv, ll)
                    if off <= 0 or off > len(out):
                        _fail(where, f"sequence {k}: offset {off} with {len(out)} bytes regenerated")
                    blk.sequences.offsets.append(off)
                    if off >= ml:
                        a = len(out) - off
                        out += out[a:a + ml]
                    else:
                        out += (bytes(out[-off:]) * (ml // off + 1))[:ml]
                out += lits[p:]
                if len(out) - n0 > BLOCK:
                    _fail(where, f"regenerates {len(out) - n0} bytes, above 128 KiB")
        blk.regen = len(out) - n0
        blocks.append(blk)
        if last:
            break
    if hdr.checksum:
        if pos + 4 > len(frame):
            _fail("frame", "checksum past the frame's end")
        want = zf.xxh64(bytes(out)) & 0xFFFFFFFF
        if int.from_bytes(frame[pos:pos + 4], "little") != want:
            _fail("frame", "content checksum mismatch")
        pos += 4
    if hdr.content_size is not None and hdr.content_size != len(out):
        _fail("frame", f"declares {hdr.content_size} bytes, regenerates {len(out)}")
    return NS(header=hdr, blocks=blocks, content=bytes(out), end=pos)
