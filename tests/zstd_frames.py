"""Hand-built RFC 8878 frames for the device frame checker (rcdc_zstd_check,
rcdc_zstd_dec.hip) -- test infrastructure, plain Python, no GPU and no
librcdc.so.

A frame writer on top of tests/zstd_model.py (frame headers with window
descriptors, every content-size width, dictionary-id fields and checksums;
raw / RLE / Huffman / treeless literals in every size format; predefined /
RLE / FSE / repeat sequence tables; every sequence-count form) and CASES, a
table of (name, frame, blob, expect_status, stricter) records:

  expect_status 0  the frame decodes to exactly the blob,
                1  it is well-formed but gives other bytes or another length,
                2  it is malformed (a wrong checksum over the right bytes too);
  stricter         None, or the RFC 8878 clause the checker enforces where the
                   libzstd at hand (1.4.8) is lax: that libzstd decodes the
                   frame to the blob, the checker calls it malformed.

The blob of a case is what its blocks regenerate: `Content` executes the
literals and sequences the way a decoder does, so a case states its
structure (lengths, offset values, tables) and the bytes follow.
tests/test_zstd_host.py proves every expectation with libzstd's streaming
decoder alone; tests/test_gpu_zstd_check.py then holds the device to it.
"""
from __future__ import annotations

import collections

import numpy as np

from oracle import zstd_ref as zr
from tests import zstd_model as zm

KiB = 1 << 10
BLOCK = 128 * KiB
MAGIC = b"\x28\xb5\x2f\xfd"

# ---- RFC 8878 3.1.1.3.2.1.1: literal-length and match-length codes ----------

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
                             4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027,
                                2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def ll_code(ll):
    return max(c for c in range(36) if LL_BASE[c] <= ll)


def ml_code(ml):
    return max(c for c in range(53) if ML_BASE[c] <= ml)


# the slice of rcdc_zstd_tables that zstd_model's sequence coder reads
T = {"llcode": [ll_code(v) for v in range(64)], "mlcode": [ml_code(v + 3) for v in range(128)],
     "llbits": LL_BITS, "mlbits": ML_BITS}


# ---- XXH64 (the frame checksum: its low 32 bits, seed 0) -------------------

_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9,
                           0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5)


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & _M


def _round(acc, x):
    return _rotl((acc + x * _P2) & _M, 31) * _P1 & _M


def xxh64(data: bytes, seed: int = 0) -> int:
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        w = np.frombuffer(data[:n // 32 * 32], "<u8").tolist()
        for i in range(0, len(w), 4):
            for k in range(4):
                v[k] = _round(v[k], w[i + k])
        i = n // 32 * 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = ((h ^ _round(0, v[k])) * _P1 + _P4) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[i:i + 8], "little")), 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = _rotl(h ^ (data[i] * _P5 & _M), 11) * _P1 & _M
        i += 1
    h ^= h >> 33
    h = h * _P2 & _M
    h ^= h >> 29
    h = h * _P3 & _M
    return h ^ (h >> 32)


# ---- frames ------------------------------------------------------------------

def window_desc(exp, mant=0):
    """The Window_Descriptor byte of 2^exp * (1 + mant / 8) bytes."""
    assert 10 <= exp <= 41 and 0 <= mant < 8
    return (exp - 10) << 3 | mant


def frame(blocks, size=None, *, fcs_bytes=None, wd=None, did_bytes=0, did=0, checksum=None,
          reserved=False):
    """A frame of (type, content, regenerated size) blocks.  Single-segment
    unless `wd` (a Window_Descriptor byte) is given; `size` is the declared
    content size in a field of `fcs_bytes` bytes (None: the smallest that
    holds it; 0: no field, needs `wd`); a dictionary-id field of `did_bytes`
    bytes holding `did`; `checksum`: the content (its XXH64 is appended) or
    the 32-bit value to write."""
    single = wd is None
    if fcs_bytes is None:
        fcs_bytes = 0 if size is None else 1 if size < 256 and single else \
            2 if 256 <= size < 65536 + 256 else 4
    assert fcs_bytes in (0, 1, 2, 4, 8) and (fcs_bytes or not single) and (single or fcs_bytes != 1)
    fhd = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6 | int(single) << 5 | int(reserved) << 3 | \
        int(checksum is not None) << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    out = bytearray(MAGIC + bytes([fhd]))
    if not single:
        out.append(wd)
    out += did.to_bytes(did_bytes, "little")
    if fcs_bytes:
        out += (size - 256 if fcs_bytes == 2 else size).to_bytes(fcs_bytes, "little")
    for i, (tpe, content, rsize) in enumerate(blocks):
        bsize = rsize if tpe == 1 else len(content)
        out += (int(i == len(blocks) - 1) | tpe << 1 | bsize << 3).to_bytes(3, "little") + content
    if checksum is not None:
        c = checksum if isinstance(checksum, int) else xxh64(bytes(checksum)) & 0xFFFFFFFF
        out += c.to_bytes(4, "little")
    return bytes(out)


# ---- literals sections (3.1.1.3.1) ----------------------------------------

def _lit_hdr(ltype, n, sf):
    if sf is None:
        sf = 0 if n < 32 else 1 if n < 4096 else 3
    if sf == 0:  # (one size-format bit: bit 3 belongs to the size)
        assert n < 32
        return bytes([ltype | n << 3])
    if sf == 1:
        assert n < 4096
        return (ltype | 1 << 2 | n << 4).to_bytes(2, "little")
    assert n < 1 << 20
    return (ltype | 3 << 2 | n << 4).to_bytes(3, "little")


def lit_raw(lits, sf=None):
    return _lit_hdr(0, len(lits), sf) + bytes(lits)


def lit_rle(byte, n, sf=None):
    return _lit_hdr(1, n, sf) + bytes([byte])


Huf = collections.namedtuple("Huf", "vals nb w maxsym")


def huf_table(lits=None, lengths=None):
    """The code table of `lits` as the device encoder builds it, or of the
    given code lengths (a list per symbol, 0 = absent)."""
    if lengths is None:
        lengths = zm.huf_lengths(np.bincount(np.frombuffer(bytes(lits), np.uint8), minlength=256))
    lengths = list(lengths) + [0] * (256 - len(lengths))
    vals, nb, w = zm.huf_codes(lengths)
    return Huf(vals, nb, w, max(s for s in range(256) if w[s]))


def huf_tree(tab, how="direct", weights=None):
    """Huffman_Tree_Description: the weights of symbols 0 .. maxsym - 1 as
    4-bit fields ("direct", at most 128) or FSE-coded ("fse"); `weights`
    overrides them (malformed cases)."""
    w = list(tab.w[:tab.maxsym]) if weights is None else list(weights)
    if how == "direct":
        assert len(w) <= 128
        return bytes([127 + len(w)]) + bytes(
            w[k] << 4 | (w[k + 1] if k + 1 < len(w) else 0) for k in range(0, len(w), 2))
    fw = zm.fse_compress_weights(w)
    assert fw is not None
    return bytes([len(fw)]) + fw


def huf_stream(part, tab, extra_bit=False):
    bw = zm.BitWriter()
    if extra_bit:  # a bit below the first code: never read
        bw.add(0, 1)
    for b in reversed(part):
        assert tab.nb[b]
        bw.add(tab.vals[b], tab.nb[b])
        bw.flush()
    bw.add(1, 1)
    bw.flush()
    if bw.nb:
        bw.out.append(bw.acc & 0xFF)
    return bytes(bw.out)


def lit_huf(lits, tab, *, sf=None, tree="direct", extra_bit=False, jump_add=0, weights=None):
    """Compressed_Literals_Block (tree "direct" / "fse") or, with tree None,
    Treeless_Literals_Block; size format sf (0: one stream; 1, 2, 3: four
    streams with 10-, 14-, 18-bit sizes), the smallest 4-stream one when
    None."""
    n = len(lits)
    desc = huf_tree(tab, tree, weights) if tree else b""
    if sf == 0:
        body = huf_stream(lits, tab, extra_bit)
    else:
        seg = (n + 3) // 4
        st = [huf_stream(lits[k * seg:min(n, (k + 1) * seg)], tab, extra_bit and k == 3)
              for k in range(4)]
        body = b"".join((len(s) + (jump_add if k == 2 else 0)).to_bytes(2, "little")
                        for k, s in enumerate(st[:3])) + b"".join(st)
    comp = len(desc) + len(body)
    if sf is None:
        sf = 1 if max(n, comp) < 1 << 10 else 2 if max(n, comp) < 1 << 14 else 3
    bits, hl = {0: 10, 1: 10, 2: 14, 3: 18}[sf], {0: 3, 1: 3, 2: 4, 3: 5}[sf]
    assert n < 1 << bits and comp < 1 << bits, (n, comp, sf)
    hdr = (2 if tree else 3) | sf << 2 | n << 4 | comp << (4 + bits)
    return hdr.to_bytes(hl, "little") + desc + body


# ---- sequences sections (3.1.1.3.2) ---------------------------------------

NAMES = ("ll", "of", "ml")
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}


def _tab(spec, prev, name):
    """(mode, description bytes, (tt, st, log)) of one stream's table."""
    if spec == "predef":
        pn, tl = zm.PREDEF_NORM[name]
        tt, st = zm.fse_ctable(pn, tl)
        return 0, b"", (tt, st, tl)
    if spec == "repeat":
        return 3, b"", prev[name]
    if spec[0] == "rle":
        return 1, bytes([spec[1]]), ([(0, 0)] * 64, [0], 0, spec[1])
    _, norm, tl = spec
    tt, st = zm.fse_ctable(norm, tl)
    return 2, zm.fse_write_ncount(norm, tl), (tt, st, tl)


def seq_count(k, form=None):
    if k < 128 and form is None:
        return bytes([k])
    if k < 0x7F00:
        assert form in (None, 2)
        return bytes([(k >> 8) + 0x80, k & 0xFF])
    return bytes([0xFF]) + (k - 0x7F00).to_bytes(2, "little")


def seq_section(seqs, specs=None, *, prev=None, form=None, modes_low=0, count=None, pad=b""):
    """Sequences_Section of [(ll, ml, offset value)]: per stream "predef",
    ("rle", code), ("fse", normalised counts, accuracy) or "repeat" (the
    tables `prev` of the block before).  Returns (bytes, tables).  `count`
    overrides the header's number, `modes_low` sets the reserved bits of the
    modes byte and `pad` goes below the bitstream (malformed and lax cases)."""
    if not seqs:
        return b"\x00", prev
    specs = dict({n: "predef" for n in NAMES}, **(specs or {}))
    made = {n: _tab(specs[n], prev, n) for n in NAMES}
    tabs = {n: made[n][2] for n in NAMES}
    for ll, ml, ofv in seqs:  # an RLE table codes one symbol only
        for n, c in (("ll", ll_code(ll)), ("of", ofv.bit_length() - 1), ("ml", ml_code(ml))):
            assert len(tabs[n]) == 3 or tabs[n][3] == c, (n, c, tabs[n][3])
    modes = made["ll"][0] << 6 | made["of"][0] << 4 | made["ml"][0] << 2 | modes_low
    bits = zm.encode_sequences_tabs({n: tabs[n][:3] for n in NAMES}, seqs, T, values=True)
    return (seq_count(len(seqs) if count is None else count, form) + bytes([modes]) +
            b"".join(made[n][1] for n in NAMES) + pad + bits), tabs


def norm_of(codes, nsym, tl, low=()):
    """Normalised counts over `nsym` symbols for the codes used (any
    iterable, with repeats), summing to 2^tl; the symbols in `low` get the
    "less than 1" probability -1."""
    cnt = [0] * nsym
    for c in codes:
        cnt[c] += 1
    for c in low:
        cnt[c] = max(cnt[c], 1)
    norm = zm.fse_normalize(cnt, tl)
    for c in low:  # a count of 1 and -1 take one cell each
        big = max((s for s in range(nsym) if s not in low), key=lambda s: norm[s])
        norm[big] += norm[c] - 1
        norm[c] = -1
    last = max(s for s in range(nsym) if norm[s])
    return norm[:last + 1]


# ---- the content a frame regenerates -----------------------------------------

class Content:
    """Executes blocks as a decoder does (3.1.1.4, 3.1.1.5): the blob."""

    def __init__(self, lax_zero_offset=False):
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.lax = lax_zero_offset  # libzstd 1.4.8: a repeat offset of 0 becomes 1

    def raw(self, data):
        self.out += data
        return (0, bytes(data), len(data))

    def rle(self, byte, n):
        self.out += bytes([byte]) * n
        return (1, bytes([byte]), n)

    def offset(self, ofv, ll):
        r = self.rep
        if ofv > 3:
            off = ofv - 3
            self.rep = [off, r[0], r[1]]
            return off
        idx = ofv - 1 + (ll == 0)
        if idx == 0:
            return r[0]
        off = r[1] if idx == 1 else r[2] if idx == 2 else r[0] - 1
        if off == 0 and self.lax:
            off = 1
        self.rep = [off, r[0], r[2]] if idx == 1 else [off, r[0], r[1]]
        return off

    def execute(self, lits, seqs, check=True):
        p = 0
        for ll, ml, ofv in seqs:
            self.out += lits[p:p + ll]
            p += ll
            off = self.offset(ofv, ll)
            if check:
                assert 0 < off <= len(self.out), (off, len(self.out))
            if off >= ml:
                self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
            else:
                pat = bytes(self.out[-off:])
                self.out += (pat * (ml // off + 1))[:ml]
        assert not check or p <= len(lits)
        self.out += lits[p:]

    def block(self, lits, seqs, litsec=None, **kw):
        """A compressed block of these literals (section `litsec`, raw when
        None) and sequences (seq_section's keywords); returns the block tuple
        and leaves the tables in self.tabs."""
        n0 = len(self.out)
        self.execute(bytes(lits), seqs)
        sec, self.tabs = seq_section(seqs, kw.pop("specs", None), prev=getattr(self, "tabs", None),
                                     **kw)
        return (2, (lit_raw(lits) if litsec is None else litsec) + sec, len(self.out) - n0)

    def blob(self):
        return bytes(self.out)


def sections(block):
    """(literals type, size format, sequence count, modes byte or None) of a
    compressed block's content: what a case asserts about its structure."""
    b0 = block[0]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt < 2:
        sf = 0 if sf == 2 else sf
        hl = 1 if sf == 0 else 2 if sf == 1 else 3
        n = int.from_bytes(block[:hl], "little") >> (3 if hl == 1 else 4)
        q = hl + (n if lt == 0 else 1)
    else:
        hl, bits = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
        q = hl + ((int.from_bytes(block[:hl], "little") >> (4 + bits)) & ((1 << bits) - 1))
    s0 = block[q]
    if s0 == 0:
        return lt, sf, 0, None
    if s0 < 128:
        k, q = s0, q + 1
    elif s0 < 255:
        k, q = ((s0 - 128) << 8) + block[q + 1], q + 2
    else:
        k, q = block[q + 1] + (block[q + 2] << 8) + 0x7F00, q + 3
    return lt, sf, k, block[q]


# ---- the cases ---------------------------------------------------------------

Case = collections.namedtuple("Case", "name frame blob expect_status stricter")
CASES = []


def _add(name, fr, blob, status, stricter=None):
    assert all(c.name != name for c in CASES), name
    assert status in (0, 1, 2) and (stricter is None or status == 2)
    CASES.append(Case(name, bytes(fr), bytes(blob), status, stricter))


def _rb(rng, n, hi=256):
    return rng.integers(0, hi, n, dtype=np.uint8).tobytes()


def _skew(rng, n, nsym=16, base=0):
    """Bytes over `nsym` symbols of falling frequency: Huffman literals."""
    p = 0.75 ** np.arange(nsym)
    return bytes((rng.choice(nsym, n, p=p / p.sum()) + base).astype(np.uint8))


def _headers(rng):
    d200, d300 = _rb(rng, 200), _rb(rng, 300)
    for fb in (1, 2, 4, 8):
        d = d200 if fb == 1 else d300
        _add(f"hdr single fcs{fb}", frame([(0, d, len(d))], len(d), fcs_bytes=fb), d, 0)
    for fb in (0, 2, 4, 8):
        _add(f"hdr window 1K fcs{fb}",
             frame([(0, d300, 300)], 300 if fb else None, fcs_bytes=fb, wd=window_desc(10)), d300, 0)
    for name, wd, st in (("1.875K", window_desc(10, 7), 0), ("128K", window_desc(17), 0),
                         ("1M", window_desc(20), 0), ("2^27", window_desc(27), 0),
                         ("2^27+2^24", window_desc(27, 1), 2)):
        _add(f"hdr window {name} no fcs", frame([(0, d300, 300)], fcs_bytes=0, wd=wd), d300, st)
    for db in (1, 2, 4):
        _add(f"hdr did{db} zero", frame([(0, d300, 300)], 300, did_bytes=db), d300, 0)
        _add(f"hdr did{db} nonzero", frame([(0, d300, 300)], 300, did_bytes=db, did=1), d300, 2)
    _add("hdr reserved bit", frame([(0, d300, 300)], 300, reserved=True), d300, 2)
    good = frame([(0, d300, 300)], 300)
    _add("hdr content size + 1", frame([(0, d300, 300)], 301), d300, 1)
    _add("hdr content size - 1", frame([(0, d300, 300)], 299), d300, 1)
    _add("blob one byte longer", good, d300 + b"x", 1)
    _add("blob one byte shorter", good, d300[:-1], 1)
    _add("blob one byte longer, no fcs", frame([(0, d300, 300)], fcs_bytes=0, wd=0), d300 + b"x", 1)
    _add("blob one byte shorter, no fcs", frame([(0, d300, 300)], fcs_bytes=0, wd=0), d300[:-1], 1)
    _add("trailing byte", good + b"\x00", d300, 2)
    _add("two frames", good + good, d300, 2)
    nofcs = frame([(0, d300, 300)], fcs_bytes=0, wd=0)
    _add("two frames, no fcs, the blob of both", nofcs + nofcs, d300 + d300, 2)
    _add("skippable frame first", b"\x50\x2a\x4d\x18" + (4).to_bytes(4, "little") + b"skip" + good,
         d300, 2)
    _add("block type 3", frame([(3, d300, 300)], 300), d300, 2)
    big = _rb(rng, BLOCK + 1)
    _add("raw block 131073", frame([(0, big, len(big))], len(big)), big, 2)
    _add("raw block 131072", frame([(0, big[:-1], BLOCK)], BLOCK), big[:-1], 0)


def _checksums(rng):
    d = _rb(rng, 333)
    z = bytes([7]) * 5000
    for tag, kw in (("", {}), (" no fcs", {"fcs_bytes": 0, "wd": window_desc(17)})):
        sz = None if kw else 333
        _add("checksum raw" + tag, frame([(0, d, 333)], sz, checksum=d, **kw), d, 0)
        _add("checksum raw wrong" + tag,
             frame([(0, d, 333)], sz, checksum=xxh64(d) & 0xFFFFFFFF ^ 0x100, **kw), d, 2)
    _add("checksum rle", frame([(1, b"\x07", 5000)], 5000, checksum=z), z, 0)
    _add("checksum rle wrong", frame([(1, b"\x07", 5000)], 5000, checksum=0), z, 2)
    # every tail of XXH64: 0-31 bytes after the stripes, and none before
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 127, 128 + 13, 12345):
        e = _rb(rng, n)
        _add(f"checksum raw {n} bytes", frame([(0, e, n)], fcs_bytes=0, wd=window_desc(17), checksum=e),
             e, 0)
    c = Content()
    lits = _skew(rng, 9000, 20, 65)
    blocks = [c.block(lits, [(100, 40, 13), (1000, 300, 1), (0, 5, 2)],
                      lit_huf(lits, huf_table(lits)))]
    blob = c.blob()
    _add("checksum compressed", frame(blocks, len(blob), checksum=blob), blob, 0)
    _add("checksum compressed wrong", frame(blocks, len(blob), checksum=xxh64(blob) + 1 & 0xFFFFFFFF),
         blob, 2)
    _add("checksum missing", frame(blocks, len(blob), checksum=blob)[:-4], blob, 2)
    other = bytearray(blob)
    other[4000] ^= 1
    _add("checksum right, blob wrong", frame(blocks, len(blob), checksum=blob), other, 1)
    _add("checksum of another blob", frame(blocks, len(blob), checksum=bytes(other)), blob, 2)


def _blocks(rng):
    d = _rb(rng, 700)
    for tag, kw in ((" one pass", {"size": 700}), (" streamed", {"fcs_bytes": 0, "wd": window_desc(17)})):
        _add("empty raw and RLE blocks" + tag,
             frame([(0, b"", 0), (1, b"\x55", 0), (0, d[:300], 300), (0, b"", 0), (1, b"\x00", 0),
                    (0, d[300:], 400), (1, b"\xff", 0), (0, b"", 0)], **kw), d, 0)
        _add("empty RLE block last" + tag, frame([(0, d, 700), (1, b"\x01", 0)], **kw), d, 0)
    big = _rb(rng, 1 + (BLOCK - 1) + BLOCK)
    fr = frame([(0, big[:1], 1), (0, big[1:BLOCK], BLOCK - 1), (0, big[BLOCK:], BLOCK)], len(big))
    assert zr.blocks(fr) == [(0, 1, False), (0, BLOCK - 1, False), (0, BLOCK, True)]
    _add("raw blocks 1, 131071, 131072", fr, big, 0)
    bad = bytearray(big)
    bad[BLOCK - 1] ^= 0x80  # the last byte of the 131071-byte block
    _add("raw blocks 1, 131071, 131072, one byte wrong", fr, bad, 1)
    z = b"\x09" + b"\x0a" * (BLOCK - 1) + b"\x0b" * BLOCK
    fr = frame([(1, b"\x09", 1), (1, b"\x0a", BLOCK - 1), (1, b"\x0b", BLOCK)], len(z))
    _add("RLE blocks 1, 131071, 131072", fr, z, 0)
    _add("RLE blocks 1, 131071, 131072, last byte wrong", fr, z[:-1] + b"\x0c", 1)
    _add("RLE block 131073", frame([(1, b"\x0b", BLOCK + 1)], BLOCK + 1), b"\x0b" * (BLOCK + 1), 2)


def _window(rng):
    w1k = window_desc(10)
    # Block_Maximum_Size = min(window, 128 KiB) off the one-pass path
    d = _rb(rng, 12288)
    four = [(0, d[i:i + 4096], 4096) for i in range(0, 12288, 4096)]
    _add("window 1K, raw block 4K, no fcs", frame(four[:1], fcs_bytes=0, wd=w1k), d[:4096], 2)
    _add("window 1K, raw blocks 4K, fcs 12288", frame(four, 12288, wd=w1k), d, 2)
    _add("window 1K, raw block 4K, fcs 4096 (one pass)", frame(four[:1], 4096, wd=w1k), d[:4096], 0)
    _add("window 1K, raw block 1025, no fcs", frame([(0, d[:1025], 1025)], fcs_bytes=0, wd=w1k),
         d[:1025], 2)
    _add("window 1K, RLE block 100000, no fcs", frame([(1, b"\x03", 100000)], fcs_bytes=0, wd=w1k),
         b"\x03" * 100000, 2)
    c = Content()
    blk = c.block(b"q", [(1, 1500, 1)])
    _add("window 1K, compressed block regenerates 1501", frame([blk], fcs_bytes=0, wd=w1k), c.blob(), 2)
    c = Content()
    blk = c.block(b"q", [(1, 1023, 1)])
    _add("window 1K, compressed block regenerates 1024", frame([blk], fcs_bytes=0, wd=w1k), c.blob(), 0)
    # blocks of 1 KiB, matches of offset exactly 1024 and 1023
    c = Content()
    blocks = [c.raw(_rb(rng, 1024))]
    blocks.append(c.block(_rb(rng, 1024 - 100), [(0, 100, 1024 + 3)]))
    blocks.append(c.block(_rb(rng, 1024 - 57), [(5, 50, 1023 + 3), (900, 7, 1024 + 3)]))
    blocks.append(c.block(_rb(rng, 300 - 20), [(280, 20, 1024 + 3)]))
    _add("window 1K, 1 KiB blocks, offsets 1024 and 1023", frame(blocks, fcs_bytes=0, wd=w1k), c.blob(), 0)
    # offsets past the window: 9000 >= 8 windows is malformed, 1000 decodes
    for off, st in ((9000, 2), (1000, 0)):
        c = Content()
        blocks = [c.raw(_rb(rng, 1024)) for _ in range(9)]
        blocks.append(c.block(_rb(rng, 200), [(10, 100, off + 3)]))
        _add(f"window 1K, offset {off} inside the output", frame(blocks, fcs_bytes=0, wd=w1k), c.blob(), st)
        if off == 9000:  # the same frame declaring a content size that fits one pass: no window there
            c = Content()
            blocks = [c.raw(_rb(rng, 1000)) for _ in range(8)]
            blocks.append(c.block(_rb(rng, 50), [(10, 100, 8000 + 3)]))
            assert len(c.out) <= 8192
            _add("window 1K, offset 8000, content size 8150 (one pass)",
                 frame(blocks, len(c.out), wd=w1k), c.blob(), 0)


def _small_blocks(rng):
    d = _rb(rng, 10000)
    for tag, kw in ((" one pass", {"size": 501}), (" streamed", {"fcs_bytes": 0, "wd": window_desc(17)})):
        _add("compressed block of 2 bytes" + tag,
             frame([(0, d[:500], 500), (2, b"\x00\x00", 0), (0, d[500:501], 1)], **kw), d[:501], 2)
        _add("compressed block of 3 bytes" + tag,
             frame([(0, d[:500], 500), (2, b"\x08" + d[500:501] + b"\x00", 1)], **kw), d[:501], 0)
        _add("compressed block of 1 byte" + tag,
             frame([(0, d[:500], 500), (2, b"\x00", 0), (0, d[500:501], 1)], **kw), d[:501], 2)
    # a compressed block regenerating 131072 bytes, and one more
    for ml, st in ((BLOCK - 1, 0), (BLOCK, 2)):
        c = Content()
        blk = c.block(b"m", [(1, ml, 1)])
        _add(f"compressed block regenerates {ml + 1}", frame([blk], ml + 1), c.blob(), st)
        c = Content()
        blk = c.block(b"m", [(1, ml, 1)])
        _add(f"compressed block regenerates {ml + 1}, no fcs", frame([blk], fcs_bytes=0, wd=window_desc(20)),
             c.blob(), st)
    c = Content()
    blk = (2, lit_rle(0x33, BLOCK) + b"\x00", BLOCK)
    _add("131072 RLE literals, no sequences", frame([blk], BLOCK), b"\x33" * BLOCK, 0)


def _literals(rng):
    for n in (0, 5, 31, 32, 4095, 4096):
        d = _rb(rng, n)
        for sf in (0, 1, 3):
            if (sf == 0 and n >= 32) or (sf == 1 and n >= 4096):
                continue
            blk = lit_raw(d, sf) + b"\x00"
            assert sections(blk)[:3] == (0, sf, 0)
            wrong = bytes(d[:-1]) + bytes([d[-1] ^ 1]) if n else b"x"
            # (no literals in one header byte and no sequences: a block of 2 bytes, below the minimum)
            _add(f"raw literals {n} sf{sf}", frame([(2, blk, n), (0, b"ab", 2)], n + 2), d + b"ab",
                 2 if len(blk) < 3 else 0)
            if n in (5, 4096):
                _add(f"raw literals {n} sf{sf}, last wrong", frame([(2, blk, n), (0, b"ab", 2)], n + 2),
                     wrong + b"ab", 1)
                # (a 1-byte header cannot be cut: there the literals are missing)
                _add(f"raw literals {n} sf{sf}, " + ("literals missing" if sf == 0 else "header truncated"),
                     frame([(2, blk[:1 if sf != 3 else 2], 0)], n), d, 2)
            blk = lit_rle(0x41, n, sf) + b"\x00"
            assert sections(blk)[:3] == (1, sf, 0)
            _add(f"RLE literals {n} sf{sf}", frame([(2, blk, n), (0, b"ab", 2)], n + 2),
                 b"\x41" * n + b"ab", 0)
            if n in (5, 4096):
                _add(f"RLE literals {n} sf{sf}, " + ("byte missing" if sf == 0 else "header truncated"),
                     frame([(2, blk[:1 if sf != 3 else 2], 0)], n), b"\x41" * n, 2)
                _add(f"RLE literals {n} sf{sf}, last wrong", frame([(2, blk, n), (0, b"ab", 2)], n + 2),
                     b"\x41" * (n - 1) + b"\x40ab", 1)


def _huffman(rng):
    def one(name, lits, tab=None, st=0, blob=None, **kw):
        tab = tab or huf_table(lits)
        blk = lit_huf(lits, tab, **kw) + b"\x00"
        _add(name, frame([(2, blk, len(lits))], len(lits)), lits if blob is None else blob, st)
        return blk

    for n in (1023, 1024, 16383, 16384):
        lits = _skew(rng, n)
        blk = one(f"huffman 4 streams regen {n}", lits)
        assert sections(blk)[:2] == (2, 1 if n < 1024 else 2 if n < 16384 else 3)
        bad = bytearray(lits)
        bad[n - 1] ^= 1
        _add(f"huffman 4 streams regen {n}, last byte wrong", frame([(2, blk, n)], n), bad, 1)
    lits = _skew(rng, 1000)
    for sf in (2, 3):
        one(f"huffman regen 1000 in size format {sf}", lits, sf=sf)
    # compressed size on both sides of the 10-bit limit: 11-bit codes for
    # every byte of the section (a table whose longest code is 11 bits)
    deep = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11]
    tab = huf_table(lengths=deep)
    assert max(tab.nb) == 11
    lits = bytes([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11] * 20)
    one("huffman longest code 11 bits", lits, tab)
    one("huffman longest code 11 bits, 1 stream", lits, tab, sf=0)
    for n in (720, 760):
        lits = bytes([10, 11] * (n // 2))
        blk = one(f"huffman regen {n}, compressed around 1023", lits, tab)
        csz = (int.from_bytes(blk[:3], "little") >> 14 if sections(blk)[1] == 1 else
               (int.from_bytes(blk[:4], "little") >> 18))
        assert (csz < 1024) == (n == 720), csz
    # the same at the 14-bit limit: regenerated sizes that fit size format 2,
    # the compressed size on either side of 16383 (format 3 by it alone)
    for n, sf in ((11900, 2), (11940, 3)):
        lits = bytes([10, 11] * (n // 2))
        # (a 128 KiB window: the block is larger than its content, which a
        # single-segment frame's Block_Maximum_Size would not allow)
        blk = lit_huf(lits, tab) + b"\x00"
        _add(f"huffman regen {n}, compressed around 16383", frame([(2, blk, n)], n, wd=window_desc(17)),
             lits, 0)
        csz = (int.from_bytes(blk[:4], "little") >> 18 if sf == 2 else
               (int.from_bytes(blk[:5], "little") >> 22) & 0x3FFFF)
        assert sections(blk)[1] == sf and (csz < 16384) == (sf == 2) and abs(csz - 16384) < 60, csz
        bad = bytearray(lits)
        bad[n - 1] ^= 1
        _add(f"huffman regen {n}, compressed around 16383, last byte wrong",
             frame([(2, blk, n)], n, wd=window_desc(17)), bad, 1)
    _add("huffman block larger than a single-segment frame's content",
         frame([(2, blk, n)], n), lits, 2)
    # (the 18-bit limit of size format 3 cannot be reached: a block holds at
    # most 128 KiB, half of 2^18)
    # a 12-bit table: RFC 8878 4.2.1 caps the code length at 11
    tab12 = huf_table(lengths=deep[:-1] + [12, 12])
    lits = bytes(range(13)) * 10
    blk = lit_huf(lits, tab12) + b"\x00"
    _add("huffman longest code 12 bits", frame([(2, blk, len(lits))], len(lits)), lits, 2)
    lits = _skew(rng, 500)
    blk = one("huffman 1 stream", lits, sf=0)
    assert sections(blk)[:2] == (2, 0)
    bad = bytearray(lits)
    bad[0] ^= 0x80
    _add("huffman 1 stream, first byte wrong", frame([(2, blk, 500)], 500), bad, 1)
    for n in (6, 7, 8, 9):
        one(f"huffman 4 streams regen {n}", _skew(rng, 400, 4)[:n] if n > 6 else bytes([0, 1, 0, 2, 1, 0]),
            huf_table(lengths=[1, 2, 3, 3]))
    for nsym in (7, 8, 128, 129):  # an odd and an even number of explicit weights
        lits = _skew(rng, 300, 5) + bytes(range(nsym)) * 2
        tab = huf_table(lits)
        assert tab.maxsym == nsym - 1
        one(f"huffman direct weights, {nsym - 1} explicit", lits, tab)
    lits = _skew(rng, 2000, 12) + bytes(range(200))
    one("huffman FSE-coded weights, 199 explicit", lits, tree="fse")
    lits = _skew(rng, 3000, 40) + bytes(range(256)) * 2
    tab = huf_table(lits)
    assert tab.maxsym == 255
    one("huffman FSE-coded weights, 255 explicit", lits, tab, tree="fse")
    # treeless literals: the table of the block before, also across raw literals
    l1, l2, l3 = _skew(rng, 600), _skew(rng, 500), _rb(rng, 40)
    tab = huf_table(l1 + l2)
    b1 = lit_huf(l1, tab) + b"\x00"
    b2 = lit_huf(l2, tab, tree=None) + b"\x00"
    b2s = lit_huf(l2, tab, tree=None, sf=0) + b"\x00"
    assert sections(b2)[0] == 3
    _add("treeless literals in the second block", frame([(2, b1, 600), (2, b2, 500)], 1100), l1 + l2, 0)
    _add("treeless literals, 1 stream", frame([(2, b1, 600), (2, b2s, 500)], 1100), l1 + l2, 0)
    _add("treeless literals after a block of raw literals",
         frame([(2, b1, 600), (2, lit_raw(l3) + b"\x00", 40), (0, l3, 40), (2, b2, 500)], 1180),
         l1 + l3 + l3 + l2, 0)
    _add("treeless literals in a first block", frame([(2, b2, 500)], 500), l2, 2)
    _add("treeless literals after raw literals only",
         frame([(2, lit_raw(l3) + b"\x00", 40), (2, b2, 500)], 540), l3 + l2, 2)
    # malformed tables and streams
    lits = _skew(rng, 400, 6)
    tab = huf_table(lits)
    w = list(tab.w[:tab.maxsym])
    one("huffman stream with an unread bit", lits, tab, st=2, extra_bit=True)
    one("huffman 1 stream with an unread bit", lits, tab, st=2, extra_bit=True, sf=0)
    one("huffman jump table longer than the section", lits, tab, st=2, jump_add=400)
    heavy = list(w)
    heavy[0] = 12
    one("huffman weight 12", lits, tab, st=2, weights=heavy)
    odd = list(w)
    odd[w.index(max(w))] -= 1  # the rest is then no power of two
    total = sum(1 << (x - 1) for x in odd if x)
    rest = (1 << total.bit_length()) - total
    assert rest & (rest - 1)
    one("huffman weights leave no power of two", lits, tab, st=2, weights=odd)
    # no weight-1 pair: weights 2, 2 and an implied 3 (codes of 2, 2, 1 bits in a 3-bit table)
    sec = (2 | 1 << 2 | 8 << 4 | 9 << 14).to_bytes(3, "little") + bytes([129, 0x22]) + \
        (1).to_bytes(2, "little") * 3 + b"\x01" * 4
    _add("huffman table without weight-1 symbols", frame([(2, sec + b"\x00", 8)], 8), bytes(8), 2)
    for sf, cut in ((1, 2), (2, 3), (3, 4)):
        lits = _skew(rng, 300)
        blk = lit_huf(lits, huf_table(lits), sf=sf)[:cut]
        _add(f"huffman literals header truncated sf{sf}", frame([(2, blk, 0)], 300), bytes(300), 2)


def _seq_codes(rng):
    # every LL and ML code at its baseline and at its largest extra bits (as
    # far as a block of 128 KiB holds the sequence), literals RLE-coded so the
    # frames stay small; matches of offset 1
    blocks, c = [], Content()

    def flush(lits_n, seqs):
        blocks.append(c.block(b"\x5a" * lits_n, seqs, lit_rle(0x5a, lits_n)))

    pend, room, nl = [], BLOCK, 0
    want = [(LL_BASE[k], 3) for k in range(36)] + \
        [(LL_BASE[k] + (1 << LL_BITS[k]) - 1, 3) for k in range(16, 35)] + [(BLOCK - 3, 3)] + \
        [(0 if k % 2 else 1, ML_BASE[k]) for k in range(53)] + \
        [(1, ML_BASE[k] + (1 << ML_BITS[k]) - 1) for k in range(32, 52)] + [(1, BLOCK - 1)]
    for ll, ml in want:
        if ll + ml > room:
            flush(nl, pend)
            pend, room, nl = [], BLOCK, 0
        # (the frame's first sequence needs a literal before its match)
        pend.append((ll if c.out or pend or ll else 1, ml, 1 + 3))
        nl += pend[-1][0]
        room -= pend[-1][0] + ml
    flush(nl, pend)
    blob = c.blob()
    used_ll = {ll_code(s[0]) for b in [want] for s in b}
    used_ml = {ml_code(s[1]) for s in want}
    assert used_ll == set(range(36)) and used_ml == set(range(53))
    _add("every LL and ML code, baseline and largest extra bits", frame(blocks, len(blob)), blob, 0)
    bad = bytearray(blob)
    bad[len(bad) // 2] ^= 4
    _add("every LL and ML code, one byte wrong", frame(blocks, len(blob)), bad, 1)
    # offset codes 0 .. 17: offsets up to 2^17 reach into the block before
    c = Content()
    blocks = [c.raw(_rb(rng, BLOCK)), c.raw(_rb(rng, 4))]
    seqs = [(2, 3, 1), (1, 4, 2), (1, 3, 3)]  # offset values 1-3: codes 0 and 1
    seqs += [(1, 5, (1 << k) + 3 - (k > 2)) for k in range(2, 18)]  # offsets 2^k (- 1)
    seqs += [(0, 7, (1 << 17) + 3), (3, 9, (1 << 17) - 1 + 3)]
    blocks.append(c.block(_rb(rng, 64), seqs))
    assert {s[2].bit_length() - 1 for s in seqs} == set(range(18))
    blob = c.blob()
    _add("offset codes 0-17, offset 2^17 into the block before", frame(blocks, len(blob)), blob, 0)
    # one byte before the frame's start
    c = Content()
    b0 = c.raw(_rb(rng, 100))
    c.execute(b"abcdef", [(6, 4, 106 + 3)])
    sec, _ = seq_section([(6, 4, 107 + 3)])
    _add("offset one byte before the frame's start",
         frame([b0, (2, lit_raw(b"abcdef") + sec, 10)], 110), c.blob(), 2)
    sec, _ = seq_section([(6, 4, 106 + 3)])
    _add("offset reaching the frame's first byte", frame([b0, (2, lit_raw(b"abcdef") + sec, 10)], 110),
         c.blob(), 0)
    sec, _ = seq_section([(7, 4, 106 + 3)])
    _add("sequence taking more literals than the section has",
         frame([b0, (2, lit_raw(b"abcdef") + sec, 10)], 110), c.blob(), 2)


def _seq_counts(rng):
    for k in (1, 63, 64, 65, 127, 128, 129, 0x7EFF, 0x7F00):
        c = Content()
        lits = _rb(rng, 40 + k // 8)
        seqs = [(1 if i % 8 == 0 else 0, 3 + (i % 3 == 0), (i % 30 + 1) + 3) for i in range(k)]
        seqs[0] = (37, 3, 30 + 3)
        blk = c.block(lits, seqs)
        assert sections(blk[1])[2] == k
        blob = c.blob()
        assert len(blob) <= BLOCK
        _add(f"{k} sequences", frame([blk], len(blob)), blob, 0)
        if k in (1, 127):
            c = Content()
            blk = c.block(lits, seqs, form=2)
            assert sections(blk[1])[2] == k and blk[1][len(lit_raw(lits))] == 0x80
            _add(f"{k} sequences, count in 2 bytes", frame([blk], len(blob)), blob, 0)
        if k in (64, 0x7F00):
            bad = bytearray(blob)
            bad[-1] ^= 1
            _add(f"{k} sequences, last byte wrong", frame([blk], len(blob)), bad, 1)


def _seq_tables(rng):
    lits = _rb(rng, 200)
    base = [(4, 5, 9 + 3), (4, 5, 10 + 3), (4, 5, 8 + 3), (4, 5, 12 + 3), (4, 5, 5 + 3)]
    # RLE mode on each stream alone and on all three (LL code 4, OF code 3, ML code 2)
    rle = {"ll": ("rle", 4), "of": ("rle", 3), "ml": ("rle", 2)}
    for which in (("ll",), ("of",), ("ml",), NAMES):
        c = Content()
        b0 = c.raw(lits[:32])
        blk = c.block(lits, base, specs={n: rle[n] for n in which})
        want = sum((1 << s) for n, s in (("ll", 6), ("of", 4), ("ml", 2)) if n in which)
        assert sections(blk[1])[3] == want
        _add("RLE tables: " + " ".join(which), frame([b0, blk], len(c.out)), c.blob(), 0)
    for n, sym in (("ll", 36), ("of", 32), ("ml", 53)):
        c = Content()
        b0 = c.raw(lits[:32])
        blk = c.block(lits, base, specs={n: rle[n]})
        i = len(lit_raw(lits)) + 2
        assert blk[1][i] == rle[n][1]
        _add(f"RLE table symbol above the alphabet: {n}",
             frame([b0, (2, blk[1][:i] + bytes([sym]) + blk[1][i + 1:], blk[2])], len(c.out)), c.blob(), 2)
    # FSE tables at accuracy 5 and at the largest (9 / 8 / 9), with -1
    # symbols and a run of more than 24 zeros in the description
    seqs = [(i % 20, 3 + (40 if i % 5 == 0 else i % 4), (i % 40 + 1) + 3) for i in range(1, 60)]
    seqs[0] = (10, 3, 2 + 3)
    lits = _rb(rng, sum(s[0] for s in seqs) + 9)
    codes = {"ll": [ll_code(s[0]) for s in seqs], "of": [s[2].bit_length() - 1 for s in seqs],
             "ml": [ml_code(s[1]) for s in seqs]}
    assert max(codes["ml"]) >= 34 and sorted(set(codes["ml"]))[-2] < max(codes["ml"]) - 25
    for tag, logs in (("accuracy 5", (5, 5, 5)), ("accuracy 6", (6, 6, 6)), ("accuracy 9/8/9", (9, 8, 9))):
        for low in (False, True):
            specs = {}
            for n, tl in zip(NAMES, logs):
                lo = (max(codes[n]), MAX_SYM[n]) if low else ()
                specs[n] = ("fse", norm_of(codes[n], MAX_SYM[n] + 1, tl, lo), tl)
                assert not low or -1 in specs[n][1]
            c = Content()
            blk = c.block(lits, seqs, specs=specs)
            assert sections(blk[1])[3] == 0xA8
            _add(f"FSE tables {tag}" + (" with -1 symbols" if low else ""), frame([blk], len(c.out)),
                 c.blob(), 0)
    # FSE accuracy above the stream's maximum, counts past the table, a symbol above the alphabet
    c = Content()
    good = c.block(lits, seqs, specs={"of": ("fse", norm_of(codes["of"], 32, 8), 8)})
    at = len(lit_raw(lits)) + 2
    assert good[1][at] & 15 == 3
    _add("FSE offset table accuracy 9", frame([(2, good[1][:at] + bytes([good[1][at] + 1]) + good[1][at + 1:],
                                               good[2])], len(c.out)), c.blob(), 2)
    for n, tl in (("ll", 10), ("ml", 10)):
        c = Content()
        blk = c.block(lits, seqs, specs={n: ("fse", norm_of(codes[n], MAX_SYM[n] + 1, 9), 9)})
        at = len(lit_raw(lits)) + 2
        assert blk[1][at] & 15 == 4
        _add(f"FSE {n} table accuracy 10", frame([(2, blk[1][:at] + bytes([blk[1][at] + 1]) + blk[1][at + 1:],
                                                  blk[2])], len(c.out)), c.blob(), 2)
    # a description whose first count alone exceeds the table (accuracy 5, count 63)
    c = Content()
    blk = c.block(lits, seqs, specs={"of": ("fse", norm_of(codes["of"], 32, 5), 5)})
    desc = zm.fse_write_ncount(norm_of(codes["of"], 32, 5), 5)
    i = blk[1].index(desc, len(lit_raw(lits)))
    over = bytes([desc[0] | 0xF0, desc[1] | 0x03]) + desc[2:]
    _add("FSE counts overshoot the table", frame([(2, blk[1][:i] + over + blk[1][i + len(desc):], blk[2])],
                                                len(c.out)), c.blob(), 2)
    # a 33rd offset symbol / a 37th literal-length symbol: one count too many
    for n, nsym in (("of", 33), ("ll", 37), ("ml", 54)):
        norm = [1] * nsym + [0]
        tl = 6 if nsym > 32 else 5
        norm[0] += (1 << tl) - nsym
        if norm[0] < 1:
            tl = 7
            norm[0] += 64
        desc = zm.fse_write_ncount(norm[:nsym], tl)
        c = Content()
        blk = c.block(lits, seqs, specs={n: ("fse", norm_of(codes[n], MAX_SYM[n] + 1, 6), 6)})
        old = zm.fse_write_ncount(norm_of(codes[n], MAX_SYM[n] + 1, 6), 6)
        i = blk[1].index(old, len(lit_raw(lits)))
        _add(f"FSE {n} table with a symbol above the alphabet",
             frame([(2, blk[1][:i] + desc + blk[1][i + len(old):], blk[2])], len(c.out)), c.blob(), 2)
    # repeat mode in the second and third block, also after an RLE-mode table
    c = Content()
    l2 = _rb(rng, 200)
    fse = {n: ("fse", norm_of(codes[n], MAX_SYM[n] + 1, 7), 7) for n in NAMES}
    rep = {n: "repeat" for n in NAMES}
    blocks = [c.block(lits, seqs, specs=fse), c.block(lits, seqs[::-1], specs=rep),
              c.block(lits, seqs[5:40], specs=dict(rep, of="predef"))]
    assert [sections(b[1])[3] for b in blocks] == [0xA8, 0xFC, 0xCC]
    blocks.append(c.block(l2, base, specs=rle))
    blocks.append(c.block(l2, base[::-1], specs=rep))
    blocks.append(c.raw(b"between"))
    blocks.append(c.block(l2, base[1:], specs=dict(rep, ml="predef")))
    _add("repeat tables in later blocks, after FSE and RLE tables", frame(blocks, len(c.out)), c.blob(), 0)
    c = Content()
    c.tabs = {n: _tab("predef", None, n)[2] for n in NAMES}
    for which in NAMES:
        c = Content()
        c.tabs = {n: _tab("predef", None, n)[2] for n in NAMES}
        blk = c.block(l2, [(20, 5, 9 + 3)] + base, specs={which: "repeat"})
        _add(f"repeat table in a first block: {which}", frame([blk], len(c.out)), c.blob(), 2)
        c = Content()
        first = (2, lit_raw(b"xy") + b"\x00", 2)
        c.out += b"xy"
        c.tabs = {n: _tab("predef", None, n)[2] for n in NAMES}
        blk = c.block(l2, [(20, 5, 9 + 3)] + base, specs={which: "repeat"})
        _add(f"repeat table after a block without sequences: {which}", frame([first, blk], len(c.out)),
             c.blob(), 2)


def _repeat_offsets(rng):
    # RFC 8878 3.1.1.5: offset values 1-3 with and without literals, at the
    # frame's first sequence (history 1, 4, 8) and in a later block
    def build(first, lax=False):
        c = Content(lax)
        blocks = [c.raw(_rb(rng, 64))]
        # (a block before: the history is still 1, 4, 8 and offsets 4 and 8 have bytes to reach)
        blocks.append(c.block(_rb(rng, 40), first + [(3, 4, 20 + 3), (2, 5, 33 + 3), (1, 6, 47 + 3)]))
        later = [(2, 4, 1), (2, 4, 2), (2, 4, 3), (1, 3, 2), (0, 4, 1), (0, 4, 2), (0, 4, 3), (2, 3, 3),
                 (0, 5, 1), (0, 3, 3), (0, 3, 3), (1, 3, 1), (0, 3, 2), (4, 3, 2)]
        blocks.append(c.block(_rb(rng, 40), later))
        return blocks, c
    for ofv in (1, 2, 3):
        for ll in (2, 0):
            if ll == 0 and ofv == 3:
                continue  # rep[0] - 1 = 0: below
            blocks, c = build([(ll, 5, ofv)])
            _add(f"repeat offset value {ofv}, ll {ll}, first sequence", frame(blocks, len(c.out)), c.blob(), 0)
            bad = bytearray(c.blob())
            bad[64 + ll + 2] ^= 1
            _add(f"repeat offset value {ofv}, ll {ll}, first sequence, match byte wrong",
                 frame(blocks, len(c.out)), bad, 1)
    blocks, c = build([(0, 5, 3)], lax=True)
    _add("repeat offset resolving to 0", frame(blocks, len(c.out)), c.blob(), 2,
         "3.1.1.5 (an offset of 0 is a corrupted frame)")


def _matches(rng):
    # overlapping matches: offsets 1-17, lengths around the 16-byte step and
    # the lane / wave split, at output positions of every residue mod 4
    c, seqs, i = Content(), [], 0
    for off in range(1, 18):
        for ml in (3, 15, 16, 17, 255, 256, 257, 1000):
            seqs.append((17 + i % 4 if not seqs else i % 4 + (off > 8), ml, off + 3))
            i += 1
    lits = _rb(rng, sum(s[0] for s in seqs) + 5)
    blk = c.block(lits, seqs)
    blob = c.blob()
    pos = 0
    res = set()
    for ll, ml, _ in seqs:
        res.add(((pos + ll) % 4, ml))
        pos += ll + ml
    assert all((r, ml) in res for r in range(4) for ml in (3, 17, 257)), "a residue is missing"
    assert len(blob) <= BLOCK
    _add("overlapping matches, offsets 1-17", frame([blk], len(blob)), blob, 0)
    for at in (len(blob) // 3, len(blob) - 6):
        bad = bytearray(blob)
        bad[at] ^= 0x10
        _add(f"overlapping matches, byte {at} wrong", frame([blk], len(blob)), bad, 1)
    # ll + ml = 256 (a lane compares it) and 257 (the whole wave)
    for tot in (256, 257):
        for ll in (0, 1, 100, tot - 3):
            c = Content()
            b0 = c.raw(_rb(rng, 50))
            blk = c.block(_rb(rng, ll + 2), [(ll, tot - ll, 7 + 3)])
            blob = c.blob()
            _add(f"sequence of ll {ll} + ml {tot - ll}", frame([b0, blk], len(blob)), blob, 0)
            for at in sorted({50, 50 + ll, 50 + tot - 1}):
                bad = bytearray(blob)
                bad[at] ^= 0x80
                _add(f"sequence of ll {ll} + ml {tot - ll}, byte {at} wrong", frame([b0, blk], len(blob)),
                     bad, 1)
    # a match ending exactly at the blob's end; literals after the last sequence
    for rest in (0, 1, 3, 4, 5):
        c = Content()
        blk = c.block(_rb(rng, 30 + rest), [(30, 11, 9 + 3)])
        blob = c.blob()
        _add(f"{rest} literals after the last sequence", frame([blk], len(blob)), blob, 0)
        bad = bytearray(blob)
        bad[-1] ^= 1
        _add(f"{rest} literals after the last sequence, last byte wrong", frame([blk], len(blob)), bad, 1)
        _add(f"{rest} literals after the last sequence, blob cut", frame([blk], fcs_bytes=0, wd=0)
             if rest == 0 else frame([blk], len(blob)), blob[:-1], 1)


def _lax(rng):
    # where the libzstd at hand is lax and the checker follows the RFC
    c = Content()
    lits = _rb(rng, 60)
    seqs = [(10, 5, 7 + 3), (20, 9, 2), (3, 4, 30 + 3)]
    blk = c.block(lits, seqs, modes_low=1)
    _add("reserved bits of the modes byte", frame([blk], len(c.out)), c.blob(), 2,
         "3.1.1.3.2.1 (Reserved must be all-zeroes)")
    c = Content()
    blk = c.block(lits, seqs, pad=b"\x00")
    _add("an unread zero byte below the sequences bitstream", frame([blk], len(c.out)), c.blob(), 2,
         "3.1.1.3.2.2 (the bitstream ends when all sequences are decoded: no bits left)")
    c = Content()
    blk = c.block(lits, seqs)
    _add("the same block as written", frame([blk], len(c.out)), c.blob(), 0)


def _every_path(rng):
    """One frame of about 1.5 KiB of content that holds each compare path
    once: a raw block, an RLE block, compressed blocks with raw, RLE and
    Huffman literals, short matches, a match above 256 bytes, an overlapping
    offset-1 match and trailing literals."""
    c = Content()
    blocks = [c.raw(_rb(rng, 311)), c.rle(0xA5, 173)]
    blocks.append(c.block(_rb(rng, 97), [(13, 4, 50 + 3), (30, 19, 300 + 3), (0, 3, 1), (41, 7, 3 + 3)]))
    blocks.append(c.block(b"\x3c" * 45, [(20, 5, 100 + 3), (9, 33, 1 + 3)], lit_rle(0x3c, 45)))
    lits = _skew(rng, 450, 12, 48)
    blocks.append(c.block(lits, [(150, 301, 411 + 3), (70, 40, 1 + 3), (101, 6, 2)],
                          lit_huf(lits, huf_table(lits))))
    blob = c.blob()
    assert 1400 <= len(blob) <= 1700
    return frame(blocks, len(blob)), blob


def _libzstd_advanced(rng):
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9))).astype(np.uint8))
             for _ in range(400)]
    text = b" ".join(words[int(i)] for i in rng.integers(0, 400, 50000))[:200000]
    for tag, kw in (("checksum", dict(checksum=True)), ("no content size", dict(content_size=False)),
                    ("windowLog 10", dict(window_log=10)), ("windowLog 17", dict(window_log=17)),
                    ("checksum, no content size, windowLog 10",
                     dict(checksum=True, content_size=False, window_log=10))):
        fr = zr.compress_adv(text, 3, **kw)
        _add("libzstd advanced: " + tag, fr, text, 0)
        if "checksum" in kw:
            _add("libzstd advanced: " + tag + ", checksum bit flipped",
                 fr[:-1] + bytes([fr[-1] ^ 0x40]), text, 2)


def _block_parallel(rng):
    """Frames of 2 x 128 KiB + a tail in 128 KiB blocks: what the
    block-parallel pass places.  (name, frame, blob, status) records."""
    out = []
    tail = 3001
    c = Content()
    blocks = []
    for n in (BLOCK, BLOCK, tail):
        lits = _skew(rng, n - 2 * (n // 8) - n // 4, 24, 32)
        seqs = [(len(lits) // 4, n // 8, 5 + 3), (len(lits) // 4, n // 8, 1), (len(lits) // 4, n // 4, 77 + 3)]
        blocks.append(c.block(lits, seqs, lit_huf(lits, huf_table(lits))))
        assert blocks[-1][2] == n, (blocks[-1][2], n)
    blob = c.blob()
    out.append(("blocks of 128 KiB", frame(blocks, len(blob)), blob, 0))
    out.append(("blocks of 128 KiB, checksum", frame(blocks, len(blob), checksum=blob), blob, 0))
    out.append(("blocks of 128 KiB, wrong checksum", frame(blocks, len(blob), checksum=1), blob, 2))
    out.append(("blocks of 128 KiB, window 256 KiB", frame(blocks, len(blob), wd=window_desc(18)), blob, 0))
    out.append(("blocks of 128 KiB, window 256 KiB, no fcs", frame(blocks, fcs_bytes=0, wd=window_desc(18)),
                blob, 0))
    for k, at in enumerate((70000, BLOCK + 131000, 2 * BLOCK + 5)):
        bad = bytearray(blob)
        bad[at] ^= 2
        out.append((f"blocks of 128 KiB, a wrong byte in block {k}", frame(blocks, len(blob)), bad, 1))
    # a match reaching 150000 bytes back: inside a 256 KiB window, past a 128 KiB one
    c = Content()
    blocks = [c.raw(_rb(rng, BLOCK)), c.rle(0, BLOCK)]
    blocks.append(c.block(_rb(rng, tail - 100), [(50, 100, 150000 + 3)]))
    blob = c.blob()
    out.append(("offset 150000, window 256 KiB", frame(blocks, fcs_bytes=0, wd=window_desc(18)), blob, 0))
    c = Content()
    blocks = [c.raw(_rb(rng, BLOCK))] + [c.rle(k, BLOCK) for k in range(8)]
    blocks.append(c.block(_rb(rng, tail - 100), [(50, 100, 8 * BLOCK + 3)]))
    blob = c.blob()
    out.append(("offset 1 MiB, window 128 KiB", frame(blocks, fcs_bytes=0, wd=window_desc(17)), blob, 2))
    out.append(("offset 1 MiB, window 1 MiB", frame(blocks, fcs_bytes=0, wd=window_desc(20)), blob, 0))
    return out


def _build():
    rng = np.random.default_rng(8878)
    for part in (_headers, _checksums, _blocks, _window, _small_blocks, _literals, _huffman, _seq_codes,
                 _seq_counts, _seq_tables, _repeat_offsets, _matches, _lax, _libzstd_advanced):
        part(rng)
    global EVERY_PATH, BLOCK_PARALLEL
    EVERY_PATH = _every_path(rng)
    BLOCK_PARALLEL = _block_parallel(rng)
    _add("every compare path once", EVERY_PATH[0], EVERY_PATH[1], 0)
    for name, fr, blob, st in BLOCK_PARALLEL:
        _add(name, fr, blob, st)


EVERY_PATH = BLOCK_PARALLEL = None
_build()
