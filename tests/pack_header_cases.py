"""The case table of the pack header parser, shared by the host and the GPU
tests, and the builders of headers aimed at tile boundaries.  A case is
(name, header bytes, expected status); everything else about it comes from
tests/pack_header_model.py."""
import hashlib

import numpy as np

from tests.pack_header_model import BAD_TYPE, CUT_SHORT, OK, OVERFLOW, entry


def bid(name) -> bytes:
    return hashlib.sha256(f"blob:{name}".encode()).digest()


def run(types, lengths=None, ids=None, ulens=None) -> bytes:
    """Entries with these type bytes back to back."""
    out = b""
    for k, t in enumerate(types):
        out += entry(t, lengths[k] if lengths else 100 + 7 * k,
                     ids[k] if ids else bid(k), (ulens[k] if ulens else 1000 + k) if t >= 2 else 0)
    return out


def sized(sizes, type_bit=0, id_byte=None) -> bytes:
    """Entries of these sizes (37 or 41), all of one blob type; ``id_byte``:
    every id byte is that value."""
    ids = [bytes([id_byte]) * 32] * len(sizes) if id_byte is not None else None
    return run([type_bit + (2 if s == 41 else 0) for s in sizes], ids=ids)


def _table():
    t = []
    add = lambda name, header, status: t.append((name, bytes(header), status))
    add("empty", b"", OK)
    add("one data", run([0]), OK)
    add("one tree", run([1]), OK)
    add("one compressed data", run([2]), OK)
    add("one compressed tree", run([3]), OK)
    add("data pack", run([0, 2, 2, 0, 2, 0, 0, 2]), OK)
    add("tree pack", run([3, 1, 3, 3, 1]), OK)
    add("mixed, data first", run([0, 1, 3, 1, 1]), OK)
    add("mixed, tree first", run([3, 0, 2]), OK)
    add("uncompressed length 0 is kept as 0", run([2, 3], ulens=[0, 0]), OK)
    add("length 0 and length 2^32 - 1", run([0, 0], lengths=[0, 0xFFFFFFFF]), OK)
    add("ids of 0xFF", run([0, 2, 0], ids=[b"\xff" * 32] * 3), OK)
    add("ids of 0x04", run([1, 3, 1], ids=[b"\x04" * 32] * 3), OK)
    add("bad type at byte 0", b"\x04" + run([0])[1:], BAD_TYPE)
    add("bad type 0xFF behind two entries", run([0, 2]) + b"\xff" + run([0])[1:], BAD_TYPE)
    add("bad type in the last byte", run([0, 1]) + b"\x09", BAD_TYPE)   # before its size
    add("a lone type byte", b"\x00", CUT_SHORT)
    add("one byte behind an entry", run([0]) + b"\x02", CUT_SHORT)
    add("a 41-byte entry of 37 bytes", run([2])[:37], CUT_SHORT)
    add("a 37-byte entry of 36 bytes", run([2, 1])[:-1], CUT_SHORT)
    add("overflow: 2^31 twice", run([0, 0], lengths=[0x80000000] * 2), OVERFLOW)
    add("no overflow: 2^31 - 1 and 2^31", run([0, 0], lengths=[0x7FFFFFFF, 0x80000000]), OK)
    add("overflow behind many", run([0] * 40, lengths=[0x07000000] * 40), OVERFLOW)
    add("overflow by the last entry", run([1, 3], lengths=[0xFFFFFFFF, 1]), OVERFLOW)
    add("bad type wins over overflow", run([0, 0], lengths=[0x80000000] * 2) + b"\x05", BAD_TYPE)
    add("cut short wins over overflow", run([0, 0], lengths=[0x80000000] * 2) + b"\x01", CUT_SHORT)
    for cut in range(1, 41):  # a last entry cut at each of 1 to 40 bytes
        add(f"last entry of {cut} bytes", run([0, 3]) + run([2 if cut > 36 else cut % 4])[:cut],
            CUT_SHORT)
    return t


TABLE = _table()


def random_header(rng, n_max=80, bad=0.2) -> bytes:
    """Entries with random type bytes and lengths; now and then cut short or
    with a bad type byte somewhere."""
    n = int(rng.integers(0, n_max))
    types = rng.integers(0, 4, n).tolist()
    h = run(types, lengths=rng.integers(0, 1 << 20, n).tolist(),
            ids=[rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)])
    r = rng.random()
    if r < bad / 2 and h:
        h = h[:int(rng.integers(1, len(h)))]       # most likely cut short
    elif r < bad and h:
        starts = np.cumsum([0] + [41 if t >= 2 else 37 for t in types])[:-1]
        p = int(starts[int(rng.integers(0, n))])
        h = h[:p] + bytes([int(rng.integers(4, 256))]) + h[p + 1:]
    return h


# ---- aimed at tile boundaries ---------------------------------------------------------

def sizes_to(total: int):
    """37s and 41s that sum to ``total`` (every total from 36 * 40 up has some)."""
    for b in range(total // 41 + 1):
        if (total - 41 * b) % 37 == 0:
            a = (total - 41 * b) // 37
            return [37] * a + [41] * b
    raise ValueError(total)


def straddle(tile: int, phase: int, id_byte=None) -> bytes:
    """A header (to lie at a 16-byte boundary) with a 41-byte entry over its
    first tile boundary, so that the second tile's first entry starts
    ``phase`` (0..40) bytes into it (phase 0: the entry ends on the
    boundary), and three entries more."""
    return sized(sizes_to(tile + phase - 41) + [41, 37, 41, 37], id_byte=id_byte)


def phase_walk(tile: int, tiles: int) -> bytes:
    """A run of 37-byte entries over ``tiles`` tiles: as 37 does not divide the
    tile, the phase differs from tile to tile."""
    return sized([37] * (tile * tiles // 37))
