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


# ---- a pattern of very many headers, expected by arithmetic ----------------------------

PATTERN = (b"", run([0]), run([1]), run([2, 2]))   # header i has shape i % 4 ...
PATTERN_BAD = b"\x04" + run([0])[1:]               # ... but every PATTERN_EVERY-th: a bad type byte
PATTERN_EVERY = 1000
_COUNT = np.array([0, 1, 1, 2])
_BLOBS = np.array([0, 100, 100, 100 + 107])        # the sum of a shape's blob lengths (``run``)


class Pattern:
    """``n`` headers back to back in one arena (``arena``, ``offs``,
    ``lens``), the first four bytes of every entry's id replaced by its
    header's number, and what rcdc_pack_header_parse gives for them by numpy
    arithmetic: ``records`` (the fields of a PK_HEADER as int64 arrays),
    ``ids[t]`` (n, 32) uint8 and ``locs[t]`` (n, 4) uint32 per type, ``packs``.
    tests/test_pack_header_host.py holds it to the model at a size the model
    handles; the device test runs it past 2^20 headers, where the model would
    take ten seconds."""

    def __init__(self, n, pack_base=(0, 0)):
        assert PATTERN_EVERY % 4 == 0
        i = np.arange(n)
        shape, bad = i % 4, i % PATTERN_EVERY == PATTERN_EVERY - 1
        self.lens = np.where(bad, len(PATTERN_BAD), np.array([len(p) for p in PATTERN])[shape])
        self.offs = np.cumsum(self.lens) - self.lens
        block = b"".join(PATTERN) * (PATTERN_EVERY // 4)
        block = block[:len(block) - len(PATTERN[3])] + PATTERN_BAD
        self.arena = np.tile(np.frombuffer(block, np.uint8), n // PATTERN_EVERY + 1)[:int(self.lens.sum())].copy()
        # an entry's id is its last 32 bytes; its first four bytes: the header's number
        stamp = i.astype("<u4").view(np.uint8).reshape(n, 4)
        for at, sel in ((5, (shape == 1) | (shape == 2) | bad), (9, (shape == 3) & ~bad),
                        (41 + 9, (shape == 3) & ~bad)):
            self.arena[(self.offs[sel] + at)[:, None] + np.arange(4)[None, :]] = stamp[sel]
        ok = ~bad
        tpe = np.where(ok & (shape == 2), 1, 0)
        count = np.where(ok, _COUNT[shape], 0)
        number, first = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.ids, self.locs, self.packs = [None, None], [None, None], [0, 0]
        for t in (0, 1):
            mine = ok & (tpe == t)
            number[mine] = pack_base[t] + np.arange(int(mine.sum()))
            first[mine] = np.cumsum(count[mine]) - count[mine]
            self.packs[t] = int(mine.sum())
            # the entries of type t in order: (header, which of its entries)
            h = np.repeat(i[mine], count[mine])
            k = np.arange(len(h)) - np.repeat(first[mine], count[mine])
            two = shape[h] == 3
            locs = np.zeros((len(h), 4), np.uint32)
            locs[:, 0] = number[h]
            locs[:, 1] = np.where(k == 1, 100, 0)
            locs[:, 2] = np.where(k == 1, 107, 100)
            locs[:, 3] = np.where(two, 1000 + k, 0)
            ids = np.empty((len(h), 32), np.uint8)
            ids[:] = np.frombuffer(bid(0), np.uint8)
            ids[k == 1] = np.frombuffer(bid(1), np.uint8)
            ids[:, :4] = stamp[h]
            self.ids[t], self.locs[t] = ids, locs
        z = np.zeros(n, np.int64)
        self.records = dict(
            status=np.where(bad, BAD_TYPE, OK), type=tpe, number=number, count=count, first=first,
            data=np.where(tpe == 0, count, 0), tree=np.where(tpe == 1, count, 0),
            size=np.where(ok, 32 + self.lens, 0),
            pack_size=np.where(ok, 36 + self.lens + _BLOBS[shape], 0), err_pos=z, err_entry=z)

    def headers(self):
        """The headers as bytes, for the model."""
        raw = self.arena.tobytes()
        return [raw[o:o + n] for o, n in zip(self.offs.tolist(), self.lens.tolist())]


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
