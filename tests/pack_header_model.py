"""A plain-Python model of rcdc_pack_header_parse (include/rcdc.h), shared by
the host and the GPU tests: ``pack.parse_header``'s rule written down once
more, plus the overflow rule, the collector's typing and numbering and the
two sizes of PackHeaderRef."""
import struct
from typing import List, NamedTuple, Tuple

OK, BAD_TYPE, CUT_SHORT, OVERFLOW = 0, 1, 2, 3


def entry(type_byte: int, length: int, id_: bytes, ulen: int = 0) -> bytes:
    """One header entry: 37 bytes for type bytes 0 / 1, 41 for 2 / 3 (and for
    any other type byte the layout of its low bit 1, to craft bad ones)."""
    assert len(id_) == 32
    if type_byte in (0, 1):
        return bytes([type_byte]) + struct.pack("<I", length) + id_
    return bytes([type_byte]) + struct.pack("<II", length, ulen) + id_


class Judged(NamedTuple):
    status: int
    err_entry: int
    err_pos: int
    entries: List[Tuple[int, int, int, int, bytes]]  # (blob type, offset, length, ulen, id)


def judge(header: bytes) -> Judged:
    pos, off, out = 0, 0, []
    while pos < len(header):
        t = header[pos]
        if t > 3:  # before the size
            return Judged(BAD_TYPE, len(out), pos, [])
        size = 41 if t >= 2 else 37
        if pos + size > len(header):
            return Judged(CUT_SHORT, len(out), pos, [])
        length, = struct.unpack_from("<I", header, pos + 1)
        ulen = struct.unpack_from("<I", header, pos + 5)[0] if t >= 2 else 0
        out.append((t & 1, off, length, ulen, header[pos + size - 32:pos + size]))
        off += length
        pos += size
    if off > 0xFFFFFFFF:  # offsets only grow: some running offset exceeds u32 iff the last does
        return Judged(OVERFLOW, 0, 0, [])
    return Judged(OK, 0, 0, out)


class Record(NamedTuple):
    status: int
    type: int
    number: int
    count: int
    first: int
    data: int
    tree: int
    size: int
    pack_size: int
    err_pos: int
    err_entry: int


class Collected:
    def __init__(self):
        self.records: List[Record] = []
        self.ids = ([], [])    # per type: 32 bytes per entry
        self.locs = ([], [])   # per type: (pack number, offset, length, ulen)
        self.packs = [0, 0]

    @property
    def status(self):
        return [r.status for r in self.records]


def collect(headers, pack_base=(0, 0)) -> Collected:
    """What one rcdc_pack_header_parse call over ``headers`` gives."""
    c = Collected()
    for h in headers:
        j = judge(bytes(h))
        if j.status != OK:
            c.records.append(Record(j.status, 0, 0, 0, 0, 0, 0, 0, 0, j.err_pos, j.err_entry))
            continue
        t = j.entries[0][0] if j.entries else 0
        number = pack_base[t] + c.packs[t]
        c.packs[t] += 1
        tree = sum(e[0] for e in j.entries)
        c.records.append(Record(OK, t, number, len(j.entries), len(c.ids[t]),
                                len(j.entries) - tree, tree, 32 + len(h),
                                36 + len(h) + sum(e[2] for e in j.entries), 0, 0))
        for _, off, length, ulen, id_ in j.entries:
            c.ids[t].append(id_)
            c.locs[t].append((number, off, length, ulen))
    return c
