"""The grammar G of rcdc_index_parse (include/rcdc.h) in plain Python, and the
collector's rule over what it accepts: the model the device parser and
``DeviceIndex.extend`` are both compared with.

``parse(data)`` -> None (outside G: NOT_PARSED) or (packs, n_delete), a pack
being (id, [(id, type, offset, length, ulen or 0), ...], size or None).
``collect(files, pack_base)`` -> the statuses and per-type arrays of a batch.
"""
WS = b" \t\n\r"
HEX = b"0123456789abcdefABCDEF"
U32_MAX = (1 << 32) - 1


class _Outside(Exception):
    pass


class _P:
    def __init__(self, data: bytes):
        self.d, self.i = bytes(data), 0

    def peek(self) -> int:
        return self.d[self.i] if self.i < len(self.d) else -1

    def ws(self) -> None:
        while self.i < len(self.d) and self.d[self.i] in WS:
            self.i += 1

    def eat(self, c: bytes) -> None:
        if self.d[self.i:self.i + len(c)] != c:
            raise _Outside(f"expected {c!r} at {self.i}")
        self.i += len(c)

    def at(self, c: bytes) -> bool:
        if self.d[self.i:self.i + len(c)] == c:
            self.i += len(c)
            return True
        return False

    def key(self, allowed, seen) -> str:
        """A key string: one of ``allowed``, literally, not seen before."""
        self.eat(b'"')
        end = self.d.find(b'"', self.i)
        if end < 0:
            raise _Outside("unterminated key")
        k = self.d[self.i:end]
        if k not in allowed or k in seen:
            raise _Outside(f"key {k!r}")
        seen.add(k)
        self.i = end + 1
        self.ws()
        self.eat(b":")
        self.ws()
        return k.decode()

    def members(self, allowed, member) -> set:
        """'{' members '}' with ``member(key)`` parsing each value."""
        self.eat(b"{")
        self.ws()
        seen = set()
        while True:
            member(self.key(allowed, seen))
            self.ws()
            if self.at(b","):
                self.ws()
                continue
            self.eat(b"}")
            return seen

    def array(self, item) -> list:
        self.eat(b"[")
        self.ws()
        out = []
        if self.at(b"]"):
            return out
        while True:
            out.append(item())
            self.ws()
            if self.at(b"]"):
                return out
            self.eat(b",")
            self.ws()

    def id(self) -> bytes:
        self.eat(b'"')
        h = self.d[self.i:self.i + 64]
        if len(h) != 64 or any(c not in HEX for c in h):
            raise _Outside("id")
        self.i += 64
        self.eat(b'"')
        return bytes.fromhex(h.decode())

    def uint(self) -> int:
        j = self.i
        while j < len(self.d) and 0x30 <= self.d[j] <= 0x39:
            j += 1
        t = self.d[self.i:j]
        if not t or (len(t) > 1 and t[0] == 0x30) or int(t) > U32_MAX:
            raise _Outside("integer")
        self.i = j
        return int(t)

    def time(self) -> None:
        if self.at(b"null"):
            return
        self.eat(b'"')
        while True:
            c = self.peek()
            if c == 0x22:
                break
            if c < 0x20 or c > 0x7E or c == 0x5C:
                raise _Outside("time")
            self.i += 1
        self.eat(b'"')

    def blob(self):
        v = {"uncompressed_length": 0}

        def member(k):
            if k == "id":
                v[k] = self.id()
            elif k == "type":
                if self.at(b'"data"'):
                    v[k] = 0
                elif self.at(b'"tree"'):
                    v[k] = 1
                else:
                    raise _Outside("type")
            elif k == "uncompressed_length":
                if not self.at(b"null"):
                    v[k] = self.uint()
                    if v[k] == 0:
                        raise _Outside("uncompressed_length 0")
            else:
                v[k] = self.uint()
        seen = self.members((b"id", b"type", b"offset", b"length", b"uncompressed_length"), member)
        if not {b"id", b"type", b"offset", b"length"} <= seen:
            raise _Outside("blob lacks a key")
        return v["id"], v["type"], v["offset"], v["length"], v["uncompressed_length"]

    def pack(self):
        v = {"size": None}

        def member(k):
            if k == "id":
                v[k] = self.id()
            elif k == "blobs":
                v[k] = self.array(self.blob)
            elif k == "time":
                self.time()
            elif not self.at(b"null"):
                v[k] = self.uint()
        seen = self.members((b"id", b"blobs", b"time", b"size"), member)
        if not {b"id", b"blobs"} <= seen:
            raise _Outside("pack lacks a key")
        return v["id"], v["blobs"], v["size"]

    def root(self):
        v = {"packs_to_delete": []}

        def member(k):
            if k == "supersedes":
                if not self.at(b"null"):
                    self.array(self.id)
            else:
                v[k] = self.array(self.pack)
        self.ws()
        seen = self.members((b"supersedes", b"packs", b"packs_to_delete"), member)
        if b"packs" not in seen:
            raise _Outside("no packs")
        self.ws()
        if self.i != len(self.d):
            raise _Outside("trailing bytes")
        return v["packs"], len(v["packs_to_delete"])


def parse(data: bytes):
    """None for a file outside G, else (packs, number of packs_to_delete)."""
    if b"\\" in data:
        return None
    try:
        return _P(data).root()
    except (_Outside, IndexError):
        return None


def pack_size(blobs, size):
    """index.IndexPack.pack_size (indexfile.rs:108-112)."""
    if size is not None:
        return size
    return sum(b[3] + (41 if b[4] else 37) for b in blobs) + 36


class Collected:
    """What rcdc_index_parse gives for a batch."""

    def __init__(self):
        self.status = []        # per file: 0 parsed, 1 not parsed
        self.files = []         # per file: (packs[2], packs_to_delete, entries[2])
        self.packs = []         # collected packs in order: (id, type, number, size)
        self.ids = ([], [])     # per type
        self.locs = ([], [])    # per type: (pack number, offset, length, ulen)


def collect(files, pack_base=(0, 0)) -> Collected:
    """The collector's rule (binarysorted.rs:127-163, DeviceIndex.extend) over
    the files of a batch that are in G; the others contribute nothing."""
    out = Collected()
    nxt = list(pack_base)
    for data in files:
        r = parse(data)
        if r is None:
            out.status.append(1)
            out.files.append(((0, 0), 0, (0, 0)))
            continue
        packs, ndel = r
        np_, ne = [0, 0], [0, 0]
        for pid, blobs, size in packs:
            t = blobs[0][1] if blobs else 0
            out.packs.append((pid, t, nxt[t], pack_size(blobs, size)))
            for b in blobs:
                out.ids[t].append(b[0])
                out.locs[t].append((nxt[t], b[2], b[3], b[4]))
            nxt[t] += 1
            np_[t] += 1
            ne[t] += len(blobs)
        out.status.append(0)
        out.files.append((tuple(np_), ndel, tuple(ne)))
    return out
