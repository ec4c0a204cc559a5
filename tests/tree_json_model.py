"""The grammar G_T of rcdc_tree_parse (include/rcdc.h) in plain Python, and
what the parse gives for a blob: the model the device parser is compared with.

``in_gt(data)`` -> whether the blob is inside G_T, by a hand-written
recogniser that reads bytes and knows nothing of ``json``.
``ids_of(data)`` -> (nodes, data ids, [(tree id, is_dir)]) over ``json.loads``:
the content ids of "file" nodes and every non-null subtree, in node order.
``collect(blobs)`` -> the statuses and arrays of a batch.
"""
import json

WS = b" \t\n\r"
HEX = b"0123456789abcdefABCDEF"
U32_MAX = (1 << 32) - 1
U64_MAX = (1 << 64) - 1
TYPES = (b"file", b"dir", b"symlink", b"dev", b"chardev", b"fifo", b"socket")
NULL_OR_U32 = (b"mode", b"uid", b"gid")
NULL_OR_STRING = (b"mtime", b"atime", b"ctime", b"user", b"group", b"linktarget_raw")
U64 = (b"inode", b"device_id", b"size", b"links", b"device")
NODE_KEYS = (b"name", b"type", b"linktarget", b"content", b"subtree",
             b"extended_attributes") + NULL_OR_U32 + NULL_OR_STRING + U64


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

    def key(self, allowed, seen) -> bytes:
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
        return k

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

    def uint(self, most: int) -> int:
        j = self.i
        while j < len(self.d) and 0x30 <= self.d[j] <= 0x39:
            j += 1
        t = self.d[self.i:j]
        if not t or (len(t) > 1 and t[0] == 0x30) or int(t) > most:
            raise _Outside("integer")
        self.i = j
        return int(t)

    def _tail(self, n: int, lo: int, hi: int) -> None:
        for k in range(n):
            c = self.peek()
            if not ((lo if k == 0 else 0x80) <= c <= (hi if k == 0 else 0xBF)):
                raise _Outside("utf-8")
            self.i += 1

    def string(self) -> None:
        """A string of G_T (Unicode 15, table 3-7 for the raw bytes)."""
        self.eat(b'"')
        while True:
            c = self.peek()
            if c < 0x20:
                raise _Outside("control byte or end of text in a string")
            self.i += 1
            if c == 0x22:
                return
            if c == 0x5C:
                e = self.peek()
                self.i += 1
                if e == 0x75:
                    h = self.d[self.i:self.i + 4]
                    if len(h) != 4 or any(x not in HEX for x in h):
                        raise _Outside("\\u")
                    if 0xD800 <= int(h, 16) <= 0xDFFF:
                        raise _Outside("surrogate")
                    self.i += 4
                elif e < 0 or e not in b'"\\/bfnrt':
                    raise _Outside("escape")
            elif c >= 0x80:
                if 0xC2 <= c <= 0xDF:
                    self._tail(1, 0x80, 0xBF)
                elif c == 0xE0:
                    self._tail(2, 0xA0, 0xBF)
                elif c == 0xED:
                    self._tail(2, 0x80, 0x9F)
                elif 0xE1 <= c <= 0xEF:
                    self._tail(2, 0x80, 0xBF)
                elif c == 0xF0:
                    self._tail(3, 0x90, 0xBF)
                elif 0xF1 <= c <= 0xF3:
                    self._tail(3, 0x80, 0xBF)
                elif c == 0xF4:
                    self._tail(3, 0x80, 0x8F)
                else:
                    raise _Outside("utf-8 lead byte")

    def null_or(self, what) -> None:
        if not self.at(b"null"):
            what()

    def xattr(self) -> None:
        seen = self.members((b"name", b"value"),
                            lambda k: self.string() if k == b"name" else self.null_or(self.string))
        if b"name" not in seen:
            raise _Outside("attribute without a name")

    def node(self) -> None:
        v = {}

        def member(k):
            if k in (b"name", b"linktarget"):
                self.string()
            elif k == b"type":
                for t in TYPES:
                    if self.at(b'"' + t + b'"'):
                        v[k] = t
                        return
                raise _Outside("type")
            elif k in NULL_OR_U32:
                self.null_or(lambda: self.uint(U32_MAX))
            elif k in NULL_OR_STRING:
                self.null_or(self.string)
            elif k in U64:
                self.uint(U64_MAX)
            elif k == b"content":
                self.null_or(lambda: self.array(self.id))
            elif k == b"subtree":
                if not self.at(b"null"):
                    self.id()
                    v[k] = True
            else:
                self.array(self.xattr)
        seen = self.members(NODE_KEYS, member)
        if not {b"name", b"type"} <= seen:
            raise _Outside("node lacks a key")
        if v[b"type"] == b"symlink" and b"linktarget" not in seen:
            raise _Outside("symlink without linktarget")
        if v[b"type"] == b"dir" and b"subtree" not in v:
            raise _Outside("dir without subtree")

    def root(self) -> None:
        self.ws()
        self.members((b"nodes",), lambda k: self.null_or(lambda: self.array(self.node)))
        self.ws()
        if self.i != len(self.d):
            raise _Outside("trailing bytes")


def in_gt(data: bytes) -> bool:
    try:
        _P(data).root()
        return True
    except (_Outside, IndexError):
        return False


def ids_of(data: bytes):
    """(nodes, [data id], [(tree id, is_dir)]) of a blob that is JSON of the
    tree shape: what the two loops of the reference read."""
    nodes = json.loads(bytes(data).decode("utf-8"))["nodes"] or []
    data_ids, tree_ids = [], []
    for n in nodes:
        if n["type"] == "file":
            data_ids += [bytes.fromhex(i) for i in n.get("content") or []]
        if n.get("subtree") is not None:
            tree_ids.append((bytes.fromhex(n["subtree"]), n["type"] == "dir"))
    return len(nodes), data_ids, tree_ids


class Collected:
    """What rcdc_tree_parse gives for a batch."""

    def __init__(self):
        self.status = []     # per blob: 0 parsed, 1 not parsed
        self.blobs = []      # per blob: (nodes, data_ids, tree_ids, data_start, tree_start)
        self.data_ids = []
        self.tree_ids = []
        self.is_dir = []
        self.nodes = 0


def collect(blobs) -> Collected:
    out = Collected()
    for data in blobs:
        d0, t0 = len(out.data_ids), len(out.tree_ids)
        if not in_gt(data):
            out.status.append(1)
            out.blobs.append((0, 0, 0, d0, t0))
            continue
        n, d, t = ids_of(data)
        out.status.append(0)
        out.blobs.append((n, len(d), len(t), d0, t0))
        out.data_ids += d
        out.tree_ids += [i for i, _ in t]
        out.is_dir += [int(f) for _, f in t]
        out.nodes += n
    return out
