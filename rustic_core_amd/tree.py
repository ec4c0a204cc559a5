"""The used blobs of a repository on the device: tree blobs parsed in HBM
(rcdc_tree_parse in include/rcdc.h) and the walk over every snapshot's tree.

Reference: ``find_used_blobs`` (commands/prune.rs:1582-1632) -- what ``prune``
needs before its plan and all of ``check``'s ``check_trees`` -- over
``TreeStreamerOnce`` (blob/tree.rs:618-800): every tree blob of the
repository is looked up in the index (``Tree::from_backend``,
blob/tree.rs:137-163), read, opened, decoded and parsed; every ``content`` id
of a file node and every ``subtree`` id of a dir node goes into one set, and
every ``subtree`` of any node is followed once.

Here a level of the walk is one batch: ``DeviceIndex.lookup`` answers
``get_tree``, ``read.read_blobs`` opens and decodes the blobs, ``parse_trees``
reads the ids out of their text, and two id-only ``rcdc_dindex`` sets keep
"followed once" and "inserted once".  Ids cross to the host only as the
lookup hits the pack reads need; the result is a device tensor, which is what
``PrunePlan.from_entries(used_ids=...)`` takes.  A blob outside the device's
grammar goes through ``parse_tree_host``.

``parse_tree_nodes`` (rcdc_tree_nodes) is the same parse with a record per
node, and ``tree_names`` (rcdc_tree_names) gathers raw names by node index:
what ``check.check_trees`` judges a level from without the text leaving HBM.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
from typing import Callable, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import ErrorKind, RusticError, status_error

OK, NOT_PARSED = 0, 1  # RCDC_TRPARSE_OK / RCDC_TRPARSE_NOT_PARSED
# rcdc_trparse_ref / rcdc_trparse_blob as numpy records
TR_REF = np.dtype([("off", "<u8"), ("len", "<u8")])
TR_BLOB = np.dtype([("status", "<u4"), ("nodes", "<u4"), ("data_ids", "<u4"), ("tree_ids", "<u4"),
                    ("data_start", "<u8"), ("tree_start", "<u8")])
# rcdc_trnode / rcdc_trnodes_blob (rcdc_tree_nodes)
TR_NODE = np.dtype([("name_off", "<u8"), ("name_len", "<u4"), ("blob", "<u4"),
                    ("data_start", "<u4"), ("n_content", "<u4"), ("tree_index", "<u4"),
                    ("type", "u1"), ("flags", "u1"), ("pad", "<u2")])
TR_NODES_BLOB = np.dtype(TR_BLOB.descr + [("node_start", "<u8")])
NODE_CONTENT, NODE_SUBTREE, NODE_NAME_ESC = 1, 2, 4  # RCDC_TRNODE_*
DESERIALIZE_MESSAGE = "Failed to deserialize tree from JSON."  # blob/tree.rs:156
NODE_TYPES = ("file", "dir", "symlink", "dev", "chardev", "fifo", "socket")
DEFAULT_BUDGET = 1 << 30

_U32 = ("mode", "uid", "gid")                                     # Option<u32>
_STRINGS = ("mtime", "atime", "ctime", "user", "group")           # Option<..> from a string
_U64 = ("inode", "device_id", "size", "links")                    # u64, default 0


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


def parse_tile() -> int:
    """The tile size of the device's structural pass (RCDC_TRPARSE_TILE)."""
    return int(_lib.lib().rcdc_tree_parse_tile())


def parse_bound(length: int) -> Tuple[int, int, int]:
    """(content ids, subtree ids, nodes) that ``length`` bytes of tree JSON
    hold at most."""
    d, t, n = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.lib().rcdc_tree_parse_bound(int(length), ctypes.byref(d), ctypes.byref(t), ctypes.byref(n))
    return int(d.value), int(t.value), int(n.value)


class ParsedTrees:
    """rcdc_tree_parse's outputs: ``data_ids`` (n, 32) uint8, ``tree_ids``
    (m, 32) uint8 and ``tree_is_dir`` (m,) uint8 device tensors (None where
    not asked for), cut to the rows that were written; the counts
    ``n_data_ids``, ``n_tree_ids`` and ``nodes`` (also where the ids were only
    counted); ``blobs`` (TR_BLOB) on the host.  From rcdc_tree_nodes
    (``parse_tree_nodes``) also ``node_records``, a (nodes, 32) uint8 device
    tensor of TR_NODE records, and ``blobs`` is TR_NODES_BLOB."""

    def __init__(self, data_ids, tree_ids, tree_is_dir, blobs, n_data_ids, n_tree_ids, nodes, raw,
                 node_records=None):
        self.data_ids, self.tree_ids, self.tree_is_dir = data_ids, tree_ids, tree_is_dir
        self.blobs, self.nodes = blobs, nodes
        self.n_data_ids, self.n_tree_ids = n_data_ids, n_tree_ids
        self.raw = raw  # the flat allocations behind the arrays, guard bytes included
        self.node_records = node_records

    def nodes_host(self) -> np.ndarray:
        """The node records as a TR_NODE array on the host."""
        return self.node_records.cpu().numpy().reshape(-1).view(TR_NODE)


def parse_trees(d_text, offs, lens, device: int = 0, want=(True, True), guard: int = 0,
                caps=None) -> ParsedTrees:
    """The tree blobs ``d_text[offs[i] : offs[i] + lens[i]]`` (a uint8 device
    tensor, any alignment) parsed on the device.  ``want``: (content ids,
    subtree ids); what is not wanted is counted only.  ``guard``: that many
    bytes of 0xA5 behind every output array (in ``raw``), and ``caps``: the
    (content, subtree) capacities instead of the bound's, both for tests."""
    return _parse(d_text, offs, lens, device, want, guard, caps, False)


def parse_tree_nodes(d_text, offs, lens, device: int = 0, want=(True, True), guard: int = 0,
                     caps=None) -> ParsedTrees:
    """``parse_trees`` by rcdc_tree_nodes: the grammar is G_N (a dir node may
    lack its subtree), the id arrays are the same, and ``node_records`` holds
    one TR_NODE per node of every OK blob.  ``caps``: (content, subtree, node)
    capacities."""
    return _parse(d_text, offs, lens, device, want, guard, caps, True)


def _parse(d_text, offs, lens, device, want, guard, caps, with_nodes: bool) -> ParsedTrees:
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    n = len(lens)
    if len(offs) != n:
        raise RusticError(ErrorKind.InvalidInput, "one offset per length")
    if not (hasattr(d_text, "data_ptr") and str(d_text.dtype) == "torch.uint8"
            and d_text.dim() == 1 and d_text.is_contiguous() and d_text.device == dev):
        raise RusticError(ErrorKind.InvalidInput,
                          f"d_text must be a contiguous uint8 tensor on {dev}")
    refs = np.zeros(n, TR_REF)
    refs["off"], refs["len"] = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
    ln = refs["len"].astype(np.uint64)
    cap_d = int(((ln + np.uint64(1)) // np.uint64(67)).sum())
    cap_t = int(((ln + np.uint64(1)) // np.uint64(102)).sum())
    cap_n = int(((ln + np.uint64(1)) // np.uint64(25)).sum())
    if caps is not None:
        cap_d, cap_t = int(caps[0]), int(caps[1])
        cap_n = int(caps[2]) if len(caps) > 2 else cap_n
    blobs = np.zeros(n, TR_NODES_BLOB if with_nodes else TR_BLOB)
    result = _lib.TrparseResult()
    raw = []

    def alloc(nbytes):
        flat = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev) if guard \
            else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        raw.append(flat)
        return flat[:nbytes]
    with torch.cuda.device(dev):
        data = alloc(cap_d * 32).view(cap_d, 32) if want[0] else None
        tree = alloc(cap_t * 32).view(cap_t, 32) if want[1] else None
        is_dir = alloc(cap_t) if want[1] else None
        ptr = lambda a: None if a is None else a.data_ptr()
        head = (_ctx(int(device)).handle, d_text.data_ptr() if d_text.numel() else None,
                int(d_text.numel()), refs.ctypes.data, n, ptr(data), cap_d, ptr(tree), ptr(is_dir),
                cap_t)
        tail = (blobs.ctypes.data, ctypes.byref(result),
                int(torch.cuda.current_stream(dev).cuda_stream))
        if with_nodes:
            records = alloc(cap_n * 32).view(cap_n, 32)
            _check(_lib.lib().rcdc_tree_nodes(*head, records.data_ptr(), cap_n, *tail))
        else:
            records = None
            _check(_lib.lib().rcdc_tree_parse(*head, *tail))
    nd, nt, nn = int(result.data_ids), int(result.tree_ids), int(result.nodes)
    return ParsedTrees(None if data is None else data[:nd], None if tree is None else tree[:nt],
                       None if is_dir is None else is_dir[:nt], blobs, nd, nt, nn, raw,
                       None if records is None else records[:nn])


def tree_names(d_text, node_records, d_index, device: int = 0, guard: int = 0):
    """rcdc_tree_names: the raw names of the nodes ``d_index`` (an int32 or
    uint32 device tensor of indices into ``node_records``) out of the arena
    ``d_text``, back to back.  Returns (offsets, names): an int64 device
    tensor of len(d_index) + 1 entries and a uint8 device tensor.  ``guard``:
    that many bytes of 0xA5 behind the names, for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    n = int(d_index.shape[0])
    with torch.cuda.device(dev):
        d_index = d_index.to(torch.int32).contiguous()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        total = ctypes.c_uint64(0)
        cap = 32 * n + 256
        while True:
            flat = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=dev)
            _check(_lib.lib().rcdc_tree_names(
                _ctx(int(device)).handle, d_text.data_ptr() if d_text.numel() else None,
                int(d_text.numel()), node_records.data_ptr() if node_records.numel() else None,
                int(node_records.shape[0]), d_index.data_ptr() if n else None, n,
                offsets.data_ptr(), flat.data_ptr(), cap, ctypes.byref(total),
                int(torch.cuda.current_stream(dev).cuda_stream)))
            if int(total.value) <= cap:
                break
            cap = int(total.value)  # the offsets are written: come again with room
    return offsets, (flat if guard else flat[:int(total.value)])


# ---- the host rule ------------------------------------------------------------

def _fail(why: str):
    return RusticError(ErrorKind.Internal, f"{DESERIALIZE_MESSAGE} ({why})")


def _pairs(pairs):
    """An object's members; a repeated key is serde's "duplicate field"."""
    o = {}
    for k, v in pairs:
        if k in o:
            raise ValueError(f"duplicate field `{k}`")
        o[k] = v
    return o


def _id(x) -> bytes:
    if not isinstance(x, str) or len(x) != 64:
        raise ValueError("an id is a string of 64 hex digits")
    return bytes.fromhex(x)


def _uint(x, bits: int) -> None:
    if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < (1 << bits):
        raise ValueError(f"not a u{bits}")


class TreeNode(NamedTuple):
    """What check_trees (commands/check.rs:627-700) reads of a node."""
    name: str
    type: str                       # one of NODE_TYPES
    content: Optional[List[bytes]]  # None: the node has no content
    subtree: Optional[bytes]


def parse_tree_nodes_host(text: bytes) -> List[TreeNode]:
    """The nodes of one tree blob by ``parse_tree_host``'s rule, in order,
    with their names: what ``check.check_trees`` judges.  A dir node without
    a subtree is returned with ``subtree=None`` (check reports it as
    NoSubTree; ``parse_tree_host`` raises there); everything else that does
    not parse raises as it does there."""
    try:
        root = json.loads(bytes(text).decode("utf-8"), object_pairs_hook=_pairs)
        if not isinstance(root, dict) or "nodes" not in root:
            raise ValueError("missing field `nodes`")
        nodes = root["nodes"] if root["nodes"] is not None else []
        if not isinstance(nodes, list):
            raise ValueError("nodes is no sequence")
        out = []
        for n in nodes:
            _check_node(n)
            content = n.get("content")
            out.append(TreeNode(n["name"], n["type"],
                                None if content is None else [_id(i) for i in content],
                                None if n.get("subtree") is None else _id(n["subtree"])))
        return out
    except (ValueError, TypeError, RecursionError) as e:
        raise _fail(str(e)) from e


def _check_node(n) -> None:
    """Node's deserialiser but for ``content`` and ``subtree``."""
    if not isinstance(n, dict) or not isinstance(n.get("name"), str):
        raise ValueError("a node is a map with a name")
    tpe = n.get("type")
    if tpe not in NODE_TYPES:
        raise ValueError(f"unknown variant `{tpe}`")
    if tpe == "symlink" and not isinstance(n.get("linktarget"), str):
        raise ValueError("missing field `linktarget`")
    for k in _U32:
        if n.get(k) is not None:
            _uint(n[k], 32)
    for k in _STRINGS + ("linktarget_raw",):
        if n.get(k) is not None and not isinstance(n[k], str):
            raise ValueError(f"{k} is no string")
    for k in _U64 + ("device",):
        if k in n:
            _uint(n[k], 64)
    for x in n.get("extended_attributes", []):
        if not isinstance(x, dict) or not isinstance(x.get("name"), str) or \
                not isinstance(x.get("value"), (str, type(None))):
            raise ValueError("extended attribute")
    content = n.get("content")
    if content is not None and not isinstance(content, list):
        raise ValueError("content is no sequence")


def parse_tree_host(text: bytes):
    """One tree blob by the host rule: ``json.loads`` plus what ``Node``'s
    deserialiser requires (backend/node.rs:78-110: ``name`` and ``type``, the
    fields' kinds, ``linktarget`` for a symlink; keys it does not know are
    skipped, as serde does).  Returns (nodes, [content id of file nodes],
    [(subtree id, is dir)]).  What does not parse raises ErrorKind.Internal
    "Failed to deserialize tree from JSON." (blob/tree.rs:153-160); a dir
    node without a subtree, which find_used_blobs unwraps, raises it too."""
    try:
        root = json.loads(bytes(text).decode("utf-8"), object_pairs_hook=_pairs)
        if not isinstance(root, dict) or "nodes" not in root:
            raise ValueError("missing field `nodes`")
        nodes = root["nodes"] if root["nodes"] is not None else []
        if not isinstance(nodes, list):
            raise ValueError("nodes is no sequence")
        data_ids, tree_ids = [], []
        for n in nodes:
            if not isinstance(n, dict) or not isinstance(n.get("name"), str):
                raise ValueError("a node is a map with a name")
            tpe = n.get("type")
            if tpe not in NODE_TYPES:
                raise ValueError(f"unknown variant `{tpe}`")
            if tpe == "symlink" and not isinstance(n.get("linktarget"), str):
                raise ValueError("missing field `linktarget`")
            for k in _U32:
                if n.get(k) is not None:
                    _uint(n[k], 32)
            for k in _STRINGS + ("linktarget_raw",):
                if n.get(k) is not None and not isinstance(n[k], str):
                    raise ValueError(f"{k} is no string")
            for k in _U64 + ("device",):
                if k in n:
                    _uint(n[k], 64)
            for x in n.get("extended_attributes", []):
                if not isinstance(x, dict) or not isinstance(x.get("name"), str) or \
                        not isinstance(x.get("value"), (str, type(None))):
                    raise ValueError("extended attribute")
            content = n.get("content")
            if content is not None and not isinstance(content, list):
                raise ValueError("content is no sequence")
            ids = [_id(i) for i in content or []]
            if tpe == "file":
                data_ids += ids
            if n.get("subtree") is not None:
                tree_ids.append((_id(n["subtree"]), tpe == "dir"))
            elif tpe == "dir":
                raise ValueError("a dir node without a subtree")
        return len(nodes), data_ids, tree_ids
    except (ValueError, TypeError, RecursionError) as e:
        raise _fail(str(e)) from e


# ---- snapshots ------------------------------------------------------------------

def snapshot_trees(key, sealed_snapshot_files: Iterable[bytes], ignore=(),
                   device: Optional[int] = 0, decode: Optional[Callable] = None) -> List[bytes]:
    """The ``tree`` id of every snapshot file (prune.rs:1590-1601).  A file's
    id is the SHA-256 of its sealed bytes; ids in ``ignore`` are left out, as
    ``ignore_snaps`` is there.  Each file goes through ``decrypt_file``
    (backend/decrypt.rs:421-439): opened with ``key``, then its own text or
    ``2`` and a zstd frame.  Snapshot files are a few hundred bytes; this is
    host code around ``key.decrypt_data`` and ``decode`` (a callable from a
    frame to its bytes; None: ``compress.decode_all`` on ``device``)."""
    from .dindex import UNSUPPORTED_MESSAGE
    ignore = {bytes(i) for i in ignore}
    out = []
    for sealed in sealed_snapshot_files:
        sealed = bytes(sealed)
        if hashlib.sha256(sealed).digest() in ignore:
            continue
        plain = key.decrypt_data(sealed)
        if plain[:1] in (b"{", b"["):
            text = plain
        elif plain[:1] == b"\x02":
            text = _decode(plain[1:], device, decode)
        else:
            raise RusticError(ErrorKind.Unsupported, UNSUPPORTED_MESSAGE)
        try:
            out.append(_id(json.loads(text)["tree"]))
        except (ValueError, TypeError, KeyError) as e:
            raise RusticError(ErrorKind.Internal,
                              f"Failed to deserialize snapshot from JSON. ({e})") from e
    return out


def _decode(frame: bytes, device, decode) -> bytes:
    if decode is not None:
        return decode(frame)
    from .compress import decode_all
    return decode_all(frame, 0 if device is None else int(device))


# ---- the walk ---------------------------------------------------------------------

def _not_found(tree_id: bytes) -> RusticError:  # blob/tree.rs:144-149
    return RusticError(ErrorKind.Internal, f"Tree ID `{bytes(tree_id).hex()}` not found in index")


def _distinct(ids: Sequence[bytes]) -> List[bytes]:
    seen, out = set(), []
    for i in ids:
        i = bytes(i)
        if len(i) != 32:
            raise RusticError(ErrorKind.InvalidInput, "a tree id has 32 bytes")
        if i not in seen:
            seen.add(i)
            out.append(i)
    return out


class _IdSet:
    """An id-only rcdc_dindex: ``take`` is first_new + add, the rows of a
    batch that the set did not hold and that no earlier selected row of the
    batch equals."""

    def __init__(self, device: int):
        import torch
        from .crypto import _ctx
        self._torch, self._dev = torch, torch.device("cuda", device)
        self._h = ctypes.c_void_p()
        _check(_lib.lib().rcdc_dindex_create(_ctx(device).handle, 0, ctypes.byref(self._h)))

    def close(self) -> None:
        if self._h is not None:
            _lib.lib().rcdc_dindex_destroy(self._h)
            self._h = None

    def take(self, ids, select=None):
        """``ids``: (n, 32) uint8 device tensor; ``select``: n flags (uint8)
        or None for all.  Returns the new rows in order, now in the set."""
        return self.take_flags(ids, select)[0]

    def take_flags(self, ids, select=None):
        """``take``, and with the rows their flags: n uint8, 1 where the row
        is one of those returned."""
        torch = self._torch
        n = int(ids.shape[0])
        if not n:
            return ids[:0], torch.empty(0, dtype=torch.uint8, device=self._dev)
        ids = ids.contiguous()
        if ids.data_ptr() % 16:
            ids = ids.clone()
        with torch.cuda.device(self._dev):
            s = int(torch.cuda.current_stream(self._dev).cuda_stream)
            new = torch.empty(n, dtype=torch.uint8, device=self._dev)
            sel = None if select is None else select.contiguous()
            _check(_lib.lib().rcdc_dindex_first_new(self._h, ids.data_ptr(), n,
                                                    None if sel is None else sel.data_ptr(),
                                                    new.data_ptr(), s))
            fresh = ids[new != 0].contiguous()
            if int(fresh.shape[0]):
                _check(_lib.lib().rcdc_dindex_add(self._h, fresh.data_ptr(), None,
                                                  int(fresh.shape[0]), 1, s))  # DEVICE_PTRS
        return fresh, new


def _level_reads(index, frontier_host: np.ndarray, hits: np.ndarray):
    """restore.py's PackReads for the tree blobs of a level, in the restore
    info's order (pack id, offset) with neighbours coalesced; a blob's
    destination is its place in the frontier."""
    from .dindex import COL_ENTRY, COL_LENGTH, COL_OFFSET, COL_PACK, COL_ULEN, MISS, NO_PACK, TREE
    from .restore import BlobLocation, PackRead, coalesce
    missing = np.nonzero((hits[:, COL_ENTRY] == MISS) | (hits[:, COL_PACK] == NO_PACK))[0]
    if len(missing):
        raise _not_found(frontier_host[int(missing[0])].tobytes())
    packs = index.packs(TREE)
    rows = sorted((packs[int(h[COL_PACK])], int(h[COL_OFFSET]), int(h[COL_LENGTH]),
                   int(h[COL_ULEN]), j) for j, h in enumerate(hits))
    reads: list = []
    for pack_id, off, ln, ul, j in rows:
        cur = PackRead(pack_id, None, off, ln, [(BlobLocation(off, ln, ul), [j])])
        merged = coalesce(reads[-1], cur) if reads else None
        if merged is not None:
            reads[-1] = merged
        else:
            reads.append(cur)
    return reads


def _load_group(group, read_partial, dev):
    """The pack parts of a group in one device buffer, 16-aligned (what
    restore_contents does with them); returns (tensor, [(read, offset)])."""
    import torch
    parts, total = [], 0
    for r in group:
        parts.append((r, total))
        total = (total + r.length + 15) // 16 * 16
    raw = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    host, tensors = None, []
    for r, o in parts:
        got = read_partial(r.pack_id, r.offset, r.length)
        n = int(got.numel()) if hasattr(got, "numel") else len(got)
        if n != r.length:
            raise RusticError(ErrorKind.InputOutput,
                              f"read_partial returned {n} of {r.length} bytes of pack "
                              f"`{bytes(r.pack_id).hex()}`")
        if hasattr(got, "data_ptr"):
            tensors.append((o, got))
        elif n:
            if host is None:
                host = np.zeros(total, np.uint8)
            host[o:o + n] = np.frombuffer(got, np.uint8)
    if host is not None:
        raw[:total].copy_(torch.from_numpy(host))
    for o, t in tensors:
        raw[o:o + int(t.numel())].copy_(t)
    return raw, parts


def _order(starts: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """The rows [starts[j], starts[j] + counts[j]) for j in order, as indices."""
    total = int(counts.sum())
    first = np.cumsum(counts) - counts
    return np.repeat(starts - first, counts) + np.arange(total, dtype=np.int64)


class _Rows:
    """Rows of a level that arrive group by group -- a group's blobs are a
    subset of the frontier in the order of the pack reads -- and are put back
    into the frontier's order: blob j's rows are [at[j], at[j] + n[j]) of the
    parts' concatenation."""

    def __init__(self, k: int, dev, width: int):
        self.at, self.n = np.zeros(k, np.int64), np.zeros(k, np.int64)
        self.parts, self.base, self.dev, self.width = [], 0, dev, width

    def add(self, js, starts, counts, rows) -> None:
        self.at[js] = self.base + np.asarray(starts, np.int64)
        self.n[js] = counts
        self.parts.append(rows)
        self.base += int(rows.shape[0])

    def add_host(self, j: int, data: bytes) -> None:
        """``data`` (host bytes) as the rows of blob j."""
        import torch
        rows = np.frombuffer(data, np.uint8).reshape((-1, self.width) if self.width else (-1,))
        self.add([j], [0], [len(rows)], torch.from_numpy(rows.copy()).to(self.dev))

    def order(self) -> np.ndarray:
        return _order(self.at, self.n)

    def gather(self):
        import torch
        shape = (0, self.width) if self.width else (0,)
        allrows = torch.cat(self.parts) if self.parts \
            else torch.empty(shape, dtype=torch.uint8, device=self.dev)
        idx = self.order()
        if not len(idx):
            return allrows[:0]
        if len(idx) == int(allrows.shape[0]) and np.array_equal(idx, np.arange(len(idx))):
            return allrows
        return allrows[torch.from_numpy(idx).to(self.dev)]


def _level_groups(key, index, frontier, read_partial, device: int, budget: int):
    """What a level of ``find_used_blobs`` and of ``check.check_trees`` share:
    one lookup of the frontier ((k, 32) device tensor; an id the index lacks
    raises before anything is read), the coalesced pack reads in groups of at
    most ``budget`` decoded bytes and one ``read.read_blobs`` per group.
    Yields (js, plain) per group: the frontier positions of its blobs and
    their decoded texts in HBM."""
    from .dindex import TREE
    from .index import IndexBlob
    from .read import read_blobs
    from .restore import _groups
    hits = index.lookup(TREE, frontier).cpu().numpy().view(np.uint32)
    reads = _level_reads(index, frontier.cpu().numpy(), hits)
    for group in _groups(reads, int(budget)):
        raw, parts = _load_group(group, read_partial, frontier.device)
        owners = sorted((dests[0], o + bl.offset - r.offset, bl)
                        for r, o in parts for bl, dests in r.blobs)
        entries = [IndexBlob(b"", TREE, at, bl.length, bl.uncompressed_length or None)
                   for _, at, bl in owners]
        yield np.array([j for j, _, _ in owners], np.int64), read_blobs(key, raw, entries, device)


def _blob_text(plain, i: int) -> bytes:
    """Blob i of a ``read_blobs`` result on the host."""
    o, ln = int(plain.offsets[i]), int(plain.lengths[i])
    return plain.data[o:o + ln].cpu().numpy().tobytes()


def _device_level(key, index, frontier, read_partial, device: int, budget: int):
    """One level on the device: (data ids, tree ids, is_dir) of the trees in
    ``frontier`` ((k, 32) device tensor), in the order blob, node, array."""
    dev = frontier.device
    k = int(frontier.shape[0])
    data, tree, flags = _Rows(k, dev, 32), _Rows(k, dev, 32), _Rows(k, dev, 0)
    for js, plain in _level_groups(key, index, frontier, read_partial, device, budget):
        res = parse_trees(plain.data, plain.offsets, plain.lengths, device)
        data.add(js, res.blobs["data_start"], res.blobs["data_ids"], res.data_ids)
        tree.add(js, res.blobs["tree_start"], res.blobs["tree_ids"], res.tree_ids)
        flags.add(js, res.blobs["tree_start"], res.blobs["tree_ids"], res.tree_is_dir)
        # the host rule for the blobs the device left: their ids join the level's arrays
        for i in np.nonzero(res.blobs["status"] != OK)[0]:
            _, d, t = parse_tree_host(_blob_text(plain, i))
            j = int(js[i])
            data.add_host(j, b"".join(d))
            tree.add_host(j, b"".join(i for i, _ in t))
            flags.add_host(j, bytes(int(f) for _, f in t))
    return data.gather(), tree.gather(), flags.gather()


def _host_blob(key, index, tree_id: bytes, read_partial, decode, device) -> bytes:
    """Tree::from_backend's read for one id on the host."""
    from .dindex import TREE, DeviceIndex
    e = index.get_id(TREE, tree_id) if isinstance(index, DeviceIndex) else index.get(tree_id)
    if e is None:
        raise _not_found(tree_id)
    pack_id, b = e
    sealed = read_partial(pack_id, int(b.offset), int(b.length))
    if hasattr(sealed, "cpu"):
        sealed = sealed.cpu().numpy().tobytes()
    plain = key.decrypt_data(bytes(sealed))
    ulen = int(getattr(b, "uncompressed_length", None) or 0)
    if not ulen:
        return plain
    out = _decode(plain, device, decode)
    if len(out) != ulen:  # decrypt.rs:86-93
        raise RusticError(ErrorKind.Internal,
                          f"Length of uncompressed data `{len(out)}` does not match the given "
                          f"length `{ulen}`.")
    return out


def _find_used_host(key, index, roots, read_partial, decode) -> np.ndarray:
    used, used_set = list(roots), set(roots)
    visited = set(roots)
    frontier = list(roots)
    while frontier:
        data, tree = [], []
        for tid in frontier:
            _, d, t = parse_tree_host(_host_blob(key, index, tid, read_partial, decode, None))
            data += d
            tree += t
        for i in data + [i for i, is_dir in tree if is_dir]:
            if i not in used_set:
                used_set.add(i)
                used.append(i)
        frontier = []
        for i, _ in tree:
            if i not in visited:
                visited.add(i)
                frontier.append(i)
    return np.frombuffer(b"".join(used), np.uint8).reshape(len(used), 32).copy()


def find_used_blobs(key, index, snap_trees: Sequence[bytes], read_partial: Callable,
                    device: Optional[int] = 0, budget: int = DEFAULT_BUDGET,
                    decode: Optional[Callable] = None):
    """find_used_blobs (commands/prune.rs:1582-1632): the distinct ids of
    every blob the snapshots with the trees ``snap_trees`` use, as one
    (m, 32) uint8 device tensor -- ``PrunePlan.from_entries``'s ``used_ids``.

    Order: the snapshot trees first, then level by level (a level is the
    trees first reached from the level before, the first being the snapshot
    trees), in order of first appearance: per level the content ids of file
    nodes in the order blob, node, array, then the subtrees of dir nodes in
    the order blob, node.

    Per level: ``index.lookup(TREE, frontier)`` (``index``: a
    ``dindex.DeviceIndex``; an id it lacks raises ErrorKind.Internal "Tree ID
    `...` not found in index", as Tree::from_backend does); the pack reads
    coalesced and taken in groups of at most ``budget`` decoded bytes, as
    ``restore.restore_contents`` takes its reads (``read_partial(pack_id,
    offset, length)`` returns bytes or a uint8 device tensor);
    ``read.read_blobs``; ``parse_trees``; ``parse_tree_host`` for the blobs
    the device's grammar leaves out, whose ids take the blob's place in the
    level's arrays.  Two id-only device sets then decide: every subtree id
    new to ``visited`` is in the next level, and the content ids and dir
    subtrees new to ``used`` are appended to the result.  The grouping does
    not change the result.

    ``device=None`` is the same rule in plain Python over ``parse_tree_host``
    and returns a numpy array: ``index`` may then also be
    ``restore.index_lookup``'s dict, ``key`` needs ``decrypt_data`` only, and
    ``decode`` (frame -> bytes) decodes compressed blobs (None:
    ``compress.decode_all``, which runs on device 0)."""
    roots = _distinct(snap_trees)
    if device is None:
        return _find_used_host(key, index, roots, read_partial, decode)
    import torch
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        if not roots:
            return torch.empty((0, 32), dtype=torch.uint8, device=dev)
        frontier = torch.from_numpy(np.frombuffer(b"".join(roots), np.uint8)
                                    .reshape(-1, 32).copy()).to(dev)
        visited, used = _IdSet(int(device)), _IdSet(int(device))
        try:
            visited.take(frontier)
            out = [used.take(frontier)]
            while int(frontier.shape[0]):
                data, tree, is_dir = _device_level(key, index, frontier, read_partial,
                                                   int(device), budget)
                out.append(used.take(data))
                out.append(used.take(tree, is_dir))
                frontier = visited.take(tree)
            return torch.cat(out)
        finally:
            visited.close()
            used.close()
