"""The ``repair snapshots`` command: which trees change is judged in HBM
(rcdc_repair_trees_level, rcdc_repair_spread in include/rcdc.h), the changed
trees and snapshots are rewritten on the host (``tree_write``), and the new
blobs go through the device's compress, seal, pack and indexer.

Reference: ``commands/repair/snapshots.rs`` (``RepairState``, the visitor)
over ``blob/tree/modify.rs`` (``TreeModifier::modify_tree``, ``save_tree``).

The rule, per tree id (a tree is processed once; its outcome depends on its
id, the index and the options only):
- a ``file`` node keeps the content ids ``index.get_data`` has; if one was
  dropped its name gets the suffix and the tree is changed; its size becomes
  the sum of ``data_length()`` of the kept ids, which alone changes nothing;
- a ``dir`` node's subtree is visited and replaced where it changed; a ``dir``
  without a subtree gets the empty tree, which is saved;
- every other type is kept as it is, its subtree is not visited;
- a tree that cannot be loaded (not in the index, a read, MAC, zstd or length
  failure, a text ``Node``'s deserialiser refuses) is changed and processed as
  the empty tree;
- a changed tree is serialised; if its new id is its old id it is unchanged
  after all;
- a ``file`` node without ``content`` makes the reference panic: here it
  raises ErrorKind.Internal with the node's path, on every route, before
  anything is written.

``device=None`` is this rule in plain Python over host parses.  With a device
the walk of ``check.check_trees`` runs with the node records in HBM; only the
texts of the trees the spread marks cross to the host, where the same rule
runs over them alone.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import ErrorKind, RusticError, status_error
from .tree_write import (FullNode, parse_snapshot, parse_tree_full, serialize_snapshot,
                         serialize_tree)

DATA, TREE = 0, 1
DEFAULT_BUDGET = 1 << 30
NO_EDGE = 0xFFFFFFFF  # RCDC_REPAIR_NO_EDGE
NO_NODE = 0xFFFFFFFFFFFFFFFF  # RCDC_REPAIR_NO_NODE
REPAIR_EDGE = np.dtype([("parent", "<u4"), ("child", "<u4")])  # rcdc_repair_edge
APPEND_ONLY_MESSAGE = ("Removing snapshots is not allowed in append-only repositories. Please "
                       "disable append-only mode first, if you know what you are doing. Aborting.")


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


class RepairSnapshotsOptions(NamedTuple):
    """RepairSnapshotsOptions and its defaults (snapshots.rs:27-59)."""
    delete: bool = True
    suffix: str = ".repaired"
    tags: Tuple[str, ...] = ("repaired",)


class SnapshotOutcome(NamedTuple):
    """``id``: the snapshot's id; ``tree``: its tree as it was; ``new_tree``
    None where the snapshot is unchanged, else its new tree with ``text``, the
    new snapshot file's JSON."""
    id: bytes
    tree: bytes
    new_tree: Optional[bytes] = None
    text: Optional[bytes] = None


class RepairPlan:
    """What ``repair snapshots`` would do.  ``changed`` {old tree id: new id},
    ``unchanged`` (a set of tree ids), ``new_trees`` [(id, text)] in the order
    the reference saves them, each id once, without those the index has,
    ``snapshots`` [SnapshotOutcome], ``delete`` [snapshot id] and ``stats``
    (``text_bytes_to_host``, ``host_parsed_blobs``, ``spread_rounds``)."""

    def __init__(self, changed, unchanged, new_trees, snapshots, delete, stats):
        self.changed, self.unchanged, self.new_trees = changed, unchanged, new_trees
        self.snapshots, self.delete, self.stats = snapshots, delete, stats

    def fields(self):
        """Everything but ``stats``, which says how the plan was reached."""
        return self.changed, self.unchanged, self.new_trees, self.snapshots, self.delete


def check_append_only(config, opts: RepairSnapshotsOptions) -> None:
    """snapshots.rs:169-174."""
    if opts.delete and getattr(config, "append_only", None) is True:
        raise RusticError(ErrorKind.AppendOnly, APPEND_ONLY_MESSAGE)


def data_length(blob) -> int:
    """IndexEntry::data_length (blob.rs:146-151)."""
    return int(blob.uncompressed_length) if blob.uncompressed_length else int(blob.length) - 32


class _HostLookups:
    """``get_id`` of a ``check.HostIndex``, a ``dindex.DeviceIndex`` or a dict
    {id: (pack id, IndexBlob)}."""

    def __init__(self, index):
        self.index = index

    def get_id(self, tpe: int, id_: bytes):
        if hasattr(self.index, "get_id"):
            return self.index.get_id(tpe, bytes(id_))
        e = self.index.get(bytes(id_))
        return e if e is not None and int(e[1].type) == tpe else None

    def get(self, id_: bytes):  # tree._host_blob asks a plain index
        return self.get_id(TREE, id_)


def _no_content(where: str) -> RusticError:
    return RusticError(ErrorKind.Internal,
                       f"file `{where}` has no content: the reference's repair panics on such a "
                       "node, so there is no result to follow")


class _Modifier:
    """TreeModifier::modify_tree with RepairState as its visitor.  ``load``
    (tree id -> [FullNode], None where the tree cannot be loaded);
    ``length_of`` (content id -> data_length, None where the index lacks it).
    ``saved``: every tree ``save_tree`` was called with, in order."""

    def __init__(self, opts: RepairSnapshotsOptions, load: Callable, length_of: Callable,
                 unchanged_unless: Optional[set] = None):
        self.opts, self.load, self.length_of = opts, load, length_of
        self.only = unchanged_unless  # the device's verdict: every other tree is unchanged
        self.changed: Dict[bytes, bytes] = {}
        self.unchanged: set = set()
        self.saved: Dict[bytes, bytes] = {}

    def save(self, nodes) -> bytes:
        text, new_id = serialize_tree(nodes)
        self.saved.setdefault(new_id, text)
        return new_id

    def modify(self, tid: bytes, path: str) -> Optional[bytes]:
        """The new id of tree ``tid``, None where it is unchanged."""
        from .check import _join
        if tid in self.changed:
            return self.changed[tid]
        if tid in self.unchanged or (self.only is not None and tid not in self.only):
            return None
        nodes = self.load(tid)
        changed = nodes is None
        new: List[FullNode] = []
        for node in nodes or []:
            where = _join(path, node.name)
            if node.type == "file":
                if node.content is None:
                    raise _no_content(where)
                kept, size = [], 0
                for i in node.content:
                    n = self.length_of(i)
                    if n is not None:
                        kept.append(i)
                        size += n
                dropped = len(kept) != len(node.content)
                if int(node.size) != size or dropped:
                    node = dataclasses.replace(
                        node, content=kept, size=size,
                        name=node.name + self.opts.suffix if dropped else node.name)
                changed |= dropped
            elif node.type == "dir":
                if node.subtree is None:
                    node = dataclasses.replace(node, subtree=self.save([]))
                    changed = True
                else:
                    below = self.modify(node.subtree, where)
                    if below is not None:
                        node = dataclasses.replace(node, subtree=below)
                        changed = True
            new.append(node)
        new_id = None
        if changed:
            got = self.save(new)
            new_id = got if got != tid else None
        if new_id is None:
            self.unchanged.add(tid)
        else:
            self.changed[tid] = new_id
        return new_id


def _snapshot_tags(tags: Sequence[str]) -> List[str]:
    return sorted({t for s in tags for t in str(s).split(",")})  # StringList::from_str, add_all


def _open_snapshots(key, snapshots, device, decode):
    from .check import _decrypt_file
    out = []
    for sid, sealed in snapshots:
        o = parse_snapshot(_decrypt_file(key, bytes(sealed), device, decode))
        out.append((bytes(sid), o, bytes.fromhex(o["tree"])))
    return out


def _finish(mod: _Modifier, opened, opts, has_tree: Callable, stats) -> RepairPlan:
    """The plan from a modifier that has seen every snapshot's tree."""
    outcomes, delete = [], []
    for sid, o, tree in opened:
        new = mod.changed.get(tree)
        if new is None:
            outcomes.append(SnapshotOutcome(sid, tree))
            continue
        o = dict(o)
        if o.get("original") is None:
            o["original"] = sid.hex()
        o["tags"] = _snapshot_tags(opts.tags)
        o["tree"] = new.hex()
        outcomes.append(SnapshotOutcome(sid, tree, new, serialize_snapshot(o, sid)))
        delete.append(sid)
    ids = list(mod.saved)
    held = has_tree(ids)
    new_trees = [(i, mod.saved[i]) for i, h in zip(ids, held) if not h]
    return RepairPlan(dict(mod.changed), set(mod.unchanged), new_trees, outcomes,
                      delete if opts.delete else [], stats)


def _plan_host(key, index, opened, read_partial, opts, decode, device, stats) -> RepairPlan:
    from .tree import _host_blob
    look = _HostLookups(index)
    lengths: Dict[bytes, Optional[int]] = {}

    def load(tid):
        try:
            text = _host_blob(key, look, tid, read_partial, decode, device)
            stats["host_parsed_blobs"] += 1
            return parse_tree_full(text)
        except Exception:  # whatever the backend, the key or the parser raises
            return None

    def length_of(i):
        if i not in lengths:
            e = look.get_id(DATA, i)
            lengths[i] = None if e is None else data_length(e[1])
        return lengths[i]
    mod = _Modifier(opts, load, length_of)
    for _, _, tree in opened:
        mod.modify(tree, "")
    return _finish(mod, opened, opts, lambda ids: [look.get_id(TREE, i) is not None for i in ids],
                   stats)


def plan_repair(key, index, snapshots, read_partial: Callable,
                opts: RepairSnapshotsOptions = RepairSnapshotsOptions(),
                device: Optional[int] = 0, budget: int = DEFAULT_BUDGET,
                decode: Optional[Callable] = None, config=None) -> RepairPlan:
    """What ``repair snapshots`` does to ``snapshots`` ([(id, sealed file)]),
    computed and not written.  ``index``: a ``dindex.DeviceIndex``; with
    ``device=None`` a ``check.HostIndex`` or a dict {id: (pack id,
    IndexBlob)}, ``key`` then needs ``decrypt_data`` only and ``decode``
    (frame -> bytes) decodes compressed blobs.  ``config`` (optional) is
    checked for append-only.

    With a device, per level of the walk: one lookup of the frontier (an id
    the tree index lacks is damaged and left out of the reads), the coalesced
    pack reads and ``read.read_blobs`` of ``tree._level_groups``,
    ``tree.parse_tree_nodes``, the content ids looked up as they are, the
    subtrees of dir nodes put into the id-only set whose entry numbers are
    the slots, rcdc_repair_trees_level.  A blob outside the device's grammar
    goes through the host rule and contributes its damage flag and edges.
    Then rcdc_repair_spread; the texts of the changed trees alone are read
    again and cross; one ``DeviceIndex.lookup`` answers every content id of
    theirs; the rule runs over them bottom-up, ids by ``hashlib``."""
    if config is not None:
        check_append_only(config, opts)
    stats = {"text_bytes_to_host": 0, "host_parsed_blobs": 0, "spread_rounds": 0}
    opened = _open_snapshots(key, snapshots, device, decode)
    if device is None:
        return _plan_host(key, index, opened, read_partial, opts, decode, None, stats)
    return _plan_device(key, index, opened, read_partial, opts, int(device), int(budget), decode,
                        stats)


# ---- the device route -------------------------------------------------------------------

def run_repair_level(res, data_hits, tree_hits, blob_slot, damaged, device: int = 0,
                     guard: int = 0):
    """rcdc_repair_trees_level over the outputs of one ``tree.parse_tree_nodes``
    (``res``; anything with ``node_records`` and ``tree_is_dir`` does), the
    (n, 6) int32 hit records of the content ids in the data index and of the
    subtree ids in the walk's id set, ``blob_slot`` (int32 device tensor, a
    slot per blob) and ``damaged`` (uint8 device tensor, a byte per slot,
    written in place).  Returns (edges, result): a (subtrees, 2) int32 device
    tensor and the _lib.RepairLevelResult.  ``guard``: that many bytes of 0xA5
    kept behind the edges (the flat tensor is then returned), for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    nodes = res.node_records
    if nodes.numel() and nodes.data_ptr() % 16:
        nodes = nodes.clone()
    n_tree = int(tree_hits.shape[0])
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    result = _lib.RepairLevelResult()
    with torch.cuda.device(dev):
        flat = torch.full((n_tree * 8 + guard,), 0xA5, dtype=torch.uint8, device=dev)
        _check(_lib.lib().rcdc_repair_trees_level(
            _ctx(int(device)).handle, ptr(nodes), int(nodes.shape[0]), ptr(data_hits),
            int(data_hits.shape[0]), ptr(res.tree_is_dir), ptr(tree_hits), n_tree, ptr(blob_slot),
            int(blob_slot.shape[0]), ptr(damaged), int(damaged.numel()), ptr(flat) if n_tree else None,
            ctypes.byref(result), int(torch.cuda.current_stream(dev).cuda_stream)))
    if guard:
        return flat, result
    return flat.view(torch.int32).view(n_tree, 2), result


def run_repair_spread(edges, damaged, device: int = 0, guard: int = 0):
    """rcdc_repair_spread: ``edges`` (n, 2) int32 device tensor of (parent,
    child) slots, ``damaged`` uint8 device tensor.  Returns (changed, rounds);
    ``guard``: bytes of 0xA5 kept behind ``changed``, for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    n, k = int(edges.shape[0]), int(damaged.numel())
    edges = edges.contiguous()
    if n and edges.data_ptr() % 8:
        edges = edges.clone()
    rounds = ctypes.c_uint64(0)
    with torch.cuda.device(dev):
        flat = torch.full((k + guard,), 0xA5, dtype=torch.uint8, device=dev)
        _check(_lib.lib().rcdc_repair_spread(
            _ctx(int(device)).handle, edges.data_ptr() if n else None, n,
            damaged.data_ptr() if k else None, flat.data_ptr() if k else None, k,
            ctypes.byref(rounds), int(torch.cuda.current_stream(dev).cuda_stream)))
    return (flat if guard else flat[:k]), int(rounds.value)


def spread_rounds_per_launch() -> int:
    """RCDC_REPAIR_SPREAD_ROUNDS."""
    return int(_lib.lib().rcdc_repair_spread_rounds_per_launch())


class _Slots:
    """The walk's id-only set: a tree id's slot is its entry number."""

    def __init__(self, device: int):
        from .tree import _IdSet
        import torch
        self.set = _IdSet(device)
        self.torch, self.dev = torch, torch.device("cuda", device)

    def close(self):
        self.set.close()

    def size(self) -> int:
        return int(_lib.lib().rcdc_dindex_size(self.set._h))

    def take(self, ids, select=None):
        return self.set.take(ids, select)

    def hits(self, ids):
        """(n, 6) int32 hit records of ``ids`` in the set."""
        torch = self.torch
        n = int(ids.shape[0])
        hits = torch.empty((n, 6), dtype=torch.int32, device=self.dev)
        if n:
            ids = ids.contiguous()
            if ids.data_ptr() % 16:
                ids = ids.clone()
            with torch.cuda.device(self.dev):
                _check(_lib.lib().rcdc_dindex_lookup(
                    self.set._h, ids.data_ptr(), n, hits.data_ptr(),
                    int(torch.cuda.current_stream(self.dev).cuda_stream)))
        return hits


def _read_level(key, index, ids, read_partial, device: int, budget: int, lost: list):
    """The tree blobs ``ids`` ((k, 32) uint8 device tensor) read as
    ``tree._level_groups`` reads a level, with two differences: a row whose id
    the tree index lacks goes to ``lost`` and is left out of the reads, and a
    group whose read, open or decode fails is taken again blob by blob, the
    failing rows going to ``lost``.  Yields (js, plain) per batch."""
    from .dindex import COL_ENTRY, COL_PACK, MISS, NO_PACK
    from .index import IndexBlob
    from .read import read_blobs
    from .restore import _groups
    from .tree import _level_reads, _load_group
    hits = index.lookup(TREE, ids).cpu().numpy().view(np.uint32)
    missing = (hits[:, COL_ENTRY] == MISS) | (hits[:, COL_PACK] == NO_PACK)
    lost += [int(j) for j in np.nonzero(missing)[0]]
    present = np.nonzero(~missing)[0]
    if not len(present):
        return
    reads = _level_reads(index, ids.cpu().numpy()[present], hits[present])
    for group in _groups(reads, int(budget)):
        try:
            raw, parts = _load_group(group, read_partial, ids.device)
        except Exception:  # the backend's error: every blob of the group is lost
            lost += [int(present[d]) for r in group for _, dests in r.blobs for d in dests]
            continue
        owners = sorted((dests[0], o + bl.offset - r.offset, bl)
                        for r, o in parts for bl, dests in r.blobs)
        entry = lambda at, bl: IndexBlob(b"", TREE, at, bl.length, bl.uncompressed_length or None)
        try:
            plain = read_blobs(key, raw, [entry(at, bl) for _, at, bl in owners], device)
            yield present[[j for j, _, _ in owners]], plain
        except RusticError:
            for j, at, bl in owners:
                try:
                    yield present[[j]], read_blobs(key, raw, [entry(at, bl)], device)
                except RusticError:
                    lost.append(int(present[j]))


def _plan_device(key, index, opened, read_partial, opts, device: int, budget: int, decode,
                 stats) -> RepairPlan:
    import torch
    from .dindex import COL_COUNT, COL_ENTRY, COL_LENGTH, COL_PACK, COL_ULEN, NO_PACK
    from .tree import OK, _blob_text, _distinct, parse_tree_nodes
    dev = torch.device("cuda", device)
    roots = _distinct([t for _, _, t in opened])
    as_rows = lambda ids: torch.from_numpy(
        np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32).copy()).to(dev)
    no_content = False
    with torch.cuda.device(dev):
        empty_hits = torch.empty((0, 6), dtype=torch.int32, device=dev)
        lookup = lambda t, ids: index.lookup(t, ids) if int(ids.shape[0]) else empty_hits
        slots = _Slots(device)
        try:
            damaged = torch.zeros(max(64, 2 * len(roots)), dtype=torch.uint8, device=dev)
            edges, host_edges = [], []
            level_ids, level_slots = [], []
            frontier = slots.take(as_rows(roots)) if roots else torch.empty((0, 32), dtype=torch.uint8,
                                                                           device=dev)
            while int(frontier.shape[0]):
                f_slots = slots.hits(frontier)[:, COL_ENTRY].contiguous()
                level_ids.append(frontier)
                level_slots.append(f_slots)
                nxt, lost = [], []

                def room():
                    nonlocal damaged
                    if slots.size() > int(damaged.numel()):
                        more = torch.zeros(2 * slots.size(), dtype=torch.uint8, device=dev)
                        more[:int(damaged.numel())] = damaged
                        damaged = more
                for js, plain in _read_level(key, index, frontier, read_partial, device, budget, lost):
                    res = parse_tree_nodes(plain.data, plain.offsets, plain.lengths, device)
                    nxt.append(slots.take(res.tree_ids, res.tree_is_dir))
                    room()
                    blob_slot = f_slots[torch.from_numpy(np.asarray(js, np.int64)).to(dev)].contiguous()
                    e, r = run_repair_level(res, lookup(DATA, res.data_ids), slots.hits(res.tree_ids),
                                            blob_slot, damaged, device)
                    edges.append(e)
                    no_content |= int(r.files_without_content) != 0
                    # a blob outside the device's grammar: the host rule, at its slot
                    for i in np.nonzero(res.blobs["status"] != OK)[0]:
                        text = _blob_text(plain, int(i))
                        stats["text_bytes_to_host"] += len(text)
                        stats["host_parsed_blobs"] += 1
                        slot = int(blob_slot[int(i)].item())
                        try:
                            nodes = parse_tree_full(text)
                        except RusticError:
                            damaged[slot] = 1
                            continue
                        no_content |= any(n.type == "file" and n.content is None for n in nodes)
                        cids = [c for n in nodes if n.type == "file" for c in n.content or []]
                        h = lookup(DATA, as_rows(cids)).cpu().numpy().view(np.uint32) if cids \
                            else np.zeros((0, 6), np.uint32)
                        if ((h[:, COL_COUNT] == 0) | (h[:, COL_PACK] == NO_PACK)).any() or \
                                any(n.type == "dir" and n.subtree is None for n in nodes):
                            damaged[slot] = 1
                        subs = [n.subtree for n in nodes if n.type == "dir" and n.subtree is not None]
                        if subs:
                            rows = as_rows(subs)
                            nxt.append(slots.take(rows))
                            room()
                            child = slots.hits(rows)[:, COL_ENTRY].cpu().numpy()
                            host_edges += [(slot, int(c)) for c in child]
                if lost:
                    damaged[f_slots[torch.tensor(lost, dtype=torch.int64, device=dev)].long()] = 1
                frontier = torch.cat(nxt) if nxt else frontier[:0]
            n_slots = slots.size()
        finally:
            slots.close()
        if no_content:
            # the path of the first such node in the rule's own order: the host rule raises it
            return _plan_host(key, index, opened, read_partial, opts, decode, device, stats)
        if host_edges:
            edges.append(torch.tensor(host_edges, dtype=torch.int64, device=dev).to(torch.int32)
                         .reshape(-1, 2))
        all_edges = torch.cat(edges) if edges else torch.empty((0, 2), dtype=torch.int32, device=dev)
        changed, rounds = run_repair_spread(all_edges, damaged[:n_slots], device)
        stats["spread_rounds"] = rounds
        # every tree id of the walk by slot, and the marked ones
        ids_all = torch.cat(level_ids) if level_ids else torch.empty((0, 32), dtype=torch.uint8,
                                                                      device=dev)
        slot_all = torch.cat(level_slots).long() if level_slots else torch.empty(0, dtype=torch.int64,
                                                                               device=dev)
        marked = changed[slot_all] != 0
        walked = [r.tobytes() for r in ids_all.cpu().numpy()]
        cand_rows = ids_all[marked].contiguous()
        cand = [r.tobytes() for r in cand_rows.cpu().numpy()]
        # the marked trees' texts cross, the others never do
        texts: Dict[bytes, Optional[List[FullNode]]] = {i: None for i in cand}
        if cand:
            lost = []
            for js, plain in _read_level(key, index, cand_rows, read_partial, device, budget, lost):
                host = plain.data.cpu().numpy()
                for j, o, n in zip(js, plain.offsets, plain.lengths):
                    text = host[int(o):int(o) + int(n)].tobytes()
                    stats["text_bytes_to_host"] += len(text)
                    stats["host_parsed_blobs"] += 1
                    try:
                        texts[cand[int(j)]] = parse_tree_full(text)
                    except RusticError:
                        pass
        # every content id of their file nodes in one lookup
        cids = list(dict.fromkeys(c for nodes in texts.values() for n in nodes or []
                                  if n.type == "file" for c in n.content or []))
        lengths: Dict[bytes, Optional[int]] = {}
        if cids:
            h = index.lookup(DATA, as_rows(cids)).cpu().numpy().view(np.uint32)
            for c, r in zip(cids, h):
                if int(r[COL_COUNT]) == 0 or int(r[COL_PACK]) == NO_PACK:
                    lengths[c] = None
                else:
                    lengths[c] = int(r[COL_ULEN]) or int(r[COL_LENGTH]) - 32
        mod = _Modifier(opts, texts.get, lengths.get, unchanged_unless=set(cand))
        for _, _, tree in opened:
            mod.modify(tree, "")
        mod.unchanged |= set(walked) - set(mod.changed)

        def has_tree(ids):
            if not ids:
                return []
            h = index.lookup(TREE, as_rows(ids)).cpu().numpy().view(np.uint32)
            return [int(r[COL_COUNT]) != 0 for r in h]
        return _finish(mod, opened, opts, has_tree, stats)


# ---- the writes -------------------------------------------------------------------------

class RepairResult(NamedTuple):
    """``apply_repair``'s result.  ``tree_ids``: the new trees' ids in save
    order; ``packs``: [repack.NewPack], the tree packs as device tensors;
    ``index_files`` / ``snapshots``: [(id, uint8 device tensor of the sealed
    file)]; ``delete``: the snapshot ids to remove.  Writing to a backend is
    the caller's."""
    tree_ids: List[bytes]
    packs: list
    index_files: list
    snapshots: list
    delete: List[bytes]


def _device_texts(torch, dev, texts: Sequence[bytes]):
    """``texts`` back to back at 16-byte steps in one device tensor:
    (tensor, offsets, lengths)."""
    lens = np.array([len(t) for t in texts], np.int64)
    offs = np.zeros(len(texts), np.int64)
    if len(texts) > 1:
        offs[1:] = np.cumsum((lens + 15) // 16 * 16)[:-1]
    total = int(offs[-1] + lens[-1]) if len(texts) else 0
    host = np.zeros(total + 64, np.uint8)
    for t, o in zip(texts, offs):
        host[int(o):int(o) + len(t)] = np.frombuffer(t, np.uint8)
    return torch.from_numpy(host).to(dev), offs, lens


def apply_repair(plan: RepairPlan, key, config, indexer=None, device: int = 0,
                 dry_run: bool = False, tree_size: int = 0, nonces: Optional[Callable] = None
                 ) -> RepairResult:
    """TreeModifier's packer and ``save_file`` for a plan.  The new tree blobs
    go in one batch through ``compress.process_blobs`` at the repository's
    level into tree packs sized by ``PackSizer.from_config(config, TREE,
    tree_size)`` (``tree_size``: ``index.total_size(TREE)``); the packs go to
    ``indexer`` (any indexer of ``repack.BlobCopier``; None: an
    ``index_write.DeviceIndexer`` of this call, whose files are returned).
    The new snapshot files go through ``save_file``'s steps in one
    ``index_write.save_index_files`` call: ``2 || zstd`` for version 2,
    sealed, the SHA-256 as the id.  ``dry_run``: the ids and nothing else.
    ``nonces`` (n -> (n, 16) uint8): the packer's and the files' nonces, for
    tests."""
    delete = list(plan.delete)
    tree_ids = [i for i, _ in plan.new_trees]
    if dry_run:
        return RepairResult(tree_ids, [], [], [], delete)
    import torch
    from .compress import process_blobs
    from .index_write import DeviceIndexer, WrittenJson, save_index_files
    from .pack import PackSizer
    from .repack import BlobCopier
    dev = torch.device("cuda", int(device))
    level = config.zstd()
    index_files: list = []
    own = indexer is None
    if own:
        def save(ids, sealed, offs, lens):
            index_files.extend((bytes(i), sealed[int(o):int(o) + int(n)])
                               for i, o, n in zip(ids, offs, lens))
        indexer = DeviceIndexer(save, device=int(device), key=key, version=int(config.version),
                                level=level or 0)
    packs: list = []
    with torch.cuda.device(dev):
        if plan.new_trees:
            texts = [t for _, t in plan.new_trees]
            d_in, offs, lens = _device_texts(torch, dev, texts)
            copier = BlobCopier(key, key, TREE, indexer,
                                PackSizer.from_config(config, TREE, int(tree_size)), level,
                                config.extra_verify_(), int(device), nonces=nonces)
            sealed, s_offs, s_lens, _, ulens = process_blobs(
                key, d_in.data_ptr(), offs, lens, level, copier._draw(len(texts)), int(device),
                config.extra_verify_())
            from .repack import _Txn
            t = _Txn(copier)
            s = torch.cuda.current_stream(dev).cuda_stream
            copier._pack(torch, dev, s, t, copier._new_blobs(s_offs, s_lens, tree_ids, ulens),
                         sealed, False)
            packs = copier._commit(torch, dev, t) + copier.finalize()
        if own:
            indexer.finalize()
        snaps = [s for s in plan.snapshots if s.text is not None]
        files: list = []
        if snaps:
            d_in, offs, lens = _device_texts(torch, dev, [s.text for s in snaps])
            written = WrittenJson(d_in, offs, lens, int(d_in.numel()), d_in, int(d_in.numel()))
            n16 = None if nonces is None else list(np.asarray(nonces(len(snaps)), np.uint8)
                                                   .reshape(len(snaps), 16))
            ids, out, f_offs, f_lens = save_index_files(key, written, int(config.version),
                                                        level or 0, n16, int(device))
            files = [(bytes(i), out[int(o):int(o) + int(n)]) for i, o, n in zip(ids, f_offs, f_lens)]
        torch.cuda.synchronize(dev)
    return RepairResult(tree_ids, packs, index_files, files, delete)


def repair_snapshots(key, index, snapshots, read_partial: Callable, config,
                     opts: RepairSnapshotsOptions = RepairSnapshotsOptions(),
                     device: Optional[int] = 0, dry_run: bool = False,
                     budget: int = DEFAULT_BUDGET, decode: Optional[Callable] = None,
                     indexer=None, nonces: Optional[Callable] = None):
    """repair_snapshots (snapshots.rs:160-232): the plan and, unless
    ``dry_run``, its writes.  Returns (plan, RepairResult).  ``device=None``
    plans on the host and can only be a dry run."""
    check_append_only(config, opts)
    plan = plan_repair(key, index, snapshots, read_partial, opts, device, budget, decode)
    if device is None and not dry_run:
        raise RusticError(ErrorKind.InvalidInput, "apply_repair needs a device")
    size = int(index.total_size(TREE)) if hasattr(index, "total_size") else 0
    return plan, apply_repair(plan, key, config, indexer, 0 if device is None else int(device),
                              dry_run, size, nonces)
