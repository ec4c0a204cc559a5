"""Prune's plan: which packs are kept, repacked, marked or deleted, and which
blobs of a repacked pack survive (rcdc_prune in include/rcdc.h).

Reference: ``PrunePlan::from_prune_options`` (commands/prune.rs:598-1160):
``PrunePlan::new`` (:611-661, duplicate packs dropped), ``count_used_blobs`` /
``check`` (:770-804), ``decide_packs`` (:822-970) over ``PackInfo::from_pack``
(:1495-1568), ``decide_repack`` (:985-1052), ``check_existing_packs``
(:1061-1115), ``filter_index_files`` (:1122-1149); the repack's pick of blobs
(:1296-1325) and the sizes after prune (:1373-1382).

The per-blob part -- the count of every used id over all index entries, the
order-dependent marking, the sums per pack and the first-wins pick -- runs on
the device over entry arrays in HBM (``DevicePrune``); ``device=None`` runs
the same rule in plain Python in the reference's sequential shape, which is
what the device is tested against.  The per-pack part (thresholds, the
candidate sort, one running sum) is host work either way.  The used ids come
from ``tree.find_used_blobs`` as a device tensor; deleting packs stays with
the caller; ``index_updates`` is the loop
of ``do_prune`` that rebuilds the index (:1230-1353) as data, and
``write_index`` feeds it to an ``index_write.DeviceIndexer`` over the plan's
own entry arrays, so the new index files are written on the device.
"""
from __future__ import annotations

import ctypes
import datetime
import enum
import functools
import re
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import ErrorKind, RusticError, status_error
from .index import IndexBlob
from .pack import PackSizer
from .repack import CopyPackBlobs, _blob_order, _coalesced

DATA, TREE = 0, 1
MIN_INDEX_LEN = 10_000        # prune.rs:48
ENTRY_LEN_COMPRESSED = 41     # packfile.rs:137
MAX_PACK_ENTRIES = 0xFFFF     # PackInfo's u16 counts
MAX_PACK_SUM = 0xFFFFFFFF     # PackInfo's u32 sizes
NONE = 0xFFFFFFFF             # RCDC_PRUNE_NONE
KIND_NONE, KIND_KEEP, KIND_REPACK = 0, 1, 2

# rcdc_prune_range / rcdc_prune_pack as numpy records
RANGE = np.dtype([("first", "<u8"), ("count", "<u4"), ("pad", "<u4")])
PACK = np.dtype([("used_size", "<u8"), ("unused_size", "<u8"), ("used_blobs", "<u4"),
                 ("unused_blobs", "<u4"), ("compressed", "<u4"), ("pad", "<u4")])


# ---- options -------------------------------------------------------------------
_UNITS = {"": 1, "b": 1, "k": 10**3, "kb": 10**3, "ki": 1 << 10, "kib": 1 << 10,
          "m": 10**6, "mb": 10**6, "mi": 1 << 20, "mib": 1 << 20,
          "g": 10**9, "gb": 10**9, "gi": 1 << 30, "gib": 1 << 30,
          "t": 10**12, "tb": 10**12, "ti": 1 << 40, "tib": 1 << 40,
          "p": 10**15, "pb": 10**15, "pi": 1 << 50, "pib": 1 << 50}


class LimitOption(NamedTuple):
    """prune.rs:184-226: ``kind`` is "size" (bytes), "percent" or "unlimited"."""
    kind: str
    value: int = 0

    @classmethod
    def parse(cls, s) -> "LimitOption":
        if isinstance(s, LimitOption):
            return s
        s = str(s)
        if s.endswith("%"):
            try:
                return cls("percent", int(s[:-1]))
            except ValueError:
                raise RusticError(ErrorKind.InvalidInput,
                                  f"Failed to parse percentage limit `{s}`") from None
        if s == "unlimited":
            return cls("unlimited")
        m = re.fullmatch(r"\s*([0-9]+(?:\.[0-9]+)?)\s*([A-Za-z]*)\s*", s)
        if not m or m.group(2).lower() not in _UNITS:
            raise RusticError(ErrorKind.InvalidInput, f"Failed to parse size limit `{s}`")
        return cls("size", int(float(m.group(1)) * _UNITS[m.group(2).lower()]))


@dataclass
class PruneOptions:
    """prune.rs:51-153 (without early_delete_index and ignore_snaps, which
    belong to steps the caller does)."""
    max_repack: object = "10%"
    max_unused: object = "5%"
    keep_pack: datetime.timedelta = datetime.timedelta(0)
    keep_delete: datetime.timedelta = datetime.timedelta(hours=23)
    instant_delete: bool = False
    fast_repack: bool = False
    repack_uncompressed: bool = False
    repack_all: bool = False
    repack_cacheable_only: Optional[bool] = None
    no_resize: bool = False


class PackToDo(enum.Enum):
    """prune.rs:411-430."""
    Undecided = 0
    Keep = 1
    Repack = 2
    MarkDelete = 3
    KeepMarked = 4
    KeepMarkedAndCorrect = 5
    Recover = 6
    Delete = 7


class PackStatus(enum.Enum):
    """prune.rs:228-239."""
    NotCompressed = 0
    TooYoung = 1
    TimeNotSet = 2
    TooLarge = 3
    TooSmall = 4
    HasUnusedBlobs = 5
    HasUsedBlobs = 6
    Marked = 7


class PackInfo(NamedTuple):
    """prune.rs:1456-1467."""
    blob_type: int
    used_blobs: int
    unused_blobs: int
    used_size: int
    unused_size: int

    def sums(self) -> Tuple[int, int, int, int]:
        return self[1:]


@dataclass
class DeleteStats:
    remove: int = 0
    recover: int = 0
    keep: int = 0

    def total(self) -> int:
        return self.remove + self.recover + self.keep


@dataclass
class PackStats:
    used: int = 0
    partly_used: int = 0
    unused: int = 0
    repack: int = 0
    keep: int = 0


@dataclass
class SizeStats:
    used: int = 0
    unused: int = 0
    remove: int = 0
    repack: int = 0
    repackrm: int = 0

    def total(self) -> int:
        return self.used + self.unused

    def unused_after_prune(self) -> int:
        return self.unused - self.remove - self.repackrm

    def total_after_prune(self) -> int:
        return self.used + self.unused_after_prune()

    def __add__(self, o: "SizeStats") -> "SizeStats":
        return SizeStats(self.used + o.used, self.unused + o.unused, self.remove + o.remove,
                         self.repack + o.repack, self.repackrm + o.repackrm)


@dataclass
class PruneStats:
    """prune.rs:349-390.  ``debug``: (PackToDo, blob type, frozenset of
    PackStatus) -> [packs, unused_blobs, unused_size, used_blobs, used_size]
    (DebugStats, :241-283)."""
    packs_to_delete: DeleteStats = field(default_factory=DeleteStats)
    size_to_delete: DeleteStats = field(default_factory=DeleteStats)
    packs: PackStats = field(default_factory=PackStats)
    blobs: Dict[int, SizeStats] = field(default_factory=lambda: {DATA: SizeStats(), TREE: SizeStats()})
    size: Dict[int, SizeStats] = field(default_factory=lambda: {DATA: SizeStats(), TREE: SizeStats()})
    packs_unref: int = 0
    size_unref: int = 0
    index_files: int = 0
    index_files_rebuild: int = 0
    debug: Dict[tuple, list] = field(default_factory=dict)

    def blobs_sum(self) -> SizeStats:
        return self.blobs[DATA] + self.blobs[TREE]

    def size_sum(self) -> SizeStats:
        return self.size[DATA] + self.size[TREE]


@dataclass
class PrunePack:
    """prune.rs:433-449, with the pack's entries as a range of the plan's
    entry arrays instead of a Vec<IndexBlob>."""
    id: bytes
    blob_type: int
    size: int
    time: Optional[str]
    marked: bool
    file: int      # number of its index file in the list given
    first: int     # its entries are [first, first + count)
    count: int
    to_do: PackToDo = PackToDo.Undecided
    info: Optional[PackInfo] = None
    status: frozenset = frozenset()
    compressed: bool = True


@dataclass
class PruneIndex:
    """prune.rs:394-408."""
    id: bytes
    modified: bool
    packs: List[PrunePack]

    def __len__(self) -> int:
        return sum(p.count for p in self.packs)


@dataclass
class IndexUpdates:
    """What ``PrunePlan.index_updates`` gives."""
    adds: list            # (index_write.PackRecord, delete flag) in add order
    delete_packs: dict    # blob type -> pack ids to remove from the backend
    delete_unindexed: list  # existing_packs removed at once (instant_delete)


def _ns(t) -> Optional[int]:
    """A pack's time (RFC 3339 text, as index.rustic_time writes it), a
    datetime or None as nanoseconds since the epoch."""
    if t is None:
        return None
    if isinstance(t, datetime.datetime):
        if t.tzinfo is None:
            t = t.replace(tzinfo=datetime.timezone.utc)
        whole = t.replace(microsecond=0)
        return int(whole.timestamp()) * 10**9 + t.microsecond * 1000
    m = re.fullmatch(r"(\d{4}-\d\d-\d\d[T ]\d\d:\d\d:\d\d)(?:\.(\d{1,9}))?(Z|[+-]\d\d:?\d\d)", str(t))
    if not m:
        raise RusticError(ErrorKind.InvalidInput, f"pack time `{t}` is not RFC 3339")
    off = m.group(3)
    off = "+00:00" if off == "Z" else (off if ":" in off else off[:3] + ":" + off[3:])
    whole = datetime.datetime.fromisoformat(m.group(1).replace(" ", "T") + off)
    return int(whole.timestamp()) * 10**9 + int((m.group(2) or "0").ljust(9, "0"))


def _span_ns(d) -> int:
    if isinstance(d, datetime.timedelta):
        return (d.days * 86400 + d.seconds) * 10**9 + d.microseconds * 1000
    return int(d) * 10**9


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


# ---- the device half -------------------------------------------------------------
class DevicePrune:
    """One rcdc_prune handle over ``used_ids`` ((m, 32) uint8 device tensor)
    on ``device``.  Calls are queued on the current torch stream."""

    def __init__(self, used_ids, device: int = 0):
        import torch
        from .crypto import _ctx
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)
        if not (hasattr(used_ids, "data_ptr") and used_ids.dtype == torch.uint8
                and used_ids.dim() == 2 and used_ids.shape[1] == 32
                and used_ids.device == self._dev):
            raise RusticError(ErrorKind.InvalidInput,
                              f"used ids must be an (m, 32) uint8 tensor on {self._dev}")
        used_ids = used_ids.contiguous()
        self.m = int(used_ids.shape[0])
        self.n = self.n_packs = 0
        self._keep = None  # the entry arrays the handle reads
        h = ctypes.c_void_p()
        with torch.cuda.device(self._dev):
            _check(_lib.lib().rcdc_prune_create(_ctx(self.device).handle,
                                                used_ids.data_ptr() if self.m else None, self.m,
                                                self._stream(), ctypes.byref(h)))
        self.handle = h

    def _stream(self) -> int:
        import torch
        return int(torch.cuda.current_stream(self._dev).cuda_stream)

    def close(self) -> None:
        if getattr(self, "handle", None) is not None:
            _lib.lib().rcdc_prune_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_entries(self, ids, lens, ulens, ranges) -> None:
        """``ids``: (n, 32) uint8, ``lens`` / ``ulens``: n 4-byte integers;
        device tensors, strided views allowed (a column of a ``d_locs``
        tensor).  ``ranges``: (first, count) per pack in processing order."""
        import torch
        n = int(ids.shape[0])
        for t, what in ((ids, "ids"), (lens, "lens"), (ulens, "ulens")):
            if not hasattr(t, "data_ptr") or t.device != self._dev:
                raise RusticError(ErrorKind.InvalidInput, f"{what} must be a tensor on {self._dev}")
        if ids.dtype != torch.uint8 or ids.dim() != 2 or ids.shape[1] != 32 or \
                (n and ids.stride(1) != 1):
            raise RusticError(ErrorKind.InvalidInput, "ids must be (n, 32) uint8 with dense rows")
        for t in (lens, ulens):
            if t.dim() != 1 or int(t.shape[0]) != n or t.element_size() != 4:
                raise RusticError(ErrorKind.InvalidInput, "one 4-byte length per entry")
        r = np.zeros(len(ranges), RANGE)
        if len(ranges):
            a = np.asarray(ranges, dtype=np.uint64).reshape(len(ranges), 2)
            if (a[:, 1] > 0xFFFFFFFF).any():
                raise RusticError(ErrorKind.InvalidInput, "a pack of 65 536 entries or more")
            r["first"], r["count"] = a[:, 0], a[:, 1]
        # a lone row's stride is whatever the view says: give the element's size
        stride = lambda t, unit: int(t.stride(0)) * unit if n > 1 else unit
        with torch.cuda.device(self._dev):
            _check(_lib.lib().rcdc_prune_set_entries(
                self.handle, ids.data_ptr() if n else None, int(ids.stride(0)) if n > 1 else 32,
                lens.data_ptr() if n else None, stride(lens, 4),
                ulens.data_ptr() if n else None, stride(ulens, 4), n,
                r.ctypes.data if len(r) else None, len(r), self._stream()))
        self._keep = (ids, lens, ulens)
        self.n, self.n_packs = n, len(r)

    def mark(self):
        """(counts (m,) uint8 device, used (n,) uint8 device, PACK records on
        the host, rcdc_prune_result)."""
        import torch
        counts = torch.empty(self.m, dtype=torch.uint8, device=self._dev)
        used = torch.empty(self.n, dtype=torch.uint8, device=self._dev)
        packs = np.zeros(self.n_packs, PACK)
        res = _lib.PruneResult()
        with torch.cuda.device(self._dev):
            _check(_lib.lib().rcdc_prune_mark(
                self.handle, counts.data_ptr() if self.m else None,
                used.data_ptr() if self.n else None,
                packs.ctypes.data if self.n_packs else None, ctypes.byref(res), self._stream()))
        return counts, used, packs, res

    def keep(self, kinds, file_rank):
        """(n,) uint8 device tensor: the blobs the repack keeps."""
        import torch
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        rank = np.ascontiguousarray(file_rank, dtype=np.uint32)
        if len(kinds) != self.n_packs or len(rank) != self.n_packs:
            raise RusticError(ErrorKind.InvalidInput, "one kind and one rank per pack")
        out = torch.empty(self.n, dtype=torch.uint8, device=self._dev)
        with torch.cuda.device(self._dev):
            _check(_lib.lib().rcdc_prune_keep(
                self.handle, kinds.ctypes.data if len(kinds) else None,
                rank.ctypes.data if len(rank) else None, out.data_ptr() if self.n else None,
                self._stream()))
        return out


# ---- the same in plain Python (the yardstick) -------------------------------------
class HostPrune:
    """``DevicePrune``'s calls over numpy arrays, one blob after the other as
    the reference does it."""

    def __init__(self, used_ids: np.ndarray):
        self.used_ids = [r.tobytes() for r in np.asarray(used_ids, np.uint8).reshape(-1, 32)]
        if len(set(self.used_ids)) != len(self.used_ids):
            raise RusticError(ErrorKind.InvalidInput, "the used ids are not distinct")
        self.m = len(self.used_ids)

    def close(self) -> None:
        pass

    def set_entries(self, ids, lens, ulens, ranges) -> None:
        ids = np.asarray(ids, np.uint8).reshape(-1, 32)
        self.ids = [r.tobytes() for r in ids]
        self.lens = [int(x) for x in np.asarray(lens)]
        self.ulens = [int(x) for x in np.asarray(ulens)]
        self.ranges = [(int(f), int(c)) for f, c in ranges]
        self.n, self.n_packs = len(self.ids), len(self.ranges)

    def mark(self):
        # count_used_blobs (prune.rs:770-784)
        counter = {i: 0 for i in self.used_ids}
        for f, c in self.ranges:
            for e in range(f, f + c):
                k = counter.get(self.ids[e])
                if k is not None:
                    counter[self.ids[e]] = min(k + 1, 255)
        counts = np.array([counter[i] for i in self.used_ids], np.uint8).reshape(self.m)
        used = np.zeros(self.n, np.uint8)
        packs = np.zeros(self.n_packs, PACK)
        # PackInfo::from_pack (prune.rs:1495-1568) over the packs in order
        for p, (f, c) in enumerate(self.ranges):
            first_needed = None
            for e in range(f, f + c):
                k = counter.get(self.ids[e])
                if k:
                    counter[self.ids[e]] = k - 1
                    if k == 1:
                        used[e] = 1
                        first_needed = e
                        break
            if first_needed is not None:
                for e in list(range(f, first_needed)) + list(range(first_needed + 1, f + c)):
                    if counter.get(self.ids[e]):
                        used[e] = 1
                        counter[self.ids[e]] = 0
            r = packs[p]
            for e in range(f, f + c):
                if used[e]:
                    r["used_blobs"] += 1
                    r["used_size"] += self.lens[e]
                else:
                    r["unused_blobs"] += 1
                    r["unused_size"] += self.lens[e]
            r["compressed"] = all(self.ulens[e] for e in range(f, f + c))
        res = _lib.PruneResult()
        zero = [j for j in range(self.m) if counts[j] == 0]
        res.missing, res.first_missing = len(zero), zero[0] if zero else NONE
        return counts, used, packs, res

    def keep(self, kinds, file_rank):
        out = np.zeros(self.n, np.uint8)
        order = sorted(range(self.n_packs), key=lambda p: int(file_rank[p]))
        used_ids = set(self.used_ids)
        # check_existing_packs takes the ids of Keep / Recover packs out (prune.rs:1092-1095)
        for p in order:
            if kinds[p] == KIND_KEEP:
                f, c = self.ranges[p]
                for e in range(f, f + c):
                    used_ids.discard(self.ids[e])
        # the repack keeps a blob whose id it can still take out (prune.rs:1320-1321)
        for p in order:
            if kinds[p] == KIND_REPACK:
                f, c = self.ranges[p]
                for e in range(f, f + c):
                    if self.ids[e] in used_ids:
                        used_ids.remove(self.ids[e])
                        out[e] = 1
        return out


# ---- the plan ---------------------------------------------------------------------
def _pack_order(a, b) -> int:
    """PackInfo::cmp (prune.rs:1475-1486) over (PackInfo, .., file, pack):
    tree packs first, then the higher unused / used ratio, in 64 bits.  The
    reference's sort is unstable and leaves equal packs in any order; here
    (file number, pack number) decides."""
    pa, pb = a[0], b[0]
    ta, tb = (0 if pa.blob_type == TREE else 1), (0 if pb.blob_type == TREE else 1)
    if ta != tb:
        return -1 if ta < tb else 1
    x, y = pb.unused_size * pa.used_size, pa.unused_size * pb.used_size
    if x != y:
        return -1 if x < y else 1
    return -1 if a[3:] < b[3:] else (1 if a[3:] > b[3:] else 0)


class PrunePlan:
    """What ``from_prune_options`` decides.  ``packs``: every pack that takes
    part, in file order, with ``to_do``, ``info`` (PackInfo) and ``status``;
    ``stats``; ``index_files``: the index files that have to be rewritten
    (PruneIndex, after ``filter_index_files``); ``counts`` / ``used`` /
    ``keep``: the per-id counts and the per-entry flags as numpy arrays."""

    def __init__(self):
        self.packs: List[PrunePack] = []
        self.stats = PruneStats()
        self.index_files: List[PruneIndex] = []
        self.existing_packs: Dict[bytes, int] = {}
        self.rounds = 0

    # ---- constructors ---------------------------------------------------------
    @classmethod
    def from_index_files(cls, files, used_ids, existing_packs, opts: PruneOptions, config, now,
                         device: Optional[int] = 0) -> "PrunePlan":
        """``files``: (index id, index.IndexFile) pairs; ``used_ids``: (m, 32)
        uint8 device tensor or numpy array; ``existing_packs``: {pack id:
        size}; ``config``: what PackSizer.from_config takes; ``now``: the
        time of the plan (datetime or RFC 3339 text).  ``device=None`` runs
        the per-blob part on the host."""
        ids, lens, ulens, offs, recs, index_ids = [], [], [], [], [], []
        for fno, (iid, f) in enumerate(files):
            index_ids.append(bytes(iid))
            for marked, packs in ((False, f.packs), (True, f.packs_to_delete)):
                for p in packs:
                    tpe = int(p.blobs[0].type) if p.blobs else DATA
                    recs.append(PrunePack(bytes(p.id), tpe, int(p.pack_size()), p.time, marked, fno,
                                          len(lens), len(p.blobs)))
                    for b in p.blobs:
                        if len(bytes(b.id)) != 32:
                            raise RusticError(ErrorKind.InvalidInput, "a blob id has 32 bytes")
                        ids.append(bytes(b.id))
                        lens.append(int(b.length))
                        ulens.append(int(b.uncompressed_length or 0))
                        offs.append(int(b.offset))
        n = len(lens)
        a_ids = np.frombuffer(b"".join(ids), np.uint8).reshape(n, 32)
        return cls.from_entries(a_ids, np.array(lens, np.uint32), np.array(ulens, np.uint32),
                                np.array(offs, np.uint32), recs, index_ids, used_ids,
                                existing_packs, opts, config, now, device)

    @classmethod
    def from_entries(cls, ids, lens, ulens, offsets, packs: Sequence[PrunePack], index_ids,
                     used_ids, existing_packs, opts: PruneOptions, config, now,
                     device: Optional[int] = 0) -> "PrunePlan":
        """The plan over entry arrays -- (n, 32) ids, n lengths, uncompressed
        lengths (0 for none) and offsets; device tensors (strided views
        allowed, so ``dindex.parse_json``'s ``ids`` / ``locs`` columns pass as
        they are) or numpy arrays -- and one PrunePack record per pack: id,
        blob_type, size, time, marked, file (number in ``index_ids``), first,
        count.  Records come file by file, a file's packs before its
        packs_to_delete.  No host object per blob is made."""
        self = cls()
        if config.version < 2 and opts.repack_uncompressed:
            raise RusticError(ErrorKind.Unsupported,
                              "Repacking uncompressed pack is unsupported in Repository version "
                              f"`{config.version}`.")
        self._now = _ns(now)
        self._opts = opts
        self._config = config
        self._offsets = offsets
        self._ids, self._lens, self._ulens = ids, lens, ulens
        # the collector sees every pack of every file (prune.rs:710-717)
        total = {DATA: 0, TREE: 0}
        for p in packs:
            total[p.blob_type] += int(p.size)
        self._filter(packs, [bytes(i) for i in index_ids])
        for p in self.packs:
            if p.count > MAX_PACK_ENTRIES:
                raise RusticError(ErrorKind.InvalidInput,
                                  f"pack `{p.id.hex()}` has {p.count} blobs, more than 65 535")
        # processing order: marked packs, then unmarked ones (prune.rs:835-842)
        self._proc = [i for i, p in enumerate(self.packs) if p.marked] + \
                     [i for i, p in enumerate(self.packs) if not p.marked]
        ranges = [(self.packs[i].first, self.packs[i].count) for i in self._proc]
        self._engine = self._make_engine(used_ids, device)
        try:
            self._engine.set_entries(*self._engine_arrays(), ranges)
            counts, used, sums, res = self._engine.mark()
            self.rounds = int(res.rounds)
            self.counts = self._host(counts)
            if res.missing:
                missing = self._used_id(int(res.first_missing))
                raise RusticError(ErrorKind.Internal,
                                  f"Blob ID `{missing.hex()}` is missing in index files.")
            self.used = self._host(used)
            for k, i in enumerate(self._proc):
                s, p = sums[k], self.packs[i]
                if int(s["used_size"]) > MAX_PACK_SUM or int(s["unused_size"]) > MAX_PACK_SUM:
                    raise RusticError(ErrorKind.InvalidInput,
                                      f"the blobs of pack `{p.id.hex()}` pass 2^32 - 1 bytes")
                p.info = PackInfo(p.blob_type, int(s["used_blobs"]), int(s["unused_blobs"]),
                                  int(s["used_size"]), int(s["unused_size"]))
                p.compressed = bool(s["compressed"])
            sizer = {t: PackSizer.from_config(config, t, total[t]) for t in (DATA, TREE)}
            cacheable_only = opts.repack_cacheable_only
            if cacheable_only is None:
                cacheable_only = getattr(config, "is_hot", None) is True
            self._decide_packs(opts, bool(cacheable_only), sizer)
            self._decide_repack(opts, sizer)
            self._check_existing_packs(dict(existing_packs))
            kinds = np.zeros(len(self.packs), np.uint8)
            rank = np.zeros(len(self.packs), np.uint32)
            for k, i in enumerate(self._proc):
                todo = self.packs[i].to_do
                kinds[k] = KIND_KEEP if todo in (PackToDo.Keep, PackToDo.Recover) else \
                    KIND_REPACK if todo == PackToDo.Repack else KIND_NONE
                rank[k] = i
            self.keep = self._host(self._engine.keep(kinds, rank))
        finally:
            self._engine.close()
        self._filter_index_files(opts.instant_delete)
        return self

    # ---- plumbing -------------------------------------------------------------
    def _make_engine(self, used_ids, device):
        if device is None:
            if hasattr(used_ids, "cpu"):
                used_ids = used_ids.cpu().numpy()
            self._used_ids = np.asarray(used_ids, np.uint8).reshape(-1, 32)
            return HostPrune(self._used_ids)
        import torch
        dev = torch.device("cuda", int(device))
        self._dev = dev
        if isinstance(used_ids, np.ndarray):
            a = np.ascontiguousarray(used_ids, dtype=np.uint8).reshape(-1, 32)
            used_ids = torch.from_numpy(a.copy()).to(dev)
        self._used_ids = used_ids
        return DevicePrune(used_ids, int(device))

    def _engine_arrays(self):
        if isinstance(self._engine, HostPrune):
            return tuple(a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
                         for a in (self._ids, self._lens, self._ulens))
        import torch
        out = []
        for a, dt in ((self._ids, np.uint8), (self._lens, np.uint32), (self._ulens, np.uint32)):
            if isinstance(a, np.ndarray):
                a = np.array(a, dtype=dt)  # a copy torch may take over
                a = torch.from_numpy(a.view(np.int32) if dt == np.uint32 else a).to(self._dev)
            out.append(a)
        return tuple(out)

    @staticmethod
    def _host(a) -> np.ndarray:
        return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)

    def _used_id(self, j: int) -> bytes:
        row = self._used_ids[j]
        return bytes(self._host(row).tobytes())

    # ---- PrunePlan::new (prune.rs:611-661) --------------------------------------
    def _filter(self, packs, index_ids) -> None:
        files = [PruneIndex(i, False, []) for i in index_ids]
        seen, seen_delete = set(), set()
        for p in packs:
            f = files[p.file]
            s = seen_delete if p.marked else seen
            if p.id in s:
                f.modified = True
                continue
            s.add(p.id)
            f.packs.append(p)
        for f in files:
            kept = []
            for p in f.packs:
                if p.marked and p.id in seen:
                    f.modified = True
                else:
                    kept.append(p)
            # a file's packs come before its packs_to_delete
            f.packs = [p for p in kept if not p.marked] + [p for p in kept if p.marked]
        self._files = files
        self.packs = [p for f in files for p in f.packs]
        self._where = {}
        for f in files:
            for k, p in enumerate(f.packs):
                self._where[id(p)] = (p.file, k)

    # ---- set_todo (prune.rs:520-560) --------------------------------------------
    def _set_todo(self, p: PrunePack, todo: PackToDo, status: frozenset) -> None:
        st, pi, t = self.stats, p.info, p.blob_type
        d = st.debug.setdefault((todo, t, status), [0, 0, 0, 0, 0])
        d[0] += 1
        d[1] += pi.unused_blobs
        d[2] += pi.unused_size
        d[3] += pi.used_blobs
        d[4] += pi.used_size
        if todo == PackToDo.Keep:
            st.packs.keep += 1
        elif todo == PackToDo.Repack:
            st.packs.repack += 1
            st.blobs[t].repack += pi.unused_blobs + pi.used_blobs
            st.blobs[t].repackrm += pi.unused_blobs
            st.size[t].repack += pi.unused_size + pi.used_size
            st.size[t].repackrm += pi.unused_size
        elif todo == PackToDo.MarkDelete:
            st.blobs[t].remove += pi.unused_blobs
            st.size[t].remove += pi.unused_size
        elif todo == PackToDo.Recover:
            st.packs_to_delete.recover += 1
            st.size_to_delete.recover += p.size
        elif todo == PackToDo.Delete:
            st.packs_to_delete.remove += 1
            st.size_to_delete.remove += p.size
        elif todo in (PackToDo.KeepMarked, PackToDo.KeepMarkedAndCorrect):
            st.packs_to_delete.keep += 1
            st.size_to_delete.keep += p.size
        p.to_do, p.status = todo, status

    # ---- decide_packs (prune.rs:822-970) ------------------------------------------
    def _decide_packs(self, opts: PruneOptions, cacheable_only: bool, sizer) -> None:
        S = PackStatus
        st = self.stats
        self._candidates = []
        keep_pack, keep_delete = _span_ns(opts.keep_pack), _span_ns(opts.keep_delete)
        for i in self._proc:
            p = self.packs[i]
            pi, t = p.info, p.blob_type
            st.blobs[t].used += pi.used_blobs
            st.blobs[t].unused += pi.unused_blobs
            st.size[t].used += pi.used_size
            st.size[t].unused += pi.unused_size
            status = set()
            time = _ns(p.time)
            too_young = time is not None and time > self._now - keep_pack
            if too_young and not p.marked:
                status.add(S.TooYoung)
            keep_uncacheable = cacheable_only and t != TREE
            to_compress = opts.repack_uncompressed and not p.compressed
            if to_compress:
                status.add(S.NotCompressed)
            size_mismatch = not sizer[t].size_ok(p.size)
            if sizer[t].is_too_small(p.size):
                status.add(S.TooSmall)
            if sizer[t].is_too_large(p.size):
                status.add(S.TooLarge)
            where = self._where[id(p)]
            cand = lambda reason: self._candidates.append(
                (pi, frozenset(status), reason) + where + (p,))
            if not p.marked and pi.used_blobs == 0:
                st.packs.unused += 1
                status.add(S.HasUnusedBlobs)
                self._set_todo(p, PackToDo.Keep if too_young else PackToDo.MarkDelete,
                               frozenset(status))
            elif not p.marked and pi.unused_blobs == 0:
                st.packs.used += 1
                status.add(S.HasUsedBlobs)
                if too_young or keep_uncacheable:
                    self._set_todo(p, PackToDo.Keep, frozenset(status))
                elif to_compress or opts.repack_all:
                    cand("ToCompress")
                elif size_mismatch:
                    cand("SizeMismatch")
                else:
                    self._set_todo(p, PackToDo.Keep, frozenset(status))
            elif not p.marked:
                st.packs.partly_used += 1
                status |= {S.HasUsedBlobs, S.HasUnusedBlobs}
                if too_young or keep_uncacheable:
                    self._set_todo(p, PackToDo.Keep, frozenset(status))
                else:
                    cand("PartlyUsed")
            elif pi.used_blobs == 0:
                status.add(S.Marked)
                if time is None:
                    status.add(S.TimeNotSet)
                    self._set_todo(p, PackToDo.KeepMarkedAndCorrect, frozenset(status))
                elif self._now - keep_delete >= time:
                    status.add(S.TooYoung)
                    self._set_todo(p, PackToDo.Delete, frozenset(status))
                else:
                    self._set_todo(p, PackToDo.KeepMarked, frozenset(status))
            else:
                status |= {S.Marked, S.HasUsedBlobs}
                self._set_todo(p, PackToDo.Recover, frozenset(status))

    # ---- decide_repack (prune.rs:985-1052) ------------------------------------------
    def _decide_repack(self, opts: PruneOptions, sizer) -> None:
        st = self.stats
        mu, mr = LimitOption.parse(opts.max_unused), LimitOption.parse(opts.max_repack)
        U64 = (1 << 64) - 1
        if opts.repack_uncompressed or opts.repack_all:
            max_unused = 0
        elif mu.kind == "unlimited":
            max_unused = U64
        elif mu.kind == "size":
            max_unused = mu.value
        else:
            max_unused = (mu.value * st.size_sum().used) // (100 - mu.value)
        max_repack = U64 if mr.kind == "unlimited" else mr.value if mr.kind == "size" else \
            (mr.value * st.size_sum().total()) // 100
        self._candidates.sort(key=functools.cmp_to_key(_pack_order))
        resize = {DATA: [], TREE: []}
        do_repack = {DATA: False, TREE: False}
        repack_size = {DATA: 0, TREE: 0}
        for pi, status, reason, _f, _k, p in self._candidates:
            t = pi.blob_type
            if (repack_size[DATA] + repack_size[TREE] + pi.used_size >= max_repack
                    or (st.size_sum().unused_after_prune() < max_unused
                        and reason == "PartlyUsed" and t == DATA)
                    or (reason == "SizeMismatch" and opts.no_resize)):
                self._set_todo(p, PackToDo.Keep, status)
            elif reason == "SizeMismatch":
                resize[t].append((p, status))
                repack_size[t] += pi.used_size
            else:
                self._set_todo(p, PackToDo.Repack, status)
                repack_size[t] += pi.used_size
                do_repack[t] = True
        self._candidates = []
        for t in (TREE, DATA):
            todo = PackToDo.Repack if do_repack[t] or repack_size[t] > sizer[t].pack_size() \
                else PackToDo.Keep
            for p, status in resize[t]:
                self._set_todo(p, todo, status)

    # ---- check_existing_packs (prune.rs:1061-1115) -------------------------------------
    def _check_existing_packs(self, existing: dict) -> None:
        existing = {bytes(k): int(v) for k, v in existing.items()}
        for p in self.packs:
            size = existing.pop(p.id, None)
            if p.to_do == PackToDo.Undecided:
                raise RusticError(ErrorKind.Internal,
                                  f"Pack `{p.id.hex()}` got no decision what to do with it!")
            if p.to_do in (PackToDo.Keep, PackToDo.Recover, PackToDo.Repack):
                if size is None:
                    raise RusticError(ErrorKind.Internal, f"Pack `{p.id.hex()}` does not exist.")
                if size != p.size:
                    raise RusticError(ErrorKind.Internal,
                                      f"Pack size `{size}` of id `{p.id.hex()}` does not match the "
                                      f"expected size `{p.size}` in the index file. ")
        self.stats.size_unref = sum(existing.values())
        self.stats.packs_unref = len(existing)
        # what is left are packs no index file knows (a BTreeMap: in id order)
        self.existing_packs = dict(sorted(existing.items()))

    # ---- filter_index_files (prune.rs:1122-1149) -----------------------------------------
    def _filter_index_files(self, instant_delete: bool) -> None:
        any_must = False
        self.stats.index_files = len(self._files)
        kept = []
        for f in self._files:
            must = f.modified or any(
                p.to_do != PackToDo.Keep and (instant_delete or p.to_do != PackToDo.KeepMarked)
                for p in f.packs)
            any_must |= must
            if must or len(f) < MIN_INDEX_LEN:
                kept.append(f)
        if not any_must and len(kept) == 1:
            kept = []
        self.index_files = kept
        self.stats.index_files_rebuild = len(kept)

    # ---- what the caller executes ------------------------------------------------------------
    def repack_packs(self) -> List[bytes]:
        """prune.rs:1153-1160."""
        return [p.id for p in self.packs if p.to_do == PackToDo.Repack]

    def repack_plans(self) -> List[Tuple[PrunePack, List[CopyPackBlobs]]]:
        """Per Repack pack, in file order: what ``repack.plan_repack`` gives
        for it -- the surviving blobs in IndexBlob order, coalesced -- from
        the ``keep`` flags."""
        offs = self._host(self._offsets)
        ids, lens, ulens = (self._host(a) for a in (self._ids, self._lens, self._ulens))
        out = []
        for p in self.packs:
            if p.to_do != PackToDo.Repack:
                continue
            blobs = [IndexBlob(ids[e].tobytes(), p.blob_type, int(offs[e]) & MAX_PACK_SUM,
                               int(lens[e]) & MAX_PACK_SUM,
                               (int(ulens[e]) & MAX_PACK_SUM) or None)
                     for e in range(p.first, p.first + p.count) if self.keep[e]]
            blobs.sort(key=_blob_order)
            out.append((p, _coalesced(CopyPackBlobs.from_index_entry(p.id, b) for b in blobs)))
        return out

    def index_updates(self, prune_time: str, instant_delete: bool = False) -> "IndexUpdates":
        """The index half of ``do_prune`` (prune.rs:1230-1353) as data.
        ``adds``: (PackRecord, delete flag) in the order the reference gives
        packs to its indexer -- first a removal record per pack of
        ``existing_packs`` (``size`` set, no blobs, ``time = prune_time``)
        unless ``instant_delete``, then every pack of ``index_files``
        according to its ``to_do``: ``into_index_pack`` keeps a pack's time
        and sets ``prune_time`` where it has none, ``into_index_pack_with_time``
        sets ``prune_time``; ``size`` is absent.  ``delete_packs``: per blob
        type, the packs to remove from the backend (``Delete`` packs, and
        with ``instant_delete`` every pack that would else be marked);
        ``delete_unindexed``: the ``existing_packs`` that ``instant_delete``
        removes.  Nothing is to do when ``index_files`` is empty (:1260-1263):
        only the removal records are given then."""
        from .index_write import PackRecord
        up = IndexUpdates([], {DATA: [], TREE: []}, [])
        if self.existing_packs:
            if instant_delete:
                up.delete_unindexed = list(self.existing_packs)
            else:
                for pid, size in self.existing_packs.items():
                    up.adds.append((PackRecord(pid, DATA, 0, 0, prune_time, size), True))
        T = PackToDo
        for index in self.index_files:
            for p in index.packs:
                keep_time = PackRecord(p.id, p.blob_type, p.first, p.count,
                                       p.time if p.time is not None else prune_time, None)
                new_time = keep_time._replace(time=prune_time)
                if p.to_do == T.Undecided:
                    raise RusticError(ErrorKind.Internal,
                                      f"Pack `{p.id.hex()}` got no decision what to do with it!")
                if p.to_do == T.Keep:
                    up.adds.append((keep_time, False))
                elif p.to_do in (T.Repack, T.MarkDelete):
                    if instant_delete:
                        up.delete_packs[p.blob_type].append(p.id)
                    else:
                        up.adds.append((new_time, True))
                elif p.to_do in (T.KeepMarked, T.KeepMarkedAndCorrect):
                    if instant_delete:
                        up.delete_packs[p.blob_type].append(p.id)
                    else:
                        up.adds.append((keep_time, True))
                elif p.to_do == T.Recover:
                    up.adds.append((new_time, False))
                else:  # Delete
                    up.delete_packs[p.blob_type].append(p.id)
        return up

    def write_index(self, key, indexer=None, prune_time: Optional[str] = None,
                    instant_delete: Optional[bool] = None, save=None, device: Optional[int] = None,
                    **indexer_args):
        """``index_updates`` fed into a ``DeviceIndexer`` over the plan's own
        entry arrays (``indexer``, or a new one made with ``save``, ``key``
        and ``indexer_args``).  Returns the indexer, not finalized, with the
        IndexUpdates as its ``updates``: the caller runs
        ``BlobCopier(.., indexer=it)`` over ``repack_plans()`` and finalizes
        it, as prune.rs:1356-1431 does."""
        from .index import rustic_time
        from .index_write import DeviceIndexer
        if instant_delete is None:
            instant_delete = self._opts.instant_delete
        if device is None:
            device = self._dev.index if getattr(self, "_dev", None) is not None else 0
        if indexer is None:
            indexer = DeviceIndexer(save, device=int(device or 0), key=key, **indexer_args)
        up = self.index_updates(prune_time or rustic_time(), instant_delete)
        entries = (self._ids, self._offsets, self._lens, self._ulens)
        for rec, delete in up.adds:
            indexer.add(rec, delete, entries=entries)
        indexer.updates = up
        return indexer

    def size_after_prune(self) -> Dict[int, int]:
        """prune.rs:1373-1377."""
        return {t: self.stats.size[t].total_after_prune()
                + self.stats.blobs[t].total_after_prune() * ENTRY_LEN_COMPRESSED
                for t in (DATA, TREE)}

    def pack_sizers(self) -> Dict[int, PackSizer]:
        """prune.rs:1380-1382: the fixed PackSizer per type for BlobCopier."""
        return {t: PackSizer.fixed(PackSizer.from_config(self._config, t, s).pack_size())
                for t, s in self.size_after_prune().items()}
