"""The blob index in device memory (rcdc_dindex in include/rcdc.h): build it
from index files, look ids up in batches that are already in HBM, run the
packer's dedup rule there.

Reference: ``index/binarysorted.rs`` -- ``IndexCollector`` (:87-163, one
``TypeIndexCollector`` per blob type: the pack id table, the entries and
``total_size``), ``IndexType`` (:23-32) and ``ReadIndex for Index``
(:230-261: ``get_id``, ``total_size``, ``has``).  The reference sorts the
entries and binary-searches them; here they stay in the order added behind a
hash table, and among several entries of one id the first added wins (what
``restore.index_lookup`` promises too).  ``first_new`` is ``Packer::add``'s
rule (packer.rs:304-315), ``count_used`` the saturating count of
``Pruner::count_used_blobs`` (prune.rs:770-784).  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import enum
from typing import Iterable, List, Optional, Tuple

import numpy as np

from . import _lib
from .errors import ErrorKind, RusticError, status_error
from .index import IndexBlob, IndexPack

DATA, TREE = 0, 1  # BlobType, as index.IndexBlob.type
MISS = 0xFFFFFFFF
NO_PACK = 0xFFFFFFFF
DEVICE_PTRS = 1

# rcdc_dindex_loc / rcdc_dindex_hit as numpy records
LOC = np.dtype([("pack", "<u4"), ("offset", "<u4"), ("length", "<u4"),
                ("uncompressed_length", "<u4")])
HIT = np.dtype([("entry", "<u4"), ("count", "<u4"), ("pack", "<u4"), ("offset", "<u4"),
                ("length", "<u4"), ("uncompressed_length", "<u4")])
# columns of the (n, 6) int32 tensor ``lookup`` returns (HIT's fields; view
# the host copy as uint32: a miss's entry is -1 as int32)
COL_ENTRY, COL_COUNT, COL_PACK, COL_OFFSET, COL_LENGTH, COL_ULEN = range(6)


class IndexType(enum.Enum):
    """binarysorted.rs:23-32: what is kept for data blobs (trees are always
    kept in full)."""
    FULL = "Full"
    DATA_IDS = "DataIds"
    ONLY_TREES = "OnlyTrees"


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


def _check_type(tpe) -> int:
    if tpe not in (DATA, TREE) or isinstance(tpe, bool):
        raise RusticError(ErrorKind.InvalidInput, f"unknown blob type {tpe!r}")
    return int(tpe)


def _check_ids(ids):
    """An (n, 32) uint8 numpy array or torch tensor, or InvalidInput."""
    shape = tuple(getattr(ids, "shape", ()))
    if isinstance(ids, np.ndarray):
        ok = ids.dtype == np.uint8
    else:
        ok = hasattr(ids, "data_ptr") and str(getattr(ids, "dtype", "")) == "torch.uint8"
    if not ok or len(shape) != 2 or shape[1] != 32:
        raise RusticError(ErrorKind.InvalidInput,
                          "ids must be an (n, 32) uint8 numpy array or device tensor")
    return ids


def _ids_array(ids: Iterable[bytes]) -> np.ndarray:
    ids = [bytes(i) for i in ids]
    if any(len(i) != 32 for i in ids):
        raise RusticError(ErrorKind.InvalidInput, "a blob id has 32 bytes")
    return np.frombuffer(b"".join(ids), np.uint8).reshape(len(ids), 32)


class _TypeIndex:
    """TypeIndex (binarysorted.rs:61-66): the pack ids by pack number, the
    total size, and the device index (created at its first use)."""

    def __init__(self, mode: str):
        self.mode = mode  # "full", "ids" or "none" (EntriesVariants)
        self.packs: List[bytes] = []
        self.total_size = 0
        self.handle = None


class DeviceIndex:
    """One rcdc_dindex per blob type on ``device``.

    Batched calls take ids as an ``(n, 32)`` uint8 device tensor (or a numpy
    array, which is uploaded) and return device tensors; they are queued on
    the current torch stream of the device."""

    def __init__(self, device: int = 0, index_type: IndexType = IndexType.FULL):
        if not isinstance(index_type, IndexType):
            raise RusticError(ErrorKind.InvalidInput, f"unknown index type {index_type!r}")
        self.device = int(device)
        self.index_type = index_type
        data = {IndexType.FULL: "full", IndexType.DATA_IDS: "ids",
                IndexType.ONLY_TREES: "none"}[index_type]
        self._t = {DATA: _TypeIndex(data), TREE: _TypeIndex("full")}

    @classmethod
    def from_index_files(cls, files, device: int = 0,
                         index_type: IndexType = IndexType.FULL) -> "DeviceIndex":
        """The ``packs`` of index.IndexFiles; ``packs_to_delete`` is ignored,
        as the collector never sees it."""
        dx = cls(device, index_type)
        dx.extend(p for f in files for p in f.packs)
        return dx

    # ---- plumbing ----------------------------------------------------------
    def _torch(self):
        import torch
        return torch, torch.device("cuda", self.device)

    def _stream(self, torch, dev) -> int:
        return int(torch.cuda.current_stream(dev).cuda_stream)

    def _handle(self, t: _TypeIndex):
        if t.handle is None:
            from .crypto import _ctx
            h = ctypes.c_void_p()
            _check(_lib.lib().rcdc_dindex_create(_ctx(self.device).handle, 0, ctypes.byref(h)))
            t.handle = h
        return t.handle

    def _device_ids(self, torch, dev, ids):
        _check_ids(ids)
        if isinstance(ids, np.ndarray):
            if not len(ids):
                return torch.empty((0, 32), dtype=torch.uint8, device=dev)
            ids = np.ascontiguousarray(ids)
            return torch.from_numpy(ids if ids.flags.writeable else ids.copy()).to(dev)
        if ids.device != dev:
            raise RusticError(ErrorKind.InvalidInput, f"ids are on {ids.device}, the index on {dev}")
        ids = ids.contiguous()
        return ids.clone() if ids.data_ptr() % 16 else ids

    def _add(self, t: _TypeIndex, ids, locs, flags: int) -> None:
        """ids / locs: numpy arrays (host pointers) or device tensors."""
        n = len(ids)
        if not n:
            return
        torch, dev = self._torch()
        ptr = (lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
        with torch.cuda.device(dev):
            _check(_lib.lib().rcdc_dindex_add(self._handle(t), ptr(ids),
                                              None if locs is None else ptr(locs), n, flags,
                                              self._stream(torch, dev)))

    def close(self) -> None:
        for t in self._t.values():
            if t.handle is not None:
                _lib.lib().rcdc_dindex_destroy(t.handle)
                t.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- loading -----------------------------------------------------------
    def extend(self, packs: Iterable[IndexPack]) -> None:
        """Extend<IndexPack> for IndexCollector (binarysorted.rs:127-163):
        every pack goes to the type of its first blob (an empty pack to
        data), gets the next pack number there and adds its ``pack_size()``
        to the type's total; its blobs become entries in order.  One device
        add per type and call."""
        ids = {DATA: [], TREE: []}
        locs = {DATA: [], TREE: []}
        for p in packs:
            tpe = _check_type(p.blobs[0].type) if p.blobs else DATA
            t = self._t[tpe]
            no = len(t.packs)  # the pack's number in its type
            t.packs.append(bytes(p.id))
            t.total_size += int(p.pack_size())
            if t.mode == "none":
                continue
            for b in p.blobs:
                ids[tpe].append(bytes(b.id))
                locs[tpe].append((no, int(b.offset), int(b.length),
                                  int(b.uncompressed_length or 0)))
        for tpe in (DATA, TREE):
            t = self._t[tpe]
            if not ids[tpe]:
                continue
            a = _ids_array(ids[tpe])
            l = np.array(locs[tpe], dtype=np.uint32).view(LOC).ravel() if t.mode == "full" else None
            self._add(t, a, l, 0)

    def add_ids(self, d_ids) -> None:
        """Id-only data entries (no pack yet): the blobs the packer holds
        before their pack is indexed."""
        t = self._t[DATA]
        _check_ids(d_ids)
        if t.mode == "none" or not len(d_ids):
            return
        if isinstance(d_ids, np.ndarray):
            self._add(t, np.ascontiguousarray(d_ids), None, 0)
        else:
            torch, dev = self._torch()
            self._add(t, self._device_ids(torch, dev, d_ids), None, DEVICE_PTRS)

    # ---- sizes ---------------------------------------------------------------
    def total_size(self, tpe: int) -> int:
        return self._t[_check_type(tpe)].total_size

    def packs(self, tpe: int) -> List[bytes]:
        return list(self._t[_check_type(tpe)].packs)

    def size(self, tpe: int) -> int:
        """Entries of the type (every added blob counts)."""
        t = self._t[_check_type(tpe)]
        return 0 if t.handle is None else int(_lib.lib().rcdc_dindex_size(t.handle))

    def keys(self, tpe: int) -> int:
        """Distinct ids of the type."""
        t = self._t[_check_type(tpe)]
        return 0 if t.handle is None else int(_lib.lib().rcdc_dindex_keys(t.handle))

    def __len__(self) -> int:
        return self.size(DATA) + self.size(TREE)

    # ---- lookups -------------------------------------------------------------
    def lookup(self, tpe: int, d_ids):
        """(n, 6) int32 device tensor of rcdc_dindex_hit records (COL_*): per
        id the lowest entry, how many entries carry it, and that entry's
        pack number, offset, length and uncompressed length (0 for None)."""
        t = self._t[_check_type(tpe)]
        _check_ids(d_ids)
        torch, dev = self._torch()
        with torch.cuda.device(dev):
            d_ids = self._device_ids(torch, dev, d_ids)
            n = int(d_ids.shape[0])
            hits = torch.empty((n, 6), dtype=torch.int32, device=dev)
            if t.mode == "none" or t.handle is None:
                hits.zero_()
                hits[:, COL_ENTRY] = -1
                return hits
            _check(_lib.lib().rcdc_dindex_lookup(t.handle, d_ids.data_ptr(), n, hits.data_ptr(),
                                                 self._stream(torch, dev)))
        return hits

    def has(self, tpe: int, ids):
        """ReadIndex::has.  One id (bytes) -> bool; a batch -> bool device
        tensor."""
        if isinstance(ids, (bytes, bytearray, memoryview)):
            _check_type(tpe)
            return bool(self.has(tpe, _ids_array([ids])).cpu().numpy()[0])
        return self.lookup(tpe, ids)[:, COL_COUNT] != 0

    def count_used(self, tpe: int, d_ids):
        """min(count, 255) per id as uint8: 0 is a blob the index lacks."""
        torch, _ = self._torch()
        c = self.lookup(tpe, d_ids)[:, COL_COUNT]
        return torch.where((c < 0) | (c > 255), torch.full_like(c, 255), c).to(torch.uint8)

    def entries(self, tpe: int, ids: Iterable[bytes]) -> List[Optional[Tuple[bytes, IndexBlob]]]:
        """get_id for a list of ids in one device call: (pack id, IndexBlob)
        per id, None where the index lacks it or keeps no location."""
        tpe = _check_type(tpe)
        ids = [bytes(i) for i in ids]
        t = self._t[tpe]
        arr = _ids_array(ids)
        if t.mode != "full" or t.handle is None or not ids:
            return [None] * len(ids)
        h = self.lookup(tpe, arr).cpu().numpy().view(np.uint32)
        out: List[Optional[Tuple[bytes, IndexBlob]]] = []
        for i, r in zip(ids, h):
            if int(r[COL_ENTRY]) == MISS or int(r[COL_PACK]) == NO_PACK:
                out.append(None)
            else:
                out.append((t.packs[int(r[COL_PACK])],
                            IndexBlob(i, tpe, int(r[COL_OFFSET]), int(r[COL_LENGTH]),
                                      int(r[COL_ULEN]) or None)))
        return out

    def get_id(self, tpe: int, id_: bytes) -> Optional[Tuple[bytes, IndexBlob]]:
        """ReadIndex::get_id."""
        return self.entries(tpe, [id_])[0]

    def get(self, id_: bytes) -> Optional[Tuple[bytes, IndexBlob]]:
        """A data blob's entry: what ``restore.index_lookup``'s dict answers."""
        return self.get_id(DATA, id_)

    # ---- backup ----------------------------------------------------------------
    def first_new(self, d_ids, select=None):
        """The packer's rule over one batch of data blob ids: bool device
        tensor, true where the id is selected (``select``: n flags, None for
        all), not in the index, and not selected earlier in the batch."""
        t = self._t[DATA]
        _check_ids(d_ids)
        torch, dev = self._torch()
        with torch.cuda.device(dev):
            d_ids = self._device_ids(torch, dev, d_ids)
            n = int(d_ids.shape[0])
            sel = None
            if select is not None:
                if isinstance(select, np.ndarray):
                    select = torch.from_numpy(np.ascontiguousarray(select))
                sel = (select != 0).to(device=dev, dtype=torch.uint8).contiguous()
                if tuple(sel.shape) != (n,):
                    raise RusticError(ErrorKind.InvalidInput, "select must have one flag per id")
            out = torch.empty(n, dtype=torch.uint8, device=dev)
            if n:
                _check(_lib.lib().rcdc_dindex_first_new(
                    self._handle(t), d_ids.data_ptr(), n, None if sel is None else sel.data_ptr(),
                    out.data_ptr(), self._stream(torch, dev)))
        return out != 0
