"""Index files written on the device (rcdc_index_write in include/rcdc.h): the
reverse of ``dindex.parse_json`` / ``DeviceIndex.load``.

Reference:
- ``repofile/indexfile.rs:24-143``: what ``serde_json::to_vec(&IndexFile)``
  writes -- ``index.IndexFile.to_json`` is that text and the contract for
  every byte of ``write_json``;
- ``backend/decrypt.rs:273-290,441-459``: ``save_file`` / ``encrypt_file``,
  here for a whole batch in HBM (``save_index_files``);
- ``index/indexer.rs:114-180``: the rule by which packs become index files
  (``DeviceIndexer``; ``index.Indexer`` is the same rule over host objects
  and stays the yardstick).

The blobs are entries of device arrays -- the ``ids`` / ``locs`` of a parse,
the arrays of a ``prune.PrunePlan`` -- and no object per blob is made on the
host: a pack is one record (id, type, first, count, time, size), a file one
record over pack records.  No CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import ErrorKind, RusticError, status_error
from .index import MAX_COUNT, IndexPack

DATA, TREE = 0, 1
HAS_TIME, HAS_SIZE = 1, 2  # RCDC_IXWRITE_HAS_TIME / RCDC_IXWRITE_HAS_SIZE
MAX_TIME = 64              # RCDC_IXWRITE_MAX_TIME

# rcdc_ixwrite_pack / _file / _out as numpy records
IXW_PACK = np.dtype([("id", "u1", (32,)), ("first", "<u8"), ("count", "<u4"), ("type", "<u4"),
                     ("flags", "<u4"), ("size", "<u4"), ("time_off", "<u4"), ("time_len", "<u4")])
IXW_FILE = np.dtype([("pack_first", "<u8"), ("pack_count", "<u4"), ("n_delete", "<u4"),
                     ("sup_first", "<u8"), ("sup_count", "<u4"), ("has_supersedes", "<u4")])
IXW_OUT = np.dtype([("off", "<u8"), ("len", "<u8")])


class PackRecord(NamedTuple):
    """A pack whose blobs are the entries [first, first + count)."""
    id: bytes
    type: int
    first: int
    count: int
    time: Optional[str] = None
    size: Optional[int] = None


class FileRecord(NamedTuple):
    """An index file: the pack records [pack_first, pack_first + pack_count),
    the last ``n_delete`` of them its packs_to_delete."""
    pack_first: int
    pack_count: int
    n_delete: int = 0
    supersedes: Optional[Sequence[bytes]] = None


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


def write_span() -> int:
    """Bytes of output one wave of the emit pass owns (RCDC_IXWRITE_SPAN)."""
    return int(_lib.lib().rcdc_index_write_span())


def write_bound(n_entries: int, n_packs: int, n_files: int, n_supersedes: int = 0,
                time_bytes: int = 0) -> int:
    """Output bytes that always suffice for these WRITTEN counts."""
    return int(_lib.lib().rcdc_index_write_bound(int(n_entries), int(n_packs), int(n_files),
                                                 int(n_supersedes), int(time_bytes)))


def pack_records(packs: Iterable) -> Tuple[np.ndarray, bytes]:
    """(IXW_PACK records, the time arena) of PackRecords (or tuples in that
    order)."""
    packs = [p if isinstance(p, PackRecord) else PackRecord(*p) for p in packs]
    recs = np.zeros(len(packs), IXW_PACK)
    times, where = bytearray(), {}
    for r, p in zip(recs, packs):
        pid = bytes(p.id)
        if len(pid) != 32:
            raise RusticError(ErrorKind.InvalidInput, "a pack id has 32 bytes")
        if not 0 <= int(p.first) < 1 << 64 or not 0 <= int(p.count) < 1 << 32:
            raise RusticError(ErrorKind.InvalidInput, "a pack's entry range is out of range")
        if isinstance(p.type, bool) or not 0 <= int(p.type) < 1 << 32:
            raise RusticError(ErrorKind.InvalidInput, f"unknown blob type {p.type!r}")
        r["id"] = np.frombuffer(pid, np.uint8)
        r["first"], r["count"], r["type"] = int(p.first), int(p.count), int(p.type)
        flags = 0
        if p.time is not None:
            t = p.time.encode() if isinstance(p.time, str) else bytes(p.time)
            if t not in where:
                where[t] = len(times)
                times += t
            r["time_off"], r["time_len"] = where[t], len(t)
            flags |= HAS_TIME
        if p.size is not None:
            if not 0 <= int(p.size) < 1 << 32:
                raise RusticError(ErrorKind.InvalidInput, "a pack size is a u32")
            r["size"] = int(p.size)
            flags |= HAS_SIZE
        r["flags"] = flags
    return recs, bytes(times)


def file_records(files: Iterable) -> Tuple[np.ndarray, np.ndarray]:
    """(IXW_FILE records, (k, 32) supersedes ids) of FileRecords."""
    files = [f if isinstance(f, FileRecord) else FileRecord(*f) for f in files]
    recs = np.zeros(len(files), IXW_FILE)
    sup: List[bytes] = []
    for r, f in zip(recs, files):
        r["pack_first"], r["pack_count"], r["n_delete"] = \
            int(f.pack_first), int(f.pack_count), int(f.n_delete)
        if f.supersedes is not None:
            ids = [bytes(s) for s in f.supersedes]
            if any(len(s) != 32 for s in ids):
                raise RusticError(ErrorKind.InvalidInput, "an index id has 32 bytes")
            r["has_supersedes"], r["sup_first"], r["sup_count"] = 1, len(sup), len(ids)
            sup += ids
    return recs, np.frombuffer(b"".join(sup), np.uint8).reshape(len(sup), 32)


class WrittenJson:
    """rcdc_index_write's output: ``data`` (uint8 device tensor, ``total``
    bytes) holds file i at ``offs[i]``, ``lens[i]`` bytes; ``raw`` is the
    whole allocation, the capacity and the guard bytes included."""

    def __init__(self, data, offs, lens, total, raw, cap):
        self.data, self.offs, self.lens, self.total = data, offs, lens, total
        self.raw, self.cap = raw, cap

    def __len__(self) -> int:
        return len(self.lens)

    def file(self, i: int):
        o, n = int(self.offs[i]), int(self.lens[i])
        return self.data[o:o + n]

    def to_bytes(self) -> List[bytes]:
        """The files on the host (tests, small batches)."""
        h = self.data.cpu().numpy()
        return [h[int(o):int(o) + int(n)].tobytes() for o, n in zip(self.offs, self.lens)]


def _int_tensor(torch, dev, a, what: str):
    """A 1-D tensor of 4-byte integers on ``dev``; numpy arrays are uploaded."""
    if isinstance(a, np.ndarray):
        a = np.array(a, dtype=np.uint32).reshape(-1)  # a copy torch may take over
        return torch.from_numpy(a.view(np.int32)).to(dev)
    if not hasattr(a, "data_ptr") or a.device != dev:
        raise RusticError(ErrorKind.InvalidInput, f"{what} must be a tensor on {dev}")
    if a.dim() != 1 or a.element_size() != 4 or a.is_floating_point():
        raise RusticError(ErrorKind.InvalidInput, f"{what}: one 4-byte integer per entry")
    return a


def _id_tensor(torch, dev, ids):
    if isinstance(ids, np.ndarray):
        ids = np.array(ids, dtype=np.uint8).reshape(-1, 32)
        return torch.from_numpy(ids).to(dev)
    if not hasattr(ids, "data_ptr") or ids.device != dev:
        raise RusticError(ErrorKind.InvalidInput, f"ids must be a tensor on {dev}")
    if ids.dtype != torch.uint8 or ids.dim() != 2 or ids.shape[1] != 32 or \
            (ids.shape[0] and ids.stride(1) != 1):
        raise RusticError(ErrorKind.InvalidInput, "ids must be (n, 32) uint8 with dense rows")
    return ids


def write_json(ids, offsets, lens, ulens, packs, files, device: int = 0,
               guard: int = 0) -> WrittenJson:
    """The JSON text of the index files ``files`` (FileRecords over the
    PackRecords ``packs``, or what ``pack_records`` / ``file_records`` made of
    them) whose blobs are entries of ``ids`` ((n, 32) uint8), ``offsets``,
    ``lens`` and ``ulens`` (n 4-byte integers each, 0 for no uncompressed
    length): device tensors, strided views allowed; numpy arrays are
    uploaded.  Byte for byte what ``IndexFile.to_json`` writes.  Queued on
    the current torch stream.  ``guard``: that many bytes of 0xA5 behind the
    capacity, and 0xA5 wherever no file is written (in ``raw``), for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    made = lambda x: isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], np.ndarray)
    p_recs, times = packs if made(packs) else pack_records(packs)
    f_recs, sup = files if made(files) else file_records(files)
    p_recs = np.ascontiguousarray(p_recs, IXW_PACK)
    f_recs = np.ascontiguousarray(f_recs, IXW_FILE)
    sup = np.ascontiguousarray(sup, np.uint8).reshape(-1, 32)
    n_files, n_packs = len(f_recs), len(p_recs)
    # the written counts, for the capacity (the call checks the ranges)
    n_w = n_wp = t_w = 0
    for f in f_recs:
        a, c = int(f["pack_first"]), int(f["pack_count"])
        if a + c > n_packs:
            raise RusticError(ErrorKind.InvalidInput, "a file's packs lie outside the pack records")
        part = p_recs[a:a + c]
        n_w += int(part["count"].sum(dtype=np.uint64))
        n_wp += c
        t_w += int(part["time_len"][(part["flags"] & HAS_TIME) != 0].sum(dtype=np.uint64))
    n_sup = int(f_recs["sup_count"][f_recs["has_supersedes"] != 0].sum(dtype=np.uint64))
    cap = (write_bound(n_w, n_wp, n_files, n_sup, t_w) + 15) // 16 * 16
    with torch.cuda.device(dev):
        d_ids = _id_tensor(torch, dev, ids)
        ints = [_int_tensor(torch, dev, a, what)
                for a, what in ((offsets, "offsets"), (lens, "lens"), (ulens, "ulens"))]
        n = int(d_ids.shape[0])
        if any(int(a.shape[0]) != n for a in ints):
            raise RusticError(ErrorKind.InvalidInput, "one offset, length and uncompressed "
                                                      "length per id")
        # 16 spare bytes: the AEAD and the encoder may read 4 past an input
        raw = torch.full((cap + 16 + guard,), 0xA5, dtype=torch.uint8, device=dev) if guard \
            else torch.empty(cap + 16, dtype=torch.uint8, device=dev)
        # a lone row's stride is whatever the view says: give the element's size
        stride = lambda t, unit: int(t.stride(0)) * unit if n > 1 else unit
        out = np.zeros(max(n_files, 1), IXW_OUT)
        total = ctypes.c_uint64(0)
        tbuf = ctypes.create_string_buffer(times, len(times)) if times else None
        _check(_lib.lib().rcdc_index_write(
            _ctx(int(device)).handle, d_ids.data_ptr() if n else None, stride(d_ids, 1),
            ints[0].data_ptr() if n else None, stride(ints[0], 4),
            ints[1].data_ptr() if n else None, stride(ints[1], 4),
            ints[2].data_ptr() if n else None, stride(ints[2], 4), n,
            p_recs.ctypes.data if n_packs else None, n_packs,
            f_recs.ctypes.data if n_files else None, n_files,
            sup.ctypes.data if len(sup) else None, len(sup),
            ctypes.addressof(tbuf) if tbuf is not None else None, len(times),
            raw.data_ptr(), cap, out.ctypes.data, ctypes.byref(total),
            int(torch.cuda.current_stream(dev).cuda_stream)))
    out = out[:n_files]
    return WrittenJson(raw[:int(total.value)], out["off"].astype(np.int64),
                       out["len"].astype(np.int64), int(total.value), raw, cap)


def _pad16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


@contextlib.contextmanager
def _stage(times: Optional[dict], name: str, torch, dev):
    if times is None:
        yield
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream(dev))
    try:
        yield
    finally:
        b.record(torch.cuda.current_stream(dev))
        b.synchronize()
        times[name] = times.get(name, 0.0) + a.elapsed_time(b)


def save_index_files(key, written: WrittenJson, version: int = 2, level: int = 0, nonces=None,
                     device: int = 0, stage_times: Optional[dict] = None):
    """``save_file`` / ``encrypt_file`` (backend/decrypt.rs:273-290,441-459)
    for every file of ``written`` in HBM: version 2 seals ``2 || zstd frame``
    of the text, version 1 the text; the file id is the device SHA-256 of
    the sealed bytes.  The frames are compressed 16 bytes into a slot each,
    so the marker byte goes in front of its frame without a copy.  Only the
    frame lengths and the ids come to the host.  Returns (ids, the sealed
    uint8 device tensor, offs, lens).  ``nonces``: one 16-byte nonce per file
    (random when None).  ``stage_times``: a dict that gets the device time of
    the stages in milliseconds (every stage then waits)."""
    import torch
    from .compress import compress_blobs, make_refs as zstd_refs, zstd_bounds
    from .crypto import _ctx, make_refs as aead_refs
    from .read import _sha256
    dev = torch.device("cuda", int(device))
    n = len(written)
    if not n:
        return [], torch.empty(0, dtype=torch.uint8, device=dev), np.zeros(0, np.int64), \
            np.zeros(0, np.int64)
    if nonces is None:
        nonces = np.frombuffer(os.urandom(16 * n), np.uint8).reshape(n, 16)
    else:
        nonces = np.frombuffer(b"".join(bytes(x) for x in nonces), np.uint8).reshape(n, 16)
    t_offs = np.asarray(written.offs, np.int64)
    t_lens = np.asarray(written.lens, np.int64)
    with torch.cuda.device(dev):
        ctx = _ctx(int(device))
        stream = int(torch.cuda.current_stream(dev).cuda_stream)
        if version >= 2:
            slots = 16 + (zstd_bounds(t_lens) + 15) // 16 * 16
            base = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64)
            frames = torch.empty(int(slots.sum()) + 16, dtype=torch.uint8, device=dev)
            with _stage(stage_times, "compress", torch, dev):
                f_lens = compress_blobs(ctx, written.raw.data_ptr(),
                                        zstd_refs(t_offs, t_lens, base + 16), frames.data_ptr(),
                                        level, stream).astype(np.int64)
                frames[torch.from_numpy(base + 15).to(dev)] = 2
            src, in_offs, in_lens = frames, base + 15, f_lens + 1
        else:
            src, in_offs, in_lens = written.raw, t_offs, t_lens
        s_lens = in_lens + 32
        s_offs = np.concatenate([[0], np.cumsum((s_lens + 15) // 16 * 16)[:-1]]).astype(np.int64)
        sealed = torch.empty(int(s_offs[-1]) + _pad16(int(s_lens[-1])), dtype=torch.uint8,
                             device=dev)
        with _stage(stage_times, "seal", torch, dev):
            key.seal_blobs(src.data_ptr(), aead_refs(in_offs, in_lens, s_offs, nonces),
                           sealed.data_ptr(), stream, ctx)
        with _stage(stage_times, "sha256", torch, dev):
            ids = _sha256(ctx, sealed, s_offs, s_lens)
    return ids, sealed, s_offs, s_lens


class _Source:
    """One set of entry arrays a DeviceIndexer's records point into."""

    def __init__(self, ids, offsets, lens, ulens):
        self.ids, self.offsets, self.lens, self.ulens = ids, offsets, lens, ulens


class DeviceIndexer:
    """``index.Indexer`` (index/indexer.rs:114-180) for packs whose blobs are
    device entries.  ``add`` takes a PackRecord into entry arrays -- those of
    ``entries`` = (ids, offsets, lens, ulens) given here, or given with the
    call -- or a host ``index.IndexPack``, whose blobs are staged and
    uploaded with the next save; so it serves as ``BlobCopier``'s indexer.

    A file closes when it holds ``max_count`` blobs or more after an add, as
    in ``Indexer.add``.  Closed files are written (``write_json``) and sealed
    (``save_index_files`` with ``key``, ``version``, ``level``) in one batch
    at ``finalize``, or as soon as ``flush_files`` of them are closed;
    ``save(ids, sealed, offs, lens)`` is the caller's backend write.  The ids
    of the files saved are in ``saved``.  ``indexed``: a set to track the
    blob ids of host packs for ``has`` (None: Indexer::new_unindexed)."""

    def __init__(self, save, max_count: int = MAX_COUNT, device: int = 0, key=None, entries=None,
                 version: int = 2, level: int = 0, flush_files: Optional[int] = None,
                 indexed: Optional[set] = None):
        self._save = save
        self.max_count = int(max_count)
        self.device = int(device)
        self.key, self.version, self.level = key, int(version), int(level)
        self.flush_files = flush_files
        self.indexed = indexed
        self.saved: List[bytes] = []
        self.count = 0
        self._sources: List[_Source] = []
        self._default = self._source(entries) if entries is not None else None
        # staged blobs of host packs since the last flush
        self._h_ids: List[bytes] = []
        self._h_ints: List[Tuple[int, int, int]] = []
        # the open file and the closed ones: lists of (source number or None
        # for staged, PackRecord), packs and packs_to_delete apart
        self._open: Tuple[list, list] = ([], [])
        self._closed: List[Tuple[list, list]] = []

    def _source(self, entries) -> int:
        for k, s in enumerate(self._sources):
            if s.ids is entries[0] and s.offsets is entries[1]:
                return k
        self._sources.append(_Source(*entries))
        return len(self._sources) - 1

    def add(self, pack, delete: bool = False, entries=None) -> None:
        if isinstance(pack, IndexPack):
            types = {int(b.type) for b in pack.blobs}
            if len(types) > 1:
                raise RusticError(ErrorKind.InvalidInput,
                                  f"pack `{bytes(pack.id).hex()}` holds blobs of two types")
            rec = PackRecord(bytes(pack.id), types.pop() if types else DATA, len(self._h_ids),
                             len(pack.blobs), pack.time, pack.size)
            for b in pack.blobs:
                if len(bytes(b.id)) != 32:
                    raise RusticError(ErrorKind.InvalidInput, "a blob id has 32 bytes")
                self._h_ids.append(bytes(b.id))
                self._h_ints.append((int(b.offset), int(b.length), int(b.uncompressed_length or 0)))
                if self.indexed is not None:
                    self.indexed.add(bytes(b.id))
            src = None
        else:
            rec = pack if isinstance(pack, PackRecord) else PackRecord(*pack)
            if entries is None and self._default is None:
                raise RusticError(ErrorKind.InvalidInput, "a record needs entry arrays")
            src = self._source(entries) if entries is not None else self._default
        self.count += int(rec.count)
        self._open[1 if delete else 0].append((src, rec))
        if self.count >= self.max_count:
            self._close()
            if self.flush_files and len(self._closed) >= self.flush_files:
                self.flush()

    def add_remove(self, pack, entries=None) -> None:  # indexer.rs add_remove
        self.add(pack, True, entries)

    def _close(self) -> None:
        if self._open[0] or self._open[1]:  # Indexer::save: an empty file is not written
            self._closed.append(self._open)
        self._open = ([], [])
        self.count = 0

    def has(self, blob_id: bytes) -> bool:
        return self.indexed is not None and bytes(blob_id) in self.indexed

    def finalize(self) -> None:
        self._close()
        self.flush()

    def _arrays(self, used: List[Optional[int]]):
        """One set of entry arrays over the sources ``used`` (None: the staged
        host blobs) and each source's first entry in it."""
        parts = []
        for s in used:
            if s is None:
                ids = np.frombuffer(b"".join(self._h_ids), np.uint8).reshape(-1, 32)
                ints = np.array(self._h_ints, np.uint32).reshape(-1, 3)
                parts.append((ids, ints[:, 0], ints[:, 1], ints[:, 2]))
            else:
                e = self._sources[s]
                parts.append((e.ids, e.offsets, e.lens, e.ulens))
        base, o = {}, 0
        for s, p in zip(used, parts):
            base[s] = o
            o += int(p[0].shape[0])
        if len(parts) == 1:
            return parts[0], base
        if all(isinstance(a, np.ndarray) for p in parts for a in p):
            return tuple(np.concatenate([p[k] for p in parts]) for k in range(4)), base
        # several sources: one copy of each on the device, back to back
        import torch
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            parts = [(_id_tensor(torch, dev, p[0]),) + tuple(
                _int_tensor(torch, dev, p[k], "an integer array") for k in (1, 2, 3)) for p in parts]
            cat = (torch.cat([p[0] for p in parts]),) + tuple(
                torch.cat([p[k].contiguous().view(torch.int32) for p in parts]) for k in (1, 2, 3))
        return cat, base

    def flush(self) -> None:
        """Write, seal and save the files closed so far."""
        if not self._closed:
            return
        if self.key is None:
            raise RusticError(ErrorKind.InvalidInput, "DeviceIndexer needs a key to seal with")
        used: List[Optional[int]] = []
        for f in self._closed:
            for part in f:
                for s, _ in part:
                    if s not in used:
                        used.append(s)
        arrays, base = self._arrays(used)
        packs, files = [], []
        for f in self._closed:
            first = len(packs)
            for part in f:
                for s, r in part:
                    packs.append(r._replace(first=int(r.first) + base.get(s, 0)))
            files.append(FileRecord(first, len(packs) - first, len(f[1])))
        written = write_json(arrays[0], arrays[1], arrays[2], arrays[3], packs, files, self.device)
        ids, sealed, offs, lens = save_index_files(self.key, written, self.version, self.level,
                                                   device=self.device)
        self._save(ids, sealed, offs, lens)
        self.saved += ids
        self._closed = []
        # staged blobs of the open file stay, renumbered from 0
        keep = sorted({(int(r.first), int(r.count)) for part in self._open for s, r in part
                       if s is None})
        ids_, ints_, moved = [], [], {}
        for a, c in keep:
            moved[a] = len(ids_)
            ids_ += self._h_ids[a:a + c]
            ints_ += self._h_ints[a:a + c]
        self._h_ids, self._h_ints = ids_, ints_
        self._open = tuple([(s, r._replace(first=moved[int(r.first)]) if s is None else r)
                            for s, r in part] for part in self._open)
