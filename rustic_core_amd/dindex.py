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

Loading: ``extend`` takes host objects; ``extend_json`` takes the JSON text
of index files that is already in HBM and has the device parse it
(rcdc_index_parse: a strict grammar, a file outside it goes through
``IndexFile.from_json`` on the host), and ``load`` is ``decrypt_file``
(backend/decrypt.rs:421-439) for a batch of sealed index files in front of
that.  ``extend_headers`` takes opened pack headers in HBM (rcdc_pack_header_
parse): what ``headers.index_checked`` adds for packs the index files have
wrong or lack.
"""
from __future__ import annotations

import contextlib
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


# ---- index files parsed on the device (rcdc_index_parse) ----------------------
PARSED, NOT_PARSED = 0, 1  # RCDC_IXPARSE_OK / RCDC_IXPARSE_NOT_PARSED
# rcdc_ixparse_ref / _file / _pack as numpy records
IX_REF = np.dtype([("off", "<u8"), ("len", "<u8")])
IX_FILE = np.dtype([("status", "<u4"), ("packs", "<u4", (2,)), ("packs_to_delete", "<u4"),
                    ("entries", "<u4", (2,))])
IX_PACK = np.dtype([("id", "u1", (32,)), ("type", "<u4"), ("number", "<u4"), ("size", "<u8")])
UNSUPPORTED_MESSAGE = ("Decryption not supported. The data is not in a supported format.")  # decrypt.rs:435
HEAD = 19  # the marker byte and the longest zstd frame header (RFC 8878: 4 + 1 + 1 + 4 + 8)
_BAD = object()


def parse_tile() -> int:
    """The tile size of the device's structural pass (RCDC_IXPARSE_TILE)."""
    return int(_lib.lib().rcdc_index_parse_tile())


def parse_bound(length: int) -> Tuple[int, int]:
    """(entries, packs) that ``length`` bytes of index JSON hold at most."""
    e, p = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.lib().rcdc_index_parse_bound(int(length), ctypes.byref(e), ctypes.byref(p))
    return int(e.value), int(p.value)


class ParsedJson:
    """rcdc_index_parse's outputs: ``ids[t]`` (cap, 32) uint8 and ``locs[t]``
    (cap, 4) int32 device tensors (None where not asked for) of which the
    first ``entries[t]`` rows are written; ``files`` (IX_FILE) and ``packs``
    (IX_PACK, the collected packs in order) on the host."""

    def __init__(self, ids, locs, files, packs, entries, raw):
        self.ids, self.locs, self.files, self.packs, self.entries = ids, locs, files, packs, entries
        self.raw = raw  # the flat allocations behind ids / locs, guard bytes included


def parse_json(d_json, offs, lens, pack_base=(0, 0), device: int = 0, want_ids=(True, True),
               want_locs=(True, True), guard: int = 0) -> ParsedJson:
    """The index files ``d_json[offs[i] : offs[i] + lens[i]]`` (a uint8 device
    tensor) parsed on the device, pack numbers counted from ``pack_base`` per
    type.  ``guard``: that many bytes of 0xA5 behind every output array (in
    ``raw``), for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    n = len(lens)
    if len(offs) != n:
        raise RusticError(ErrorKind.InvalidInput, "one offset per length")
    if not (hasattr(d_json, "data_ptr") and str(d_json.dtype) == "torch.uint8"
            and d_json.dim() == 1 and d_json.is_contiguous() and d_json.device == dev):
        raise RusticError(ErrorKind.InvalidInput,
                          f"d_json must be a contiguous uint8 tensor on {dev}")
    refs = np.zeros(n, IX_REF)
    refs["off"], refs["len"] = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
    cap_e = sum(parse_bound(int(l))[0] for l in lens)
    cap_p = sum(parse_bound(int(l))[1] for l in lens)
    files = np.zeros(n, IX_FILE)
    packs = np.zeros(max(cap_p, 1), IX_PACK)
    result = _lib.IxparseResult()
    base = (ctypes.c_uint32 * 2)(int(pack_base[0]), int(pack_base[1]))
    ids, locs, raw = [None, None], [None, None], []
    with torch.cuda.device(dev):
        for t in (DATA, TREE):
            for arr, want, width in ((ids, want_ids[t], 32), (locs, want_locs[t], 16)):
                if not want:
                    continue
                flat = torch.full((cap_e * width + guard,), 0xA5, dtype=torch.uint8, device=dev) \
                    if guard else torch.empty(cap_e * width, dtype=torch.uint8, device=dev)
                raw.append(flat)
                body = flat[:cap_e * width]
                arr[t] = body.view(cap_e, 32) if width == 32 else body.view(torch.int32).view(cap_e, 4)
        pi = (ctypes.c_void_p * 2)(*[None if a is None else a.data_ptr() for a in ids])
        pl = (ctypes.c_void_p * 2)(*[None if a is None else a.data_ptr() for a in locs])
        _check(_lib.lib().rcdc_index_parse(
            _ctx(int(device)).handle, d_json.data_ptr() if d_json.numel() else None,
            int(d_json.numel()), refs.ctypes.data, n, base, pi, pl, cap_e, files.ctypes.data,
            packs.ctypes.data, cap_p, ctypes.byref(result),
            int(torch.cuda.current_stream(dev).cuda_stream)))
    npacks = int(result.packs[0] + result.packs[1])
    return ParsedJson(ids, locs, files, packs[:npacks],
                      (int(result.entries[0]), int(result.entries[1])), raw)


def _pad16(n: int) -> int:
    return (int(n) + 15) // 16 * 16


def _layout(lens) -> np.ndarray:
    """16-byte aligned offsets of buffers of ``lens`` laid back to back."""
    offs, o = np.zeros(len(lens), np.uint64), 0
    for i, n in enumerate(lens):
        offs[i] = o
        o += _pad16(n)
    return offs


def _frame_content_size(head: bytes):
    """Frame_Content_Size of the zstd frame that starts ``head`` (RFC 8878
    3.1.1.1), None when the header has none, _BAD when ``head`` is no
    complete frame header."""
    if len(head) < 5 or head[:4] != b"\x28\xb5\x2f\xfd":
        return _BAD
    fhd = head[4]
    single = (fhd >> 5) & 1
    fcs_len = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    if not fcs_len:
        return None
    if len(head) < at + fcs_len:
        return _BAD
    v = int.from_bytes(head[at:at + fcs_len], "little")
    return v + 256 if fcs_len == 2 else v


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
        # a dict here makes load / extend_json add the device time of their
        # stages to it (milliseconds by HIP events; every stage then waits)
        self.stage_times: Optional[dict] = None

    @contextlib.contextmanager
    def _stage(self, name: str):
        if self.stage_times is None:
            yield
            return
        torch, dev = self._torch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(dev))
        try:
            yield
        finally:
            b.record(torch.cuda.current_stream(dev))
            b.synchronize()
            self.stage_times[name] = self.stage_times.get(name, 0.0) + a.elapsed_time(b)

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

    def extend_json(self, d_json, offs, lens) -> np.ndarray:
        """``extend`` for index files whose JSON text is in HBM: file i is
        ``d_json[offs[i] : offs[i] + lens[i]]`` (a uint8 device tensor).  The
        batch is parsed on the device (rcdc_index_parse) and its arrays go to
        rcdc_dindex_add as device pointers.  Returns the per-file status
        (PARSED / NOT_PARSED).

        The rule for files the device leaves to the host (outside its
        grammar): files are added in their order.  Consecutive parsed files
        form a run, added with one device add per type; a NOT_PARSED file is
        copied to the host and goes through ``IndexFile.from_json`` and
        ``extend`` between the runs (what ``from_json`` refuses raises here,
        as there, after the files before it were added), and the pack
        numbers of the runs after it are shifted by the packs it added.  So
        pack numbers, entry numbers and sizes are those of ``extend`` over
        all the files in order."""
        from .index import IndexFile
        torch, dev = self._torch()
        base = {t: len(self._t[t].packs) for t in (DATA, TREE)}  # what the parse counts from
        with self._stage("parse"):
            res = parse_json(d_json, offs, lens, (base[DATA], base[TREE]), device=self.device,
                             want_ids=(self._t[DATA].mode != "none", True),
                             want_locs=(self._t[DATA].mode == "full", True))
        e0 = {DATA: 0, TREE: 0}
        p0 = 0
        i, n = 0, len(res.files)
        while i < n:
            if res.files["status"][i] != PARSED:
                o, ln = int(offs[i]), int(lens[i])
                text = d_json[o:o + ln].cpu().numpy().tobytes()
                self.extend(IndexFile.from_json(text).packs)
                i += 1
                continue
            j = i
            while j < n and res.files["status"][j] == PARSED:
                j += 1
            run = res.files[i:j]
            npacks = int(run["packs"].sum())
            for p in res.packs[p0:p0 + npacks]:
                t = self._t[int(p["type"])]
                t.packs.append(p["id"].tobytes())
                t.total_size += int(p["size"])
            p0 += npacks
            for tpe in (DATA, TREE):
                t = self._t[tpe]
                ne = int(run["entries"][:, tpe].sum())
                a, b = e0[tpe], e0[tpe] + ne
                e0[tpe] = b
                if not ne or t.mode == "none":
                    continue
                locs = None
                if t.mode == "full":
                    locs = res.locs[tpe][a:b]
                    # packs added by host files since the parse
                    shift = len(t.packs) - base[tpe] - int(res.files["packs"][:j, tpe].sum())
                    if shift:
                        locs[:, 0] += shift
                with self._stage("add"):
                    self._add(t, res.ids[tpe][a:b], locs, DEVICE_PTRS)
            i = j
        return res.files["status"].copy()

    def extend_headers(self, d_plain, offs, lens, pack_ids) -> np.ndarray:
        """``extend`` for packs whose opened headers are in HBM: header i is
        ``d_plain[offs[i] : offs[i] + lens[i]]`` (a uint8 device tensor) and
        belongs to pack ``pack_ids[i]``.  The batch is parsed on the device
        (rcdc_pack_header_parse) and its arrays go to rcdc_dindex_add as
        device pointers; the pack ids and ``pack_size()`` are recorded per
        type.  Returns the per-header records (``headers.PK_HEADER``).

        A header that failed (status not OK) or is mixed (blobs of both
        types) is not added and is left to the caller, by its record.
        Consecutive added headers form a run, added with one device add per
        type; the parse has numbered a mixed header as a pack of its first
        blob's type, so the pack numbers of the runs after it are shifted
        down, as ``extend_json`` shifts them up for the files of the host.
        So pack numbers, entry numbers and sizes are those of ``extend``
        over the added packs in order."""
        from .headers import OK, parse_headers
        pack_ids = [bytes(i) for i in pack_ids]
        if len(pack_ids) != len(lens):
            raise RusticError(ErrorKind.InvalidInput, "one pack id per header")
        base = {t: len(self._t[t].packs) for t in (DATA, TREE)}  # what the parse counts from
        with self._stage("parse"):
            res = parse_headers(d_plain, offs, lens, (base[DATA], base[TREE]), device=self.device,
                                want_ids=(self._t[DATA].mode != "none", True),
                                want_locs=(self._t[DATA].mode == "full", True))
        h = res.headers
        good = (h["status"] == OK) & ~((h["data"] != 0) & (h["tree"] != 0))
        skipped = {DATA: 0, TREE: 0}  # mixed headers the parse has numbered so far
        i, n = 0, len(h)
        while i < n:
            if not good[i]:
                if h["status"][i] == OK:
                    skipped[int(h["type"][i])] += 1
                i += 1
                continue
            j = i
            while j < n and good[j]:
                j += 1
            run = h[i:j]
            for k in range(i, j):
                t = self._t[int(h["type"][k])]
                t.packs.append(pack_ids[k])
                t.total_size += int(h["pack_size"][k])
            for tpe in (DATA, TREE):
                t = self._t[tpe]
                sel = run[run["type"] == tpe]
                ne = int(sel["count"].sum())
                if not ne or t.mode == "none":
                    continue
                a = int(sel["first"][0])  # a type's entries follow each other in header order
                locs = None
                if t.mode == "full":
                    locs = res.locs[tpe][a:a + ne]
                    if skipped[tpe]:
                        locs[:, 0] -= skipped[tpe]
                with self._stage("add"):
                    self._add(t, res.ids[tpe][a:a + ne], locs, DEVICE_PTRS)
            i = j
        return h.copy()

    def load(self, key, sealed_files) -> np.ndarray:
        """``decrypt_file`` (backend/decrypt.rs:421-439) for a batch of
        sealed index files (bytes each), then ``extend_json``: the sealed
        bytes are uploaded once and opened on the device; a file that starts
        with ``{`` or ``[`` is its own text, one that starts with ``2`` is a
        zstd frame and is decoded on the device, anything else is
        ErrorKind.Unsupported.  Only the first bytes of each opened file go
        to the host.  Returns ``extend_json``'s statuses."""
        from .compress import DEC_CORRUPT, DEC_FULL, DECODE_MESSAGE, decompress_frames
        from .crypto import _ctx, make_refs as aead_refs
        from .read import MAC_MESSAGE, SHORT_MESSAGE
        torch, dev = self._torch()
        sealed = [bytes(s) for s in sealed_files]
        n = len(sealed)
        if not n:
            return np.zeros(0, np.uint32)
        if min(len(s) for s in sealed) < 16:
            raise RusticError(ErrorKind.Cryptography, SHORT_MESSAGE)
        s_lens = np.array([len(s) for s in sealed], np.int64)
        s_offs = _layout(s_lens)
        host = np.zeros(int(s_offs[-1]) + _pad16(int(s_lens[-1])) + 16, np.uint8)
        for o, s in zip(s_offs, sealed):
            host[int(o):int(o) + len(s)] = np.frombuffer(s, np.uint8)
        p_lens = np.maximum(s_lens - 32, 0)
        p_offs = _layout(p_lens + HEAD)  # every file has HEAD readable bytes
        with torch.cuda.device(dev):
            stream = self._stream(torch, dev)
            ctx = _ctx(self.device)
            d_sealed = torch.from_numpy(host).to(dev)
            plain = torch.zeros(int(p_offs[-1]) + _pad16(int(p_lens[-1]) + HEAD) + 16,
                                dtype=torch.uint8, device=dev)
            with self._stage("open"):
                st = key.open_blobs(d_sealed.data_ptr(), aead_refs(s_offs, s_lens, p_offs),
                                    plain.data_ptr(), stream, ctx)
            if st.any():
                raise RusticError(ErrorKind.Cryptography, MAC_MESSAGE)
            idx = torch.from_numpy(p_offs.astype(np.int64)).to(dev)[:, None] + \
                torch.arange(HEAD, device=dev)[None, :]
            heads = plain[idx].cpu().numpy()
            offs, lens = p_offs.astype(np.int64), p_lens.copy()
            frames = []
            for i in range(n):
                first = int(heads[i, 0]) if p_lens[i] else -1
                if first in (0x7B, 0x5B):
                    continue
                if first != 2:
                    raise RusticError(ErrorKind.Unsupported, UNSUPPORTED_MESSAGE)
                frames.append(i)
            if not frames:
                return self.extend_json(plain, offs, lens)
            # capacity: the frame's content size where its header has one,
            # else a guess that doubles while the decoder reports "full"
            caps = {}
            for i in frames:
                cs = _frame_content_size(heads[i, 1:min(HEAD, int(p_lens[i]))].tobytes())
                if cs is _BAD:
                    raise RusticError(ErrorKind.Internal, DECODE_MESSAGE)
                caps[i] = (int(cs), True) if cs is not None else (8 * int(p_lens[i]) + (128 << 10), False)
            text = None
            todo = list(frames)
            while todo:
                c = np.array([caps[i][0] for i in todo], np.int64)
                o_offs = _layout(c)
                out = torch.empty(int(o_offs[-1]) + _pad16(int(c[-1])) + 16, dtype=torch.uint8,
                                  device=dev)
                with self._stage("decode"):
                    dst, dln = decompress_frames(ctx, plain.data_ptr(),
                                                 [int(p_offs[i]) + 1 for i in todo],
                                                 [int(p_lens[i]) - 1 for i in todo],
                                                 out.data_ptr(), o_offs, c, stream)
                if (dst == DEC_CORRUPT).any():
                    raise RusticError(ErrorKind.Internal, DECODE_MESSAGE)
                again = []
                base = 0 if text is None else int(text.numel())
                for k, i in enumerate(todo):
                    if int(dst[k]) == DEC_FULL:
                        if caps[i][1] or caps[i][0] > 1 << 32:
                            raise RusticError(ErrorKind.Internal, DECODE_MESSAGE)
                        caps[i] = (2 * caps[i][0], False)
                        again.append(i)
                    else:
                        offs[i], lens[i] = base + int(o_offs[k]), int(dln[k])
                text = out if text is None else torch.cat([text, out])
                todo = again
            # one arena: the decoded texts, then the files that were text already
            tb = int(text.numel())
            for i in range(n):
                if i not in caps:
                    offs[i] += tb
            return self.extend_json(torch.cat([text, plain]), offs, lens)

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
