"""Pack headers read in bulk (rcdc_pack_header_parse in include/rcdc.h) and
what the reference does by reading them: ``repair index`` and the checked
index of ``check`` / ``prune``.

Reference:
- ``repofile/packfile.rs:88-242``: ``PackHeader::from_binary`` --
  ``pack.parse_header`` is that rule on the host, for one header, and stays
  the contract of ``parse_headers``;
- ``packfile.rs:259-330``: ``PackHeader::from_file`` (``read_headers``, for a
  batch of packs: one upload, one ``Key.open_blobs``, one ``parse_headers``);
- ``commands/repair/index.rs:40-113``: ``repair_index``; ``:115-179``:
  ``PackChecker``; ``:181-225``: ``index_checked_from_collector``
  (``index_checked``).

The device path keeps entries and ids in HBM from the opened header to the
written index file (``index_write.DeviceIndexer``) or to the device index
(``DeviceIndex.extend_headers``).  ``device=None`` is the same rule on the
host, one header at a time, and what the device path is tested against.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .dindex import DATA, TREE, DeviceIndex, IndexType, _layout, _pad16
from .errors import ErrorKind, RusticError, status_error
from .index import IndexFile, IndexPack, Indexer
from .pack import header_size, parse_header

OK, BAD_TYPE, CUT_SHORT, OVERFLOW = 0, 1, 2, 3  # RCDC_PKHDR_*
# rcdc_pkhdr_ref / rcdc_pkhdr_header as numpy records
PK_REF = np.dtype([("off", "<u8"), ("len", "<u8")])
PK_HEADER = np.dtype([("status", "<u4"), ("type", "<u4"), ("number", "<u4"), ("count", "<u4"),
                      ("first", "<u8"), ("data", "<u4"), ("tree", "<u4"), ("size", "<u8"),
                      ("pack_size", "<u8"), ("err_pos", "<u8"), ("err_entry", "<u4"),
                      ("pad", "<u4")])
assert PK_HEADER.itemsize == 64

LENGTH_LEN = 4      # constants::LENGTH_LEN: the u32 at a pack's end
COMP_OVERHEAD = 32  # constants::COMP_OVERHEAD: nonce and tag of the sealed header
# packfile.rs:259-330
LENGTH_MESSAGE = "Reading pack header length failed"
TOO_LARGE_MESSAGE = "Read header length `{size_real}` + `{length}` is larger than `{pack_size}`!"
READ_MESSAGE = "Reading pack header failed."
CONTENTS_MESSAGE = "Read header length doesn't match header contents!"
PACK_SIZE_MESSAGE = ("pack size `{size_computed}` computed from header doesn't match real pack "
                     "file size `{size_real}`!")
# the reference's `offset += length` is a u32 add: it has no message of its own
OVERFLOW_MESSAGE = "Reading pack header failed: the blob offsets exceed 2^32 - 1."


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


def parse_tile() -> int:
    """The tile size of the device's passes (RCDC_PKHDR_TILE)."""
    return int(_lib.lib().rcdc_pack_header_parse_tile())


def parse_bound(length: int) -> int:
    """Entries that ``length`` bytes of pack header hold at most."""
    return int(_lib.lib().rcdc_pack_header_parse_bound(int(length)))


class ParsedHeaders:
    """rcdc_pack_header_parse's outputs: ``ids[t]`` (cap, 32) uint8 and
    ``locs[t]`` (cap, 4) int32 device tensors (None where not asked for) of
    which the first ``entries[t]`` rows are written; ``headers`` (PK_HEADER,
    one per header) on the host; ``packs[t]``: the OK headers of type t."""

    def __init__(self, ids, locs, headers, entries, packs, raw):
        self.ids, self.locs, self.headers, self.entries, self.packs = ids, locs, headers, entries, packs
        self.raw = raw  # the flat allocations behind ids / locs, guard bytes included

    def columns(self, t: int):
        """(ids, offsets, lens, ulens) of type t's entries, the last three as
        strided views of ``locs[t]``: the entry arrays of
        ``index_write.write_json`` / ``DeviceIndexer``.  The same objects at
        every call."""
        if not hasattr(self, "_columns"):
            self._columns = {}
        if t not in self._columns:
            n = self.entries[t]
            ids, locs = self.ids[t][:n], self.locs[t][:n]
            self._columns[t] = (ids, locs[:, 1], locs[:, 2], locs[:, 3])
        return self._columns[t]


def parse_headers(d_plain, offs, lens, pack_base=(0, 0), device: int = 0, want_ids=(True, True),
                  want_locs=(True, True), guard: int = 0) -> ParsedHeaders:
    """The opened pack headers ``d_plain[offs[i] : offs[i] + lens[i]]`` (a
    uint8 device tensor) parsed on the device, pack numbers counted from
    ``pack_base`` per type.  ``guard``: that many bytes of 0xA5 behind every
    output array (in ``raw``), for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    n = len(lens)
    if len(offs) != n:
        raise RusticError(ErrorKind.InvalidInput, "one offset per length")
    if not (hasattr(d_plain, "data_ptr") and str(d_plain.dtype) == "torch.uint8"
            and d_plain.dim() == 1 and d_plain.is_contiguous() and d_plain.device == dev):
        raise RusticError(ErrorKind.InvalidInput,
                          f"d_plain must be a contiguous uint8 tensor on {dev}")
    refs = np.zeros(n, PK_REF)
    refs["off"], refs["len"] = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
    cap = int((refs["len"] // np.uint64(37)).sum())  # rcdc_pack_header_parse_bound, summed
    headers = np.zeros(n, PK_HEADER)
    result = _lib.PkhdrResult()
    base = (ctypes.c_uint32 * 2)(int(pack_base[0]), int(pack_base[1]))
    ids, locs, raw = [None, None], [None, None], []
    with torch.cuda.device(dev):
        for t in (DATA, TREE):
            for arr, want, width in ((ids, want_ids[t], 32), (locs, want_locs[t], 16)):
                if not want:
                    continue
                flat = torch.full((cap * width + guard,), 0xA5, dtype=torch.uint8, device=dev) \
                    if guard else torch.empty(cap * width, dtype=torch.uint8, device=dev)
                raw.append(flat)
                body = flat[:cap * width]
                arr[t] = body.view(cap, 32) if width == 32 else body.view(torch.int32).view(cap, 4)
        pi = (ctypes.c_void_p * 2)(*[None if a is None else a.data_ptr() for a in ids])
        pl = (ctypes.c_void_p * 2)(*[None if a is None else a.data_ptr() for a in locs])
        _check(_lib.lib().rcdc_pack_header_parse(
            _ctx(int(device)).handle, d_plain.data_ptr() if d_plain.numel() else None,
            int(d_plain.numel()), refs.ctypes.data, n, base, pi, pl, cap, headers.ctypes.data,
            ctypes.byref(result), int(torch.cuda.current_stream(dev).cuda_stream)))
    return ParsedHeaders(ids, locs, headers, (int(result.entries[0]), int(result.entries[1])),
                         (int(result.packs[0]), int(result.packs[1])), raw)


# ---- PackHeader::from_file for a batch ---------------------------------------------

class HeaderResult(NamedTuple):
    """A pack's header as read.  On the device path its entries are the rows
    [first, first + count) of ``parsed.columns(type)`` and ``index_pack`` is
    None -- unless the header is mixed (blobs of both types), then it went
    through ``pack.parse_header`` on the host and ``index_pack`` holds it.
    With ``device=None`` there is only ``index_pack``."""
    id: bytes
    type: int
    first: int
    count: int
    data: int
    tree: int
    pack_size: int
    parsed: Optional[ParsedHeaders] = None
    index_pack: Optional[IndexPack] = None

    @property
    def mixed(self) -> bool:
        return self.data != 0 and self.tree != 0


def _host_bytes(got) -> bytes:
    if hasattr(got, "data_ptr"):
        return got.cpu().numpy().tobytes()
    return bytes(got)


def _internal(message: str, **context) -> RusticError:
    return RusticError(ErrorKind.Internal, message.format(**context))


def _read_sealed(pack_id: bytes, size_hint: Optional[int], pack_size: int,
                 read_partial: Callable) -> Union[bytes, RusticError]:
    """from_file up to the sealed header (packfile.rs:265-305).  A guess
    that does not fit the pack is cut down to it (the reference's
    ``pack_size - read_size`` would wrap)."""
    guess = min(int(size_hint or 0), max(int(pack_size) - LENGTH_LEN, 0))
    read_size = guess + LENGTH_LEN
    if read_size > pack_size:
        return _internal(LENGTH_MESSAGE)
    data = _host_bytes(read_partial(pack_id, pack_size - read_size, read_size))
    if len(data) != read_size:
        return RusticError(ErrorKind.InputOutput,
                           f"read_partial returned {len(data)} of {read_size} bytes of pack "
                           f"`{pack_id.hex()}`")
    size_real = int.from_bytes(data[guess:], "little")
    if size_real + LENGTH_LEN > pack_size:
        return _internal(TOO_LARGE_MESSAGE, size_real=size_real, length=LENGTH_LEN,
                         pack_size=pack_size)
    if size_real <= guess:  # the header was already read
        return data[guess - size_real:guess]
    # the guess was too small: read again
    sealed = _host_bytes(read_partial(pack_id, pack_size - size_real - LENGTH_LEN, size_real))
    if len(sealed) != size_real:
        return RusticError(ErrorKind.InputOutput,
                           f"read_partial returned {len(sealed)} of {size_real} bytes of pack "
                           f"`{pack_id.hex()}`")
    return sealed


def _host_header(pack_id: bytes, plain: bytes, pack_size: int) -> Union[HeaderResult, RusticError]:
    """from_file behind the decrypt (packfile.rs:307-329) on the host."""
    try:
        blobs = parse_header(plain)
    except RusticError as e:
        cut = "cut short" in str(e)  # parse_header's two errors
        return _internal(CONTENTS_MESSAGE if cut else READ_MESSAGE)
    if sum(b.length for b in blobs) > 0xFFFFFFFF:
        return _internal(OVERFLOW_MESSAGE)
    p = IndexPack(pack_id)
    for b in blobs:
        p.add(b.id, b.type, b.offset, b.length, b.uncompressed_len or None)
    computed = p.pack_size()
    if computed != pack_size:
        return _internal(PACK_SIZE_MESSAGE, size_computed=computed, size_real=pack_size)
    tree = sum(b.type for b in blobs)
    return HeaderResult(pack_id, blobs[0].type if blobs else DATA, 0, len(blobs),
                        len(blobs) - tree, tree, computed, None, p)


def _read_batch(packs, read_partial: Callable):
    """(one slot per pack: the error of its reads or None, [(pack, sealed header)])."""
    out: List[Union[HeaderResult, RusticError, None]] = []
    sealed: List[Tuple[int, bytes]] = []
    for k, (pid, hint, size) in enumerate(packs):
        got = _read_sealed(pid, hint, size, read_partial)
        if isinstance(got, RusticError):
            out.append(got)
        else:
            out.append(None)
            sealed.append((k, got))
    return out, sealed


def read_headers(key, packs: Sequence[Tuple[bytes, Optional[int], int]], read_partial: Callable,
                 device: Optional[int] = 0) -> List[Union[HeaderResult, RusticError]]:
    """``PackHeader::from_file`` (packfile.rs:259-330) for the batch ``packs``
    = [(pack id, size hint or None, pack size)], one result per pack in order.
    An error is returned in the pack's place, not raised: ``repair_index``
    drops such a pack with a warning, ``index_checked`` raises the first.

    Per pack, as there: ``read_partial(pack_id, offset, length)`` for the
    last ``size_hint + 4`` bytes; the u32 at the end is the sealed header's
    length, and where the guess was too small a second read fetches it.  All
    sealed headers then go into one arena that is uploaded once, opened in
    one ``Key.open_blobs`` call and parsed in one ``parse_headers`` call.
    After that: a MAC failure is ErrorKind.Cryptography; a type byte above 3
    "Reading pack header failed."; an entry cut short "Read header length
    doesn't match header contents!" (the reference's from_binary ends at such
    an entry as at the end, and ``size()`` then differs from the length read);
    ``pack_size()`` other than the pack's size the reference's message for
    that.  A mixed header (blobs of both types) is copied to the host and
    goes through ``pack.parse_header``; its result carries an ``IndexPack``.

    ``device=None``: ``key.decrypt_data`` and ``pack.parse_header`` per pack,
    the same results with an ``IndexPack`` each."""
    packs = [(bytes(i), h, int(s)) for i, h, s in packs]
    out, sealed = _read_batch(packs, read_partial)
    if device is None:
        for k, s in sealed:
            try:
                plain = key.decrypt_data(s)
            except RusticError as e:
                out[k] = e
                continue
            out[k] = _host_header(packs[k][0], plain, packs[k][2])
        return out
    op = _open_batch(key, out, sealed, int(device))
    if op is None:
        return out
    res = parse_headers(op.plain, op.offs, op.lens, device=int(device))
    for k, o, n, h in zip(op.packs, op.offs, op.lens, res.headers):
        pid, _, size = packs[k]
        err = _judge(h, size)
        if err is not None:
            out[k] = err
        elif h["data"] and h["tree"]:
            r = _host_header(pid, op.text(o, n), size)
            out[k] = r if isinstance(r, RusticError) else r._replace(
                first=int(h["first"]), parsed=res)
        else:
            out[k] = HeaderResult(pid, int(h["type"]), int(h["first"]), int(h["count"]),
                                  int(h["data"]), int(h["tree"]), int(h["pack_size"]), res)
    return out


def _judge(h, pack_size: int) -> Optional[RusticError]:
    """from_file's errors behind the decrypt, from a header's PK_HEADER record."""
    status = int(h["status"])
    if status == BAD_TYPE:
        return _internal(READ_MESSAGE)
    if status == CUT_SHORT:
        return _internal(CONTENTS_MESSAGE)
    if status == OVERFLOW:
        return _internal(OVERFLOW_MESSAGE)
    if int(h["pack_size"]) != pack_size:
        return _internal(PACK_SIZE_MESSAGE, size_computed=int(h["pack_size"]), size_real=pack_size)
    return None


class _Opened:
    """The opened headers of a batch in one device arena: header i is
    ``plain[offs[i] : offs[i] + lens[i]]`` and belongs to pack ``packs[i]`` of
    the batch."""

    def __init__(self, plain, offs, lens, packs):
        self.plain, self.offs, self.lens, self.packs = plain, offs, lens, packs

    def text(self, off: int, n: int) -> bytes:
        return self.plain[int(off):int(off) + int(n)].cpu().numpy().tobytes()


def _open_batch(key, out: list, sealed: List[Tuple[int, bytes]], device: int) -> Optional[_Opened]:
    """The sealed headers in one arena, uploaded once and opened in one
    ``Key.open_blobs`` call; a header that does not open gets its error in
    ``out``.  None when there is nothing to open."""
    from .read import MAC_MESSAGE, SHORT_MESSAGE
    if not sealed:
        return None
    import torch
    from .crypto import _ctx, make_refs as aead_refs
    dev = torch.device("cuda", device)
    s_lens = np.array([len(s) for _, s in sealed], np.int64)
    s_offs = _layout(s_lens)
    host = np.zeros(int(s_offs[-1]) + _pad16(int(s_lens[-1])) + 16, np.uint8)
    for o, (_, s) in zip(s_offs, sealed):
        host[int(o):int(o) + len(s)] = np.frombuffer(s, np.uint8)
    p_lens = np.maximum(s_lens - 32, 0)
    p_offs = _layout(p_lens)
    with torch.cuda.device(dev):
        stream = int(torch.cuda.current_stream(dev).cuda_stream)
        d_sealed = torch.from_numpy(host).to(dev)
        plain = torch.zeros(int(p_offs[-1]) + _pad16(int(p_lens[-1])) + 16, dtype=torch.uint8,
                            device=dev)
        st = key.open_blobs(d_sealed.data_ptr(), aead_refs(s_offs, s_lens, p_offs),
                            plain.data_ptr(), stream, _ctx(device))
    opened = [j for j in range(len(sealed)) if st[j] == 0]
    for j, (k, _) in enumerate(sealed):
        if st[j] != 0:
            out[k] = RusticError(ErrorKind.Cryptography,
                                 SHORT_MESSAGE if st[j] == 2 else MAC_MESSAGE)
    return _Opened(plain, p_offs[opened].astype(np.int64), p_lens[opened].astype(np.int64),
                   [sealed[j][0] for j in opened])


# ---- repair index ---------------------------------------------------------------------------

class PackChecker:
    """repair/index.rs:115-179 over the listed packs ``{pack id: size}``.
    ``dropped``: the packs ``check_pack`` took out of an index file because
    they are not listed, or were indexed before."""

    def __init__(self, listed_packs: Dict[bytes, int]):
        self.packs = {bytes(i): int(s) for i, s in dict(listed_packs).items()}
        self.packs_to_read: List[Tuple[bytes, Optional[int], int]] = []
        self.dropped: List[bytes] = []

    def check_pack(self, index_file: IndexFile, read_all: bool = False) -> Tuple[IndexFile, bool]:
        new_index, changed = IndexFile(), False
        for to_delete, part in ((False, index_file.packs), (True, index_file.packs_to_delete)):
            for p in part:
                index_size = p.pack_size()
                size = self.packs.pop(bytes(p.id), None)
                if size is None:
                    # not there, or indexed in another index file already: out of the index
                    self.dropped.append(bytes(p.id))
                    changed = True
                elif index_size != size or read_all:
                    self.packs_to_read.append((bytes(p.id), header_size(p.blobs) + COMP_OVERHEAD,
                                               size))
                    changed = True
                else:
                    new_index.add(p, to_delete)
        return new_index, changed

    def into_pack_to_read(self) -> List[Tuple[bytes, Optional[int], int]]:
        """The packs to read, then those listed but in no index file."""
        rest = [(i, None, s) for i, s in self.packs.items()]
        self.packs = {}
        return self.packs_to_read + rest


class RepairReport(NamedTuple):
    modified: List[bytes]                      # index files changed (removed unless dry_run)
    dropped: List[bytes]                       # packs taken out of the index
    read: List[bytes]                          # packs whose header was read
    failed: List[Tuple[bytes, RusticError]]    # packs whose header could not be read
    saved: List[bytes]                         # ids of the index files saved


def repair_index(key, index_files: Iterable[Tuple[bytes, IndexFile]],
                 listed_packs: Dict[bytes, int], read_partial: Callable, save: Callable,
                 remove: Callable, read_all: bool = False, dry_run: bool = False,
                 device: Optional[int] = 0, version: int = 2, level: int = 0) -> RepairReport:
    """``repair index`` (commands/repair/index.rs:40-113).

    ``index_files``: (index id, IndexFile) of every index file;
    ``listed_packs``: {pack id: size} as the backend lists them.  Every index
    file goes through ``PackChecker.check_pack``; a changed one is saved
    again without the packs taken out (unless nothing is left) and then
    ``remove(index_id)``d.  The headers of the packs to read are read in one
    ``read_headers`` batch; a pack whose header fails is reported (a warning,
    and ``failed``) and stays out of the index; every other one goes, without
    delete mark, time or size, to one ``index_write.DeviceIndexer`` as a
    ``PackRecord`` over the parser's arrays, so no entry passes the host.
    ``dry_run`` saves and removes nothing.

    ``save(ids, sealed, offs, lens)`` is the backend write of
    ``DeviceIndexer``: file i has the id ``ids[i]`` and the bytes
    ``sealed[offs[i] : offs[i] + lens[i]]`` (a uint8 device tensor).

    A difference from the reference: a mixed pack (blobs of both types in one
    header) reaches ``DeviceIndexer.add`` as an ``IndexPack`` and gets that
    class's ErrorKind.InvalidInput, where the reference writes it as it is.

    ``device=None``: the same rule with ``index.Indexer`` on the host;
    ``save(index_file)`` then takes an ``IndexFile`` and returns its id."""
    checker = PackChecker(listed_packs)
    modified: List[bytes] = []
    saved: List[bytes] = []
    for index_id, index_file in index_files:
        new_index, changed = checker.check_pack(index_file, read_all)
        if not changed:
            continue
        modified.append(bytes(index_id))
        if dry_run:
            continue
        if new_index.packs or new_index.packs_to_delete:
            saved.append(_save_host_file(key, new_index, save, device, version, level))
        remove(bytes(index_id))
    to_read = checker.into_pack_to_read()
    results = read_headers(key, to_read, read_partial, device)
    if device is None:
        indexer = Indexer(save)
    else:
        from .index_write import DeviceIndexer, PackRecord
        indexer = DeviceIndexer(save, device=int(device), key=key, version=version, level=level)
    read: List[bytes] = []
    failed: List[Tuple[bytes, RusticError]] = []
    for (pid, _, _), r in zip(to_read, results):
        if isinstance(r, RusticError):
            warnings.warn(f"error reading pack {pid.hex()} (-> removing from index): {r}")
            failed.append((pid, r))
            continue
        read.append(pid)
        if dry_run:
            continue
        if r.index_pack is not None:
            indexer.add(IndexPack(pid, list(r.index_pack.blobs)))
        else:
            indexer.add(PackRecord(pid, r.type, r.first, r.count), entries=r.parsed.columns(r.type))
    if not dry_run:
        indexer.finalize()
    return RepairReport(modified, checker.dropped, read, failed, saved + list(indexer.saved))


def _save_host_file(key, index_file: IndexFile, save: Callable, device: Optional[int],
                    version: int, level: int) -> bytes:
    """``be.save_file`` of a host IndexFile through the caller's ``save``."""
    if device is None:
        return bytes(save(index_file))
    import torch
    from .index import save_index_file
    id_, sealed = save_index_file(key, index_file, version, level, device=int(device))
    dev = torch.device("cuda", int(device))
    data = torch.frombuffer(bytearray(sealed), dtype=torch.uint8).to(dev)
    save([id_], data, np.zeros(1, np.int64), np.array([len(sealed)], np.int64))
    return id_


def index_checked(key, index_files: Iterable[IndexFile], listed_packs: Dict[bytes, int],
                  read_partial: Callable, device: int = 0,
                  index_type: IndexType = IndexType.FULL) -> DeviceIndex:
    """``index_checked_from_collector`` (repair/index.rs:181-225): the index
    ``check`` and ``prune`` open a repository with when its index files may be
    wrong.  The packs an index file has right (listed, with the listed size)
    are ``extend``ed from it; the headers of the others, and of the packs
    listed but in no index file, are read (``read_headers``) and
    ``extend_headers``ed on the device.  The first header error is raised."""
    checker = PackChecker(listed_packs)
    dx = DeviceIndex(int(device), index_type)
    for f in index_files:
        dx.extend(checker.check_pack(f, False)[0].packs)
    to_read = checker.into_pack_to_read()
    out, sealed = _read_batch(to_read, read_partial)
    op = _open_batch(key, out, sealed, int(device))
    mixed: List[IndexPack] = []
    if op is not None:
        recs = dx.extend_headers(op.plain, op.offs, op.lens, [to_read[k][0] for k in op.packs])
        for k, o, n, h in zip(op.packs, op.offs, op.lens, recs):
            pid, _, size = to_read[k]
            out[k] = _judge(h, size)
            if out[k] is None and h["data"] and h["tree"]:
                r = _host_header(pid, op.text(o, n), size)
                if isinstance(r, RusticError):
                    out[k] = r
                else:
                    mixed.append(r.index_pack)
    for e in out:
        if e is not None:
            dx.close()
            raise e
    dx.extend(mixed)
    return dx
