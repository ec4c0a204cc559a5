"""The ``check`` command: the index pass, the trees and the pack reads, in
batches on the device (rcdc_check_packs in include/rcdc.h, and the batched
calls the read path already has).

Reference: ``commands/check.rs`` --
- ``:40-181``  ``ReadSubsetOption`` and ``parse_n_m`` (``ReadSubset``);
- ``:225-321`` ``check_repository`` without the cache and hot-file passes;
- ``:456-615`` ``check_packs``, ``check_packs_list``, ``check_packs_list_hot``;
- ``:627-700`` ``check_trees`` over ``TreeStreamerOnce``;
- ``:718-814`` ``check_pack`` (``read.check_pack`` for one pack,
  ``check_pack_batch`` for many).

``device=None`` is the same rule in plain Python everywhere, as in
``headers.py`` and ``tree.py``: it needs only ``key.decrypt_data`` and a
``decode`` callable (frame -> bytes), and is what the device path is tested
against.  A finding is ``(level, read.Finding)`` with level ``"Error"`` or
``"Warn"``; ids in a finding's fields are bytes, blob types 0 (data) / 1
(tree), a ``source`` is the ``RusticError``.
"""
from __future__ import annotations

import calendar
import ctypes
import datetime
import hashlib
import json
import random
import re
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import ErrorKind, RusticError, status_error
from .index import IndexBlob, IndexFile, IndexPack
from .read import Finding, MAC_MESSAGE, SHORT_MESSAGE, _ulen

ERROR, WARN = "Error", "Warn"  # CheckErrorLevel
DATA, TREE = 0, 1
OK, HOST = 0, 1                            # RCDC_CKPACK_OK / _HOST
NOT_COMPARED, EQUAL, DIFFERS = 0, 1, 2     # header verdicts
KIND_TYPE, KIND_OFFSET = 0, 1              # finding kinds
NO_HEADER = 0xFFFFFFFF
DEFAULT_BUDGET = 1 << 30
# rcdc_prune_range / rcdc_ckpack_hdr / rcdc_ckpack_pack / rcdc_ckpack_finding as numpy records
CK_RANGE = np.dtype([("first", "<u8"), ("count", "<u4"), ("pad", "<u4")])
CK_HDR = np.dtype([("type", "<u4"), ("count", "<u4"), ("first", "<u8")])
CK_PACK = np.dtype([("status", "<u4"), ("type", "<u4"), ("type_findings", "<u4"),
                    ("offset_findings", "<u4"), ("end_offset", "<u4"), ("header_verdict", "<u4"),
                    ("header_diff", "<u4"), ("sorted", "<u4"), ("header_len", "<u8"),
                    ("first_finding", "<u8")])
CK_FINDING = np.dtype([("pack", "<u4"), ("entry", "<u4"), ("kind", "<u4"), ("got", "<u4"),
                       ("expected", "<u4")])
assert CK_PACK.itemsize == 48 and CK_FINDING.itemsize == 20 and CK_HDR.itemsize == 16

Result = Tuple[str, Finding]


def _check(st: int) -> None:
    if st != 0:
        raise status_error(st, _lib.last_error())


def sort_max() -> int:
    """Entries of a pack out of order that the device still sorts
    (RCDC_CKPACK_SORT_MAX)."""
    return int(_lib.lib().rcdc_check_packs_sort_max())


# ---- ReadSubsetOption (check.rs:40-181) -------------------------------------------

_UNITS = {"": 1, "b": 1}
for _i, _p in enumerate("kmgtpe", 1):
    _UNITS[_p] = _UNITS[_p + "b"] = 1000 ** _i
    _UNITS[_p + "i"] = _UNITS[_p + "ib"] = 1024 ** _i


def _u32(s: str) -> int:
    """``str::parse::<u32>``."""
    if not re.fullmatch(r"\+?[0-9]+", s) or int(s) > 0xFFFFFFFF:
        raise ValueError(f"invalid u32 `{s}`")
    return int(s)


def parse_n_m(now: datetime.datetime, n_in: str, m_in: str) -> Tuple[int, int]:
    """check.rs:107-130: ``n/m`` with the named settings, which depend on the
    date ``now``.  Returns (n % m, m); what is no number raises ValueError."""
    yday = now.timetuple().tm_yday
    in_month = calendar.monthrange(now.year, now.month)[1]
    in_year = 366 if calendar.isleap(now.year) else 365
    named = {"hourly": (yday - 1) * 24 + now.hour, "daily": yday - 1,
             "weekly": now.isocalendar()[1] - 1, "monthly": now.month - 1}
    n = named[n_in] if n_in in named else _u32(n_in)
    pairs = {("hourly", "day"): 24, ("hourly", "week"): 24 * 7, ("hourly", "month"): 24 * in_month,
             ("hourly", "year"): 24 * in_year, ("daily", "week"): 7, ("daily", "month"): in_month,
             ("daily", "year"): in_year, ("weekly", "month"): 4, ("weekly", "year"): 52,
             ("monthly", "year"): 12}
    suffixed = {"month_hours": 24 * in_month, "year_hours": 24 * in_year, "month_days": in_month,
                "year_days": in_year}
    if (n_in, m_in) in pairs:
        m = pairs[(n_in, m_in)]
    elif m_in in suffixed:
        m = suffixed[m_in]
    else:
        m = _u32(m_in)
    if m == 0:
        raise ValueError("m is 0")  # the reference's n % m panics
    return n % m, m


class ReadSubset(NamedTuple):
    """ReadSubsetOption: ``kind`` is "All", "Percentage" (value: float),
    "Size" (value: bytes) or "IdSubSet" (value: (n, m))."""
    kind: str = "All"
    value: object = None

    @classmethod
    def parse(cls, s: str, now: Optional[datetime.datetime] = None) -> "ReadSubset":
        """FromStr (check.rs:132-181): ``all``, ``x%``, ``n/m`` or a size."""
        if s == "all":
            return cls("All")
        if s.endswith("%"):
            try:
                return cls("Percentage", float(s[:-1]))
            except ValueError as e:
                raise RusticError(ErrorKind.InvalidInput,
                                  f"Error parsing percentage from value `{s[:-1]}` for ReadSubset "
                                  "option. Did you forget the '%'?") from e
        if "/" in s:
            n, m = s.split("/", 1)
            try:
                return cls("IdSubSet", parse_n_m(now or datetime.datetime.now().astimezone(), n, m))
            except ValueError as e:
                raise RusticError(ErrorKind.InvalidInput,
                                  f"Error parsing 'n/m' from value `{s}` for ReadSubset option. "
                                  "Allowed values: 'all', 'x%', 'n/m' or a size.") from e
        mt = re.fullmatch(r"\s*([0-9]+(?:\.[0-9]*)?|\.[0-9]+)\s*([A-Za-z]*)\s*", s)
        if not mt or mt.group(2).lower() not in _UNITS:
            raise RusticError(ErrorKind.InvalidInput,
                              f"Error parsing size from value `{s}` for ReadSubset option. "
                              "Allowed values: 'all', 'x%', 'n/m' or a size.")
        return cls("Size", int(float(mt.group(1)) * _UNITS[mt.group(2).lower()]))

    def apply(self, packs: Iterable[IndexPack], rng: Optional[random.Random] = None
              ) -> List[IndexPack]:
        """apply_with_rng (check.rs:60-102).  ``rng``: the shuffle's
        ``random.Random`` (a fresh one when None); the reference's StdRng
        sequence is not reproduced, so which packs a random subset holds
        differs from there, and its size rule does not."""
        packs = list(packs)
        total = sum(int(p.pack_size()) for p in packs)
        if self.kind == "All":
            return packs
        if self.kind == "IdSubSet":
            n, m = self.value
            # Id::as_u32: the little-endian u32 of id bytes 0..4
            return [p for p in packs if int.from_bytes(bytes(p.id)[:4], "little") % m == n % m]
        if self.kind == "Percentage":
            f = total * float(self.value) / 100.0
            top = (1 << 64) - 1  # `as u64` saturates, and NaN gives 0
            size = 0 if f != f or f < 0 else top if f >= float(top) else int(f)
        else:
            size = int(self.value)
        (rng or random.Random()).shuffle(packs)
        out = []
        for p in packs:
            p_size = int(p.pack_size())
            if size > p_size:
                size -= p_size
                out.append(p)
        return out


# ---- the index pass (check.rs:484-507) ----------------------------------------------

def _blob_type(p: IndexPack) -> int:
    return int(p.blobs[0].type) if p.blobs else DATA


def _sorted_blobs(blobs: Sequence) -> list:
    """IndexBlob's order: by (offset, length, uncompressed length); equal
    locations keep their order (rcdc_check_packs' tie rule)."""
    return sorted(blobs, key=lambda b: (int(b.offset), int(b.length), _ulen(b)))


def _type_finding(pid, blob_id, got, expected) -> Result:
    return ERROR, Finding("PackBlobTypesMismatch",
                          dict(id=pid, blob_id=blob_id, blob_type=int(got), expected=int(expected)))


def _offset_finding(pid, blob_id, got, expected) -> Result:
    return ERROR, Finding("PackBlobOffsetMismatch",
                          dict(id=pid, blob_id=blob_id, offset=int(got), expected=int(expected)))


def index_pass_host(p: IndexPack) -> List[Result]:
    """check.rs:484-507 for one pack in plain Python.  ``expected`` wraps at
    2^32 as a release build's u32 add does."""
    pid, blob_type = bytes(p.id), _blob_type(p)
    out, expected = [], 0
    for b in _sorted_blobs(p.blobs):
        if int(b.type) != blob_type:
            out.append(_type_finding(pid, bytes(b.id), b.type, blob_type))
        if int(b.offset) != expected:
            out.append(_offset_finding(pid, bytes(b.id), b.offset, expected))
        expected = (expected + int(b.length)) & 0xFFFFFFFF
    return out


class CheckedPacks:
    """rcdc_check_packs' outputs: ``packs`` (CK_PACK, host), ``findings``
    (a (cap, 5) int32 device tensor of CK_FINDING rows of which the first
    min(total, cap) are written), ``total`` findings, ``order`` (n int32
    device tensor or None), the counters ``packs_host`` and
    ``packs_sorted_on_device``."""

    def __init__(self, packs, findings, total, order, packs_host, packs_sorted, raw):
        self.packs, self.findings, self.total, self.order = packs, findings, total, order
        self.packs_host, self.packs_sorted_on_device = packs_host, packs_sorted
        self.raw = raw  # the flat allocations behind findings / order, guard bytes included

    def findings_host(self) -> np.ndarray:
        n = min(self.total, int(self.findings.shape[0]))
        return self.findings[:n].cpu().numpy().view(np.uint32).reshape(n, 5).copy().view(CK_FINDING).ravel()


def _ptr_stride(t, width: int):
    """(address, stride in bytes) of a tensor of rows."""
    if t.dim() == 2 and (int(t.shape[1]) != width or (int(t.shape[0]) and t.stride(1) != 1)):
        raise RusticError(ErrorKind.InvalidInput, f"rows of {width} elements, densely stored")
    stride = int(t.stride(0)) * t.element_size() if int(t.shape[0]) > 1 else width * t.element_size()
    return t.data_ptr(), stride


def run_check_packs(ids, offs, lens, ulens, types, ranges, hdr=None, device: int = 0,
                    cap_findings: Optional[int] = None, want_order: bool = False,
                    guard: int = 0) -> CheckedPacks:
    """rcdc_check_packs over entry columns on the device: ``ids`` (n, 32)
    uint8, ``offs`` / ``lens`` / ``ulens`` n int32 each (strided views of an
    (n, 4) array of rcdc_dindex_loc records pass as they are, as
    ``ParsedHeaders.columns`` and ``ParsedJson`` give them), ``types`` n uint8
    or None, ``ranges`` [(first, count)] per pack (or a CK_RANGE array, which
    is passed as it is).  ``hdr``: (ParsedHeaders,
    CK_HDR records) for the header compare.  ``cap_findings`` None: as many
    as there are (a second call when the first guess was too small).
    ``guard``: that many 0xA5 bytes behind every device output, for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    n = int(ids.shape[0])
    if isinstance(ranges, np.ndarray) and ranges.dtype == CK_RANGE:
        rg = np.ascontiguousarray(ranges)  # as they are: nothing per pack in Python
    else:
        rg = np.zeros(len(ranges), CK_RANGE)
        if len(ranges):
            pairs = np.asarray(ranges, np.uint64).reshape(len(ranges), 2)
            rg["first"], rg["count"] = pairs[:, 0], pairs[:, 1]
    packs = np.zeros(len(rg), CK_PACK)
    result = _lib.CkpackResult()
    raw = []

    def alloc(nbytes):
        flat = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev) if guard \
            else torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        raw.append(flat)
        return flat[:nbytes]
    hi = hl = he = hr = None
    if hdr is not None:
        parsed, recs = hdr
        recs = np.ascontiguousarray(recs, CK_HDR)
        if len(recs) != len(rg):
            raise RusticError(ErrorKind.InvalidInput, "one header record per pack")
        hi = (ctypes.c_void_p * 2)(*[None if a is None else a.data_ptr() for a in parsed.ids])
        hl = (ctypes.c_void_p * 2)(*[None if a is None else a.data_ptr() for a in parsed.locs])
        he = (ctypes.c_uint64 * 2)(int(parsed.entries[0]), int(parsed.entries[1]))
        hr = recs.ctypes.data
    with torch.cuda.device(dev):
        stream = int(torch.cuda.current_stream(dev).cuda_stream)
        order = alloc(n * 4).view(torch.int32) if want_order else None
        pi, si = _ptr_stride(ids, 32)
        (po, so), (pl, sl), (pu, su) = (_ptr_stride(t, 1) for t in (offs, lens, ulens))
        cap = cap_findings
        if cap is None:
            cap = min(2 * int(rg["count"].sum()), 1 << 16)
        while True:
            fbuf = alloc(cap * 20)
            _check(_lib.lib().rcdc_check_packs(
                _ctx(int(device)).handle, pi if n else None, si, po if n else None, so,
                pl if n else None, sl, pu if n else None, su,
                None if types is None or not n else types.data_ptr(), n, rg.ctypes.data, len(rg),
                hi, hl, he, hr, packs.ctypes.data, fbuf.data_ptr() if cap else None, cap,
                None if order is None else order.data_ptr(), ctypes.byref(result), stream))
            if cap_findings is not None or int(result.findings) <= cap:
                break
            raw.pop()
            cap = int(result.findings)
    return CheckedPacks(packs, fbuf.view(torch.int32).view(cap, 5), int(result.findings), order,
                        int(result.packs_host), int(result.packs_sorted_on_device), raw)


def _flatten(packs: Sequence[IndexPack]):
    """(ids, locs, types, ranges) of the packs' blobs as numpy arrays."""
    n = sum(len(p.blobs) for p in packs)
    ids = np.zeros((n, 32), np.uint8)
    locs = np.zeros((n, 4), np.uint32)
    types = np.zeros(n, np.uint8)
    ranges, at = [], 0
    for k, p in enumerate(packs):
        c = len(p.blobs)
        if c:
            ids[at:at + c] = np.frombuffer(b"".join(bytes(b.id) for b in p.blobs),
                                           np.uint8).reshape(c, 32)
            locs[at:at + c] = [(k, int(b.offset), int(b.length), _ulen(b)) for b in p.blobs]
            types[at:at + c] = [int(b.type) for b in p.blobs]
        ranges.append((at, c))
        at += c
    return ids, locs, types, ranges


def _upload(torch, dev, ids, locs, types):
    d_ids = torch.from_numpy(ids).to(dev)
    d_locs = torch.from_numpy(locs.view(np.int32)).to(dev)
    d_types = torch.from_numpy(types).to(dev)
    return d_ids, d_locs, d_types


def _index_pass_device(packs: Sequence[IndexPack], device: int) -> List[List[Result]]:
    """index_pass_host for every pack, through one rcdc_check_packs call; a
    pack the kernel leaves to the host (status HOST) goes through the Python
    rule."""
    import torch
    dev = torch.device("cuda", int(device))
    ids, locs, types, ranges = _flatten(packs)
    d_ids, d_locs, d_types = _upload(torch, dev, ids, locs, types)
    res = run_check_packs(d_ids, d_locs[:, 1], d_locs[:, 2], d_locs[:, 3], d_types, ranges,
                          device=device)
    out: List[List[Result]] = [[] for _ in packs]
    for f in res.findings_host():
        k, e = int(f["pack"]), int(f["entry"])
        pid, bid = bytes(packs[k].id), ids[e].tobytes()
        make = _type_finding if int(f["kind"]) == KIND_TYPE else _offset_finding
        out[k].append(make(pid, bid, f["got"], f["expected"]))
    for k in np.nonzero(res.packs["status"] == HOST)[0]:
        out[int(k)] = index_pass_host(packs[int(k)])
    return out


def _packs_lists(findings: List[Result], packs: Dict[bytes, Tuple[int, bool]],
                 tree_packs: Dict[bytes, Tuple[int, bool]], listed_packs, hot_listed) -> None:
    """check_packs_list_hot (check.rs:579-615), then check_packs_list
    (:537-567); ``packs`` keeps the packs that are not listed."""
    if hot_listed is not None:
        tree_packs = dict(tree_packs)
        for id_, size in hot_listed:
            id_ = bytes(id_)
            got = tree_packs.pop(id_, None)
            if got is None:
                kind = "HotDataPack" if id_ in packs else "HotPackNotReferenced"
                findings.append((WARN, Finding(kind, dict(id=id_))))
            elif got[0] != int(size):
                findings.append((ERROR, Finding("HotPackSizeMismatchIndex",
                                                dict(id=id_, to_delete=got[1], index_size=got[0],
                                                     size=int(size)))))
        for id_ in sorted(tree_packs):
            size, to_delete = tree_packs[id_]
            findings.append((ERROR, Finding("NoHotPack", dict(id=id_, to_delete=to_delete,
                                                              size=size))))
    for id_, size in sorted((bytes(i), int(s)) for i, s in listed_packs):
        got = packs.pop(id_, None)
        if got is None:
            findings.append((WARN, Finding("PackNotReferenced", dict(id=id_))))
        elif got[0] != size:
            findings.append((ERROR, Finding("PackSizeMismatchIndex",
                                            dict(id=id_, to_delete=got[1], index_size=got[0],
                                                 size=size))))
    for id_ in sorted(packs):
        size, to_delete = packs[id_]
        findings.append((ERROR, Finding("NoPack", dict(id=id_, to_delete=to_delete, size=size))))


def check_packs(index_files: Iterable[IndexFile], listed_packs, hot_listed=None,
                device: Optional[int] = 0):
    """check_packs (check.rs:456-615).  ``index_files``: every index.IndexFile
    in the order they are read; ``listed_packs``: [(pack id, size)] as the
    backend lists them; ``hot_listed``: the same of the hot backend, or None
    when there is none.

    Per pack of every file (``packs``, then ``packs_to_delete``):
    PackTimeNotSet for a pack to delete without a time, then the index pass --
    one rcdc_check_packs call over the blobs of all packs, flattened with
    their type bytes; packs with status HOST go through ``index_pass_host``.
    Then ``check_packs_list_hot`` and ``check_packs_list``.

    Returns (findings, the collected IndexPacks -- ``packs`` only, as
    ``index_collector.extend(index.packs)`` -- and the map {pack id:
    (size, to_delete)} of the packs that are indexed and not listed)."""
    index_files = list(index_files)
    all_packs = [(p, d) for f in index_files for part, d in ((f.packs, False),
                                                             (f.packs_to_delete, True))
                 for p in part]
    collected = [p for f in index_files for p in f.packs]
    only = [p for p, _ in all_packs]
    per_pack = [index_pass_host(p) for p in only] if device is None \
        else _index_pass_device(only, int(device))
    findings: List[Result] = []
    packs: Dict[bytes, Tuple[int, bool]] = {}
    tree_packs: Dict[bytes, Tuple[int, bool]] = {}
    for (p, to_delete), found in zip(all_packs, per_pack):
        pid = bytes(p.id)
        packs[pid] = (int(p.pack_size()), to_delete)
        if hot_listed is not None and _blob_type(p) == TREE:
            tree_packs[pid] = packs[pid]
        if to_delete and p.time is None:
            findings.append((ERROR, Finding("PackTimeNotSet", dict(id=pid))))
        findings += found
    _packs_lists(findings, packs, tree_packs, listed_packs, hot_listed)
    return findings, collected, packs


class PackRecord(NamedTuple):
    """A pack whose entries are rows [first, first + count) of device arrays."""
    id: bytes
    first: int
    count: int
    to_delete: bool = False
    time_set: bool = True
    size: Optional[int] = None


def check_packs_entries(entries, records: Sequence[PackRecord], listed_packs, hot_listed=None,
                        device: int = 0):
    """``check_packs`` for entries that are on the device already: ``entries``
    = (ids, offsets, lengths, uncompressed lengths[, types]) as
    ``run_check_packs`` takes them -- ``headers.ParsedHeaders.columns(t)`` or
    the arrays of ``dindex.parse_json`` -- and ``records`` the packs over them.
    Nothing is flattened and only the findings' blob ids come to the host.

    What rcdc_index_parse's arrays cannot give this call: per-blob types (it
    files every blob under its pack's type, so without a types column there
    are no PackBlobTypesMismatch findings), ``packs_to_delete`` (it counts
    them and keeps none of their entries) and the packs' times, so
    PackTimeNotSet needs the caller's ``time_set``.  Returns (findings,
    {pack id: (size, to_delete)} of the packs not listed); the pack size is
    the record's, or header length + 4 + the end offset as a u32."""
    import torch
    ids, offs, lens, ulens = entries[:4]
    types = entries[4] if len(entries) > 4 else None
    res = run_check_packs(ids, offs, lens, ulens, types, [(r.first, r.count) for r in records],
                          device=device)
    per_pack: List[List[Result]] = [[] for _ in records]
    fh = res.findings_host()
    if len(fh):
        rows = torch.from_numpy(fh["entry"].astype(np.int64)).to(ids.device)
        bids = ids[rows].cpu().numpy()
        for f, bid in zip(fh, bids):
            k = int(f["pack"])
            make = _type_finding if int(f["kind"]) == KIND_TYPE else _offset_finding
            per_pack[k].append(make(bytes(records[k].id), bid.tobytes(), f["got"], f["expected"]))
    findings: List[Result] = []
    packs: Dict[bytes, Tuple[int, bool]] = {}
    tree_packs: Dict[bytes, Tuple[int, bool]] = {}
    for k, (r, rec) in enumerate(zip(records, res.packs)):
        pid = bytes(r.id)
        if int(rec["status"]) == HOST:
            sl = slice(r.first, r.first + r.count)
            cols = [t[sl].cpu().numpy() for t in (ids, offs, lens, ulens)]
            tp = types[sl].cpu().numpy() if types is not None else np.zeros(r.count, np.uint8)
            p = IndexPack(pid, [IndexBlob(cols[0][i].tobytes(), int(tp[i]), int(cols[1][i]) & 0xFFFFFFFF,
                                          int(cols[2][i]) & 0xFFFFFFFF,
                                          (int(cols[3][i]) & 0xFFFFFFFF) or None)
                                for i in range(r.count)])
            per_pack[k] = index_pass_host(p)
            size, tpe = p.pack_size() & 0xFFFFFFFF, _blob_type(p)
        else:
            size = (int(rec["header_len"]) + 4 + int(rec["end_offset"])) & 0xFFFFFFFF
            tpe = int(rec["type"])
        packs[pid] = (int(r.size) if r.size is not None else size, bool(r.to_delete))
        if hot_listed is not None and tpe == TREE:
            tree_packs[pid] = packs[pid]
        if r.to_delete and not r.time_set:
            findings.append((ERROR, Finding("PackTimeNotSet", dict(id=pid))))
        findings += per_pack[k]
    _packs_lists(findings, packs, tree_packs, listed_packs, hot_listed)
    return findings, packs


# ---- check_trees (check.rs:627-700) ---------------------------------------------------

class HostIndex:
    """IndexCollector's rule on the host (binarysorted.rs:127-163) for
    ``device=None``: every blob of a pack is filed under the type of the
    pack's first blob; the first entry of an id wins."""

    def __init__(self, packs: Iterable[IndexPack] = ()):
        self._t: Dict[int, Dict[bytes, Tuple[bytes, IndexBlob]]] = {DATA: {}, TREE: {}}
        self._packs: Dict[int, List[IndexPack]] = {DATA: [], TREE: []}
        self.extend(packs)

    def extend(self, packs: Iterable[IndexPack]) -> None:
        for p in packs:
            tpe = _blob_type(p)
            self._packs[tpe].append(p)
            for b in p.blobs:
                self._t[tpe].setdefault(bytes(b.id), (bytes(p.id), b))

    def get_id(self, tpe: int, id_: bytes) -> Optional[Tuple[bytes, IndexBlob]]:
        return self._t[tpe].get(bytes(id_))

    def into_packs(self) -> List[IndexPack]:
        return _collected_packs(self._packs[TREE], self._packs[DATA])


def _collected_packs(tree: Sequence[IndexPack], data: Sequence[IndexPack]) -> List[IndexPack]:
    """``index.into_index().into_iter()`` (binarysorted.rs:165-228): the tree
    packs, then the data packs, each with its id and blobs only -- no time,
    no size, and every blob under the pack's type."""
    return [IndexPack(bytes(p.id), [IndexBlob(bytes(b.id), tpe, int(b.offset), int(b.length),
                                              b.uncompressed_length) for b in p.blobs])
            for tpe, part in ((TREE, tree), (DATA, data)) for p in part]


_SIMPLE = {"a": 7, "b": 8, "f": 12, "n": 10, "r": 13, "t": 9, "v": 11, "\\": 92, "'": 39, '"': 34}


def node_name(name: str) -> str:
    """Node::name (backend/node.rs:352-354): the name with the escapes of
    Go's strconv.Quote undone (\\\\, \\xHH, \\uXXXX, \\UXXXXXXXX, octal and the
    letter escapes); a name that does not unescape is taken as it is.  Bytes
    that are no UTF-8 come back as surrogate escapes."""
    if "\\" not in name:
        return name
    out, i = bytearray(), 0
    try:
        while i < len(name):
            c = name[i]
            i += 1
            if c != "\\":
                out += c.encode("utf-8", "surrogateescape")
                continue
            c = name[i]
            i += 1
            if c in _SIMPLE:
                out.append(_SIMPLE[c])
            elif c == "x":
                out.append(int(name[i:i + 2], 16))
                i += 2
            elif c in "uU":
                w = 4 if c == "u" else 8
                if len(name) < i + w:
                    raise ValueError
                out += chr(int(name[i:i + w], 16)).encode("utf-8")
                i += w
            elif c in "01234567":
                out.append(int(name[i - 1:i + 2], 8) & 0xFF)
                i += 2
            else:
                raise ValueError
        return out.decode("utf-8", "surrogateescape")
    except (ValueError, IndexError):
        return name


def _join(path: str, name: str) -> str:
    """PathBuf::join for a node's name."""
    name = node_name(name)
    if name.startswith("/") or not path:
        return name
    return path + name if path.endswith("/") else path + "/" + name


def _decrypt_file(key, sealed: bytes, device, decode) -> bytes:
    """decrypt_file (backend/decrypt.rs:421-439)."""
    from .dindex import UNSUPPORTED_MESSAGE
    from .tree import _decode
    plain = key.decrypt_data(bytes(sealed))
    if plain[:1] in (b"{", b"["):
        return plain
    if plain[:1] == b"\x02":
        return _decode(plain[1:], device, decode)
    raise RusticError(ErrorKind.Unsupported, UNSUPPORTED_MESSAGE)


def _host_texts(key, index, frontier: List[bytes], read_partial, decode) -> List[bytes]:
    from .tree import _host_blob, _not_found
    for tid in frontier:
        if index.get_id(TREE, tid) is None:
            raise _not_found(tid)

    class _Dict:  # _host_blob asks a plain index with ``get``
        def get(self, tid):
            return index.get_id(TREE, tid)
    return [_host_blob(key, _Dict(), tid, read_partial, decode, None) for tid in frontier]


def _device_texts(key, index, frontier: List[bytes], read_partial, device: int, budget: int):
    """The decoded tree blobs of a level: one lookup, the pack reads of
    ``tree.find_used_blobs`` and one ``read.read_blobs`` per group."""
    import torch
    from .read import read_blobs
    from .restore import _groups
    from .tree import _level_reads, _load_group
    dev = torch.device("cuda", device)
    ids = np.frombuffer(b"".join(frontier), np.uint8).reshape(-1, 32).copy()
    hits = index.lookup(TREE, torch.from_numpy(ids).to(dev)).cpu().numpy().view(np.uint32)
    reads = _level_reads(index, ids, hits)  # raises for an id the index lacks
    texts: List[Optional[bytes]] = [None] * len(frontier)
    for group in _groups(reads, int(budget)):
        raw, parts = _load_group(group, read_partial, dev)
        owners = sorted((dests[0], o + bl.offset - r.offset, bl)
                        for r, o in parts for bl, dests in r.blobs)
        entries = [IndexBlob(b"", TREE, at, bl.length, bl.uncompressed_length or None)
                   for _, at, bl in owners]
        plain = read_blobs(key, raw, entries, device)
        host = plain.data.cpu().numpy()
        for (j, _, _), o, n in zip(owners, plain.offsets, plain.lengths):
            texts[j] = host[int(o):int(o) + int(n)].tobytes()
    return texts


def _lookup_level(index, tpe: int, ids: List[bytes], device) -> List[Optional[bytes]]:
    """The pack id of every id's entry in the index, None for a miss: one
    ``DeviceIndex.lookup`` for the level."""
    if not ids:
        return []
    if device is None:
        got = [index.get_id(tpe, i) for i in ids]
        return [None if g is None else g[0] for g in got]
    import torch
    from .dindex import COL_COUNT, COL_PACK, NO_PACK
    arr = np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32).copy()
    hits = index.lookup(tpe, torch.from_numpy(arr).to(torch.device("cuda", int(device))))
    h = hits.cpu().numpy().view(np.uint32)
    packs = index.packs(tpe)
    return [None if int(r[COL_COUNT]) == 0 or int(r[COL_PACK]) == NO_PACK
            else packs[int(r[COL_PACK])] for r in h]


_NULL_ID = bytes(32)
# RCDC_CKTREE_*: the kinds of rcdc_check_trees_level, in its numbering
LEVEL_KINDS = ("FileHasNoContent", "FileBlobHasNullId", "FileBlobNotInIndex", "NoSubTree",
               "NullSubTree", "SubTreeMissingInIndex")
# rcdc_cktree_finding as a numpy record
CKT_FINDING = np.dtype([("node", "<u4"), ("kind", "<u4"), ("blob_num", "<u4"), ("pad", "<u4")])
NODE_FACTS = ("host", "device")


def level_ids(level) -> Tuple[List[bytes], List[bytes]]:
    """The ids a level looks up: the content ids of file nodes, and the
    subtrees of dir nodes that are neither absent nor all zero.  ``level``:
    [(path, [tree.TreeNode])]."""
    data_ids = [i for _, nodes in level for n in nodes if n.type == "file"
                for i in n.content or []]
    tree_ids = [n.subtree for _, nodes in level for n in nodes
                if n.type == "dir" and n.subtree is not None and n.subtree != _NULL_ID]
    return data_ids, tree_ids


def judge_level(level, data_packs, tree_packs, findings: List[Result], packs: set) -> list:
    """check_trees' rule for the nodes of a level (check.rs:645-697), which
    rcdc_check_trees_level is held against.  ``data_packs`` / ``tree_packs``:
    per id of ``level_ids`` the pack id of its index entry, None for a miss.
    Appends to ``findings``, adds to ``packs`` and returns [(subtree, path)]
    of every node with a subtree, in order."""
    data_packs, tree_packs = iter(data_packs), iter(tree_packs)
    subtrees = []
    for path, nodes in level:
        for n in nodes:
            where = _join(path, n.name)
            if n.type == "file":
                if n.content is None:
                    findings.append((ERROR, Finding("FileHasNoContent", dict(file=where))))
                for i, id_ in enumerate(n.content or []):
                    if id_ == _NULL_ID:
                        findings.append((ERROR, Finding("FileBlobHasNullId",
                                                        dict(file=where, blob_num=i))))
                    pack = next(data_packs)
                    if pack is None:
                        findings.append((ERROR, Finding("FileBlobNotInIndex",
                                                        dict(file=where, blob_id=id_))))
                    else:
                        packs.add(pack)
            elif n.type == "dir":
                if n.subtree is None:
                    findings.append((ERROR, Finding("NoSubTree", dict(dir=where))))
                elif n.subtree == _NULL_ID:
                    findings.append((ERROR, Finding("NullSubTree", dict(dir=where))))
                else:
                    pack = next(tree_packs)
                    if pack is None:
                        findings.append((ERROR, Finding("SubTreeMissingInIndex",
                                                        dict(dir=where, blob_id=n.subtree))))
                    else:
                        packs.add(pack)
            if n.subtree is not None:
                subtrees.append((n.subtree, where))
    return subtrees


def check_trees(key, index, snap_trees: Sequence[bytes], read_partial: Callable,
                device: Optional[int] = 0, budget: int = DEFAULT_BUDGET,
                decode: Optional[Callable] = None, findings: Optional[List[Result]] = None,
                node_facts: Optional[str] = None, stats: Optional[dict] = None):
    """check_trees (check.rs:627-700) over TreeStreamerOnce.  Returns
    (findings, the set of pack ids the trees refer to).

    The walk goes level by level in ``tree.find_used_blobs``'s order: a level
    is the trees first reached from the level before, the first being the
    distinct snapshot trees, each with the path it was first reached by.  The
    reference's order and the path a tree reached twice is reported under
    depend on its threads' timing; this order is fixed.

    Per level: every tree id is looked up (``index``: a ``dindex.DeviceIndex``,
    or a ``HostIndex`` with ``device=None``); one the index lacks raises
    ErrorKind.Internal "Tree ID `...` not found in index" before anything of
    the level is read -- the findings of earlier levels are in ``findings``
    (pass a list to keep them; ``check_repository`` turns the error into
    ErrorCheckingTrees and an empty pack set).  Then the coalesced pack reads
    of ``find_used_blobs`` with one ``read.read_blobs`` per group.

    ``node_facts`` (with a device; ``device=None`` ignores it) says where the
    nodes are judged.  "host": every blob's text comes to the host, the node
    facts by ``tree.parse_tree_nodes_host`` and ``judge_level``, the level's
    content ids and dir subtrees looked up in one ``lookup`` each.  "device"
    (None means this): the texts stay in HBM, ``tree.parse_tree_nodes`` gives
    node records, the id arrays are looked up as they are,
    rcdc_check_trees_level judges the records and marks the packs, and only
    the count of findings crosses; names cross for the nodes that have a
    finding and for the path above them, and a blob outside the device's
    grammar goes alone through the host rule, at its place.  Both give the
    same findings in the same order and the same packs.  ``stats`` (a dict)
    receives ``text_bytes_to_host``, ``name_bytes_to_host`` and
    ``host_parsed_blobs``; on a clean repository inside the grammar the device
    route leaves all three 0.  Every subtree of any node is followed once."""
    from .tree import _distinct, parse_tree_nodes_host
    if node_facts is not None and node_facts not in NODE_FACTS:
        raise RusticError(ErrorKind.InvalidInput, f"node_facts is one of {NODE_FACTS} or None")
    findings = [] if findings is None else findings
    stats = {} if stats is None else stats
    for k in ("text_bytes_to_host", "name_bytes_to_host", "host_parsed_blobs"):
        stats[k] = 0
    if device is not None and node_facts != "host":
        return _check_trees_device(key, index, snap_trees, read_partial, int(device), budget,
                                   findings, stats)
    packs = set()
    frontier = [(t, "") for t in _distinct(snap_trees)]
    visited = {t for t, _ in frontier}
    while frontier:
        tids = [t for t, _ in frontier]
        if device is None:
            texts = _host_texts(key, index, tids, read_partial, decode)
        else:
            texts = _device_texts(key, index, tids, read_partial, int(device), budget)
            stats["text_bytes_to_host"] += sum(len(t) for t in texts)
        stats["host_parsed_blobs"] += len(texts)
        level = [(path, parse_tree_nodes_host(text)) for (_, path), text in zip(frontier, texts)]
        data_ids, tree_ids = level_ids(level)
        subtrees = judge_level(level, _lookup_level(index, DATA, data_ids, device),
                               _lookup_level(index, TREE, tree_ids, device), findings, packs)
        frontier = []
        for subtree, where in subtrees:
            if subtree not in visited:
                visited.add(subtree)
                frontier.append((subtree, where))
    return findings, packs


def run_check_level(res, data_hits, tree_hits, data_marks, tree_marks, device: int = 0,
                    cap: int = 1024, guard: int = 0):
    """rcdc_check_trees_level over the outputs of one ``tree.parse_tree_nodes``
    (``res``; anything with ``node_records``, ``data_ids``, ``tree_ids`` and
    ``tree_is_dir`` does) and the (n, 6) int32 hit records of its two lookups;
    the marks are uint8 device tensors, one byte per pack of the type.
    Returns (count, findings): CKT_FINDING records on the host, None where the
    count is 0 -- then nothing but the count has crossed.  ``cap``: the room
    for findings tried first; ``guard``: bytes of 0xA5 kept behind them (the
    flat tensor is then returned instead), both for tests."""
    import torch
    from .crypto import _ctx
    dev = torch.device("cuda", int(device))
    al = lambda t: t.clone() if t.numel() and t.data_ptr() % 16 else t
    nodes, data, tree = al(res.node_records), al(res.data_ids), al(res.tree_ids)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    count = ctypes.c_uint64(0)
    with torch.cuda.device(dev):
        while True:
            flat = torch.full((cap * 16 + guard,), 0xA5, dtype=torch.uint8, device=dev)
            _check(_lib.lib().rcdc_check_trees_level(
                _ctx(int(device)).handle, ptr(nodes), int(nodes.shape[0]), ptr(data),
                ptr(data_hits), int(data.shape[0]), ptr(tree), ptr(res.tree_is_dir),
                ptr(tree_hits), int(tree.shape[0]), ptr(data_marks), int(data_marks.numel()),
                ptr(tree_marks), int(tree_marks.numel()), ptr(flat) if cap else None, cap,
                ctypes.byref(count), int(torch.cuda.current_stream(dev).cuda_stream)))
            if int(count.value) <= cap:
                break
            cap = int(count.value)  # nothing was written: come again with room
    n = int(count.value)
    if guard:
        return n, flat
    return n, (flat[:n * 16].cpu().numpy().view(CKT_FINDING) if n else None)


class _LevelNames:
    """The raw names of a level's frontier entries, kept in HBM: per entry
    the entry of the level before it hangs under and where its name lies (a
    ``tree.tree_names`` arena of a group, or a path the host already knows).
    ``path`` builds an entry's path when a finding needs it."""

    def __init__(self, stats):
        self.levels = [None]  # per level: (parents, part, within, arenas); None: the roots
        self.known = {}       # (level, entry) -> path
        self.stats = stats

    def raw(self, arena, i: int) -> str:
        offsets, names = arena
        o = offsets[i:i + 2].cpu().numpy()
        raw = names[int(o[0]):int(o[1])].cpu().numpy().tobytes()
        self.stats["name_bytes_to_host"] += len(raw)
        return raw_name(raw)

    def path(self, level: int, j: int) -> str:
        if self.levels[level] is None:
            return ""
        if (level, j) not in self.known:
            parents, part, within, arenas = self.levels[level]
            self.known[level, j] = _join(self.path(level - 1, int(parents[j])),
                                         self.raw(arenas[int(part[j])], int(within[j])))
        return self.known[level, j]


def raw_name(raw: bytes) -> str:
    """A node's name from the raw bytes between its quotes: the rule
    ``tree.parse_tree_nodes_host`` applies to the whole blob."""
    return json.loads(b'"' + bytes(raw) + b'"')


def _check_trees_device(key, index, snap_trees, read_partial, device: int, budget: int,
                        findings: List[Result], stats: dict):
    """check_trees with the node facts judged in HBM (``check_trees``)."""
    import torch
    from .dindex import COL_COUNT, COL_PACK, NO_PACK
    from .tree import (NODE_SUBTREE, OK, TR_NODE, _blob_text, _distinct, _IdSet, _level_groups,
                       _Rows, parse_tree_nodes, parse_tree_nodes_host, tree_names)
    dev = torch.device("cuda", device)
    packs = set()
    roots = _distinct(snap_trees)
    if not roots:
        return findings, packs
    names = _LevelNames(stats)
    with torch.cuda.device(dev):
        marks = {t: torch.zeros(len(index.packs(t)), dtype=torch.uint8, device=dev)
                 for t in (DATA, TREE)}
        empty_hits = torch.empty((0, 6), dtype=torch.int32, device=dev)
        lookup = lambda t, ids: index.lookup(t, ids) if int(ids.shape[0]) else empty_hits
        frontier = torch.from_numpy(np.frombuffer(b"".join(roots), np.uint8)
                                    .reshape(-1, 32).copy()).to(dev)
        visited = _IdSet(device)
        try:
            visited.take(frontier)
            level = 0
            while int(frontier.shape[0]):
                k = int(frontier.shape[0])
                found = []                 # (frontier position, finding), sorted at the end
                subtrees = _Rows(k, dev, 32)
                # per row of subtrees.parts: its blob, its name's arena and place there
                owner, part, within, arenas = [], [], [], []
                for js, plain in _level_groups(key, index, frontier, read_partial, device, budget):
                    res = parse_tree_nodes(plain.data, plain.offsets, plain.lengths, device)
                    blobs = res.blobs
                    n, got = run_check_level(res, lookup(DATA, res.data_ids),
                                             lookup(TREE, res.tree_ids), marks[DATA], marks[TREE],
                                             device)
                    if n:
                        found += _device_findings(names, level, js, plain, res, got, device)
                    # the names of the nodes with a subtree, in d_tree_ids' order
                    flags = res.node_records[:, 29]
                    with_subtree = torch.nonzero(flags & NODE_SUBTREE).reshape(-1)
                    subtrees.add(js, blobs["tree_start"], blobs["tree_ids"], res.tree_ids)
                    owner.append(np.repeat(js, blobs["tree_ids"].astype(np.int64)))
                    part.append(np.full(res.n_tree_ids, len(arenas), np.int64))
                    within.append(np.arange(res.n_tree_ids, dtype=np.int64))
                    arenas.append(tree_names(plain.data, res.node_records, with_subtree, device))
                    # a blob outside the device's grammar: the host rule, at its place
                    for i in np.nonzero(blobs["status"] != OK)[0]:
                        text = _blob_text(plain, i)
                        stats["text_bytes_to_host"] += len(text)
                        stats["host_parsed_blobs"] += 1
                        j = int(js[i])
                        one = [(names.path(level, j), parse_tree_nodes_host(text))]
                        data_ids, tree_ids = level_ids(one)
                        mine: List[Result] = []
                        below = judge_level(one, _lookup_level(index, DATA, data_ids, device),
                                            _lookup_level(index, TREE, tree_ids, device), mine, packs)
                        found += [(j, f) for f in mine]
                        subtrees.add_host(j, b"".join(s for s, _ in below))
                        owner.append(np.full(len(below), j, np.int64))
                        part.append(np.full(len(below), len(arenas), np.int64))
                        within.append(np.arange(len(below), dtype=np.int64))
                        arenas.append([w for _, w in below])
                findings += [f for _, f in sorted(found, key=lambda x: x[0])]
                # the next frontier: the subtrees first reached, in the level's order
                order = subtrees.order()
                frontier, new = visited.take_flags(subtrees.gather())
                rows = order[np.nonzero(new.cpu().numpy())[0]]
                cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)
                nxt = (cat(owner)[rows], cat(part)[rows], cat(within)[rows], arenas)
                names.levels.append(nxt)
                level += 1
                # what the host rule reached is a path already
                for e in np.nonzero([isinstance(arenas[p], list) for p in nxt[1]])[0]:
                    names.known[level, int(e)] = arenas[int(nxt[1][e])][int(nxt[2][e])]
        finally:
            visited.close()
        for t in (DATA, TREE):
            ids = index.packs(t)
            packs |= {ids[int(i)] for i in torch.nonzero(marks[t]).reshape(-1).cpu().numpy()}
    return findings, packs


def _device_findings(names, level: int, js, plain, res, got, device: int) -> list:
    """The findings of rcdc_check_trees_level (``got``: CKT_FINDING) as
    check_trees reports them, each with the frontier position of its blob:
    the records, names and ids of the nodes that have one come to the host."""
    import torch
    from .tree import TR_NODE, tree_names
    dev = res.node_records.device
    which, inverse = np.unique(got["node"], return_inverse=True)
    d_which = torch.from_numpy(which.astype(np.int64)).to(dev)
    recs = res.node_records[d_which].cpu().numpy().reshape(-1).view(TR_NODE)
    offsets, raw = tree_names(plain.data, res.node_records, d_which, device)
    offsets, raw = offsets.cpu().numpy(), raw.cpu().numpy().tobytes()
    names.stats["name_bytes_to_host"] += len(raw)
    # the ids a finding quotes, one gather per array
    r_of = recs[inverse]
    is_data = got["kind"] == LEVEL_KINDS.index("FileBlobNotInIndex")
    is_tree = got["kind"] == LEVEL_KINDS.index("SubTreeMissingInIndex")

    def rows(t, at):
        if not len(at):
            return []
        got_rows = t[torch.from_numpy(at.astype(np.int64)).to(dev)].cpu().numpy()
        return [r.tobytes() for r in got_rows]
    data_rows = iter(rows(res.data_ids, (r_of["data_start"].astype(np.int64) +
                                         got["blob_num"].astype(np.int64))[is_data]))
    tree_rows = iter(rows(res.tree_ids, r_of["tree_index"][is_tree]))
    out = []
    for f, u in zip(got, inverse):
        r = recs[u]
        j = int(js[int(r["blob"])])
        where = _join(names.path(level, j),
                      raw_name(raw[int(offsets[u]):int(offsets[u + 1])]))
        kind = LEVEL_KINDS[int(f["kind"])]
        if kind == "FileHasNoContent":
            d = dict(file=where)
        elif kind == "FileBlobHasNullId":
            d = dict(file=where, blob_num=int(f["blob_num"]))
        elif kind == "FileBlobNotInIndex":
            d = dict(file=where, blob_id=next(data_rows))
        elif kind == "SubTreeMissingInIndex":
            d = dict(dir=where, blob_id=next(tree_rows))
        else:
            d = dict(dir=where)
        out.append((j, (ERROR, Finding(kind, d))))
    return out


# ---- check_pack for a batch (check.rs:304-316, 718-814) -------------------------------

def _checking(pid: bytes, source: Exception) -> Result:
    return ERROR, Finding("ErrorCheckingPack", dict(id=pid, source=source))


def _fallback(key, p: IndexPack, d_pack, device: int) -> List[Result]:
    from .read import check_pack
    try:
        return [(ERROR, f) for f in check_pack(key, p, d_pack, device)]
    except RusticError as e:
        return [_checking(bytes(p.id), e)]


def _pack_groups(packs: Sequence[IndexPack], budget: int) -> List[List[int]]:
    groups, cur, size = [], [], 0
    for k, p in enumerate(packs):
        n = int(p.pack_size())
        if cur and size + n > budget:
            groups.append(cur)
            cur, size = [], 0
        cur.append(k)
        size += n
    if cur:
        groups.append(cur)
    return groups


def check_pack_batch(key, index_packs: Sequence[IndexPack], read_full: Callable,
                     device: int = 0, budget: int = DEFAULT_BUDGET,
                     stage_times: Optional[dict] = None) -> List[Result]:
    """The ``read_data`` loop of check_repository (check.rs:304-316) with
    ``check_pack`` (:718-814) for many packs: the findings of every pack, in
    the packs' order.  ``read_full(pack_id)`` returns the pack's bytes (or a
    uint8 device tensor); what it raises is ErrorReadingPack for that pack.

    Packs are taken in groups of at most ``budget`` bytes (a larger pack is a
    group of its own).  Per group: one upload; one ``sha256_device`` over all
    packs; one gather of the trailing u32s; the header lengths from
    rcdc_check_packs' records; one ``Key.open_blobs`` over all headers; one
    ``headers.parse_headers``; one rcdc_check_packs with the header side,
    which also gives the sorted order; one ``open_blobs`` over all blobs in
    that order; one decode with ``read._decode``'s retry rule; one
    ``sha256_device``; the id compare as a tensor op.

    Per pack the semantics are ``read.check_pack``'s: the early returns at
    PackSizeMismatch, PackHashMismatch, PackHeaderLengthMismatch and
    PackHeaderMismatchIndex; what that function raises is ErrorCheckingPack
    {id, source} for that pack only, the findings of its blobs before the
    failing one in sorted order are kept, and no other pack is affected.  A
    pack with blobs of both types in its index entries or its header, a
    header the parser gives a status for, or kernel status HOST goes through
    ``read.check_pack`` on its bytes in the group's arena.

    ``stage_times``: a dict that gets the device time of each stage added
    (milliseconds by events; every stage then waits)."""
    out: List[List[Result]] = [[] for _ in index_packs]
    for group in _pack_groups(index_packs, int(budget)):
        _check_group(key, [index_packs[k] for k in group], read_full, int(device), stage_times,
                     [out[k] for k in group])
    return [r for per in out for r in per]


class _Stage:
    def __init__(self, times, name, torch, dev):
        self.times, self.name, self.torch, self.dev = times, name, torch, dev

    def __enter__(self):
        if self.times is not None:
            self.a = self.torch.cuda.Event(enable_timing=True)
            self.b = self.torch.cuda.Event(enable_timing=True)
            self.a.record(self.torch.cuda.current_stream(self.dev))

    def __exit__(self, *exc):
        if self.times is not None:
            self.b.record(self.torch.cuda.current_stream(self.dev))
            self.b.synchronize()
            self.times[self.name] = self.times.get(self.name, 0.0) + self.a.elapsed_time(self.b)
        return False


def _check_group(key, packs: List[IndexPack], read_full, device: int, times, out) -> None:
    import torch
    from .compress import DEC_OK, DECODE_MESSAGE, decompress_frames
    from .crypto import _ctx, make_refs as aead_refs
    from .device import sha256_device
    from .dindex import _layout, _pad16
    from .headers import OK as HDR_OK, parse_headers
    dev = torch.device("cuda", device)
    ctx = _ctx(device)
    stage = lambda name: _Stage(times, name, torch, dev)
    # 1. the reads and PackSizeMismatch
    live, datas = [], []
    for k, p in enumerate(packs):
        pid = bytes(p.id)
        try:
            data = read_full(pid)
        except Exception as e:  # whatever the backend raises
            out[k].append((ERROR, Finding("ErrorReadingPack", dict(id=pid, source=e))))
            continue
        n = int(data.numel()) if hasattr(data, "numel") else len(data)
        size = int(p.pack_size())
        if n != size:
            out[k].append((ERROR, Finding("PackSizeMismatch", dict(id=pid, size=n, expected=size))))
            continue
        live.append(k)
        datas.append(data)
    if not live:
        return
    with torch.cuda.device(dev):
        s = int(torch.cuda.current_stream(dev).cuda_stream)
        # one upload: every pack on a 16-byte boundary of one arena
        sizes = np.array([int(packs[k].pack_size()) for k in live], np.int64)
        base = _layout(sizes).astype(np.int64)
        total = int(base[-1]) + _pad16(int(sizes[-1])) + 64
        arena = torch.empty(total, dtype=torch.uint8, device=dev)
        host = None
        for b, d in zip(base, datas):
            if hasattr(d, "data_ptr"):
                arena[int(b):int(b) + int(d.numel())].copy_(d)
            elif len(d):
                if host is None:
                    host = np.zeros(total, np.uint8)
                host[int(b):int(b) + len(d)] = np.frombuffer(d, np.uint8)
        if host is not None:
            mask = [not hasattr(d, "data_ptr") for d in datas]
            if all(mask):
                arena.copy_(torch.from_numpy(host))
            else:
                h = torch.from_numpy(host).to(dev)
                for b, n, m in zip(base, sizes, mask):
                    if m:
                        arena[int(b):int(b) + int(n)].copy_(h[int(b):int(b) + int(n)])
        # 2. PackHashMismatch and the trailing u32s: one hash call, one gather, one copy back
        with stage("pack_hash"):
            refs = torch.from_numpy(np.stack([base, sizes], 1)).to(dev)
            dig = sha256_device(ctx, arena, refs)
            want = torch.from_numpy(np.frombuffer(b"".join(bytes(packs[k].id) for k in live),
                                                  np.uint8).reshape(-1, 32).copy()).to(dev)
            ends = np.maximum(base + sizes - 4, 0)
            at = torch.from_numpy(ends[:, None] + np.arange(4)[None, :]).to(dev)
            both = torch.cat([dig, arena[at]], 1).cpu().numpy()
        wrong = (dig != want).any(1).cpu().numpy()
        trailing = both[:, 32:].copy().view("<u4").ravel()
        keep = []
        for j, k in enumerate(live):
            if wrong[j]:
                out[k].append((ERROR, Finding("PackHashMismatch",
                                              dict(id=bytes(packs[k].id),
                                                   comp_id=both[j, :32].tobytes()))))
            else:
                keep.append(j)
        # 3. the index side: header lengths, mixed types and HOST from the kernel's records
        flat = _flatten([packs[live[j]] for j in keep])
        d_ids, d_locs, d_types = _upload(torch, dev, *flat[:3])
        with stage("compare"):
            first = run_check_packs(d_ids, d_locs[:, 1], d_locs[:, 2], d_locs[:, 3], d_types,
                                    flat[3], device=device, cap_findings=0)
        slow, rest = [], []
        for i, j in enumerate(keep):
            k, rec = live[j], first.packs[i]
            pid, n = bytes(packs[k].id), int(sizes[j])
            header_len = int(rec["header_len"])
            if int(rec["status"]) == HOST or int(rec["type_findings"]):
                slow.append(j)
            elif n < 4:
                out[k].append(_checking(pid, RusticError(
                    ErrorKind.Internal,
                    f"Error reading pack header length `{header_len}` for `{pid.hex()}`")))
            elif int(trailing[j]) != header_len:
                out[k].append((ERROR, Finding("PackHeaderLengthMismatch",
                                              dict(id=pid, length=int(trailing[j]),
                                                   computed=header_len))))
            elif header_len + 4 > n:
                out[k].append(_checking(pid, RusticError(
                    ErrorKind.Internal, f"Error reading pack header for id `{pid.hex()}`")))
            else:
                rest.append((i, j, header_len))
        # 4. every header opened in one call and parsed in one call
        opened = []
        if rest:
            h_lens = np.array([h for _, _, h in rest], np.int64)
            h_in = np.array([int(base[j]) + int(sizes[j]) - 4 - h for _, j, h in rest], np.int64)
            p_lens = h_lens - 32
            p_offs = _layout(p_lens).astype(np.int64)
            plain = torch.zeros(int(p_offs[-1]) + _pad16(int(p_lens[-1])) + 16, dtype=torch.uint8,
                                device=dev)
            with stage("header_open"):
                st = key.open_blobs(arena.data_ptr(), aead_refs(h_in, h_lens, p_offs),
                                    plain.data_ptr(), s, ctx)
            for (i, j, _), code, o, ln in zip(rest, st, p_offs, p_lens):
                if code:
                    k = live[j]
                    out[k].append(_checking(bytes(packs[k].id), RusticError(
                        ErrorKind.Cryptography, SHORT_MESSAGE if code == 2 else MAC_MESSAGE)))
                else:
                    opened.append((i, j, int(o), int(ln)))
        todo = []
        if opened:
            with stage("parse"):
                parsed = parse_headers(plain, [o for _, _, o, _ in opened],
                                       [ln for _, _, _, ln in opened], device=device)
            hdr = np.zeros(len(keep), CK_HDR)
            hdr["type"] = NO_HEADER
            for (i, j, _, _), h in zip(opened, parsed.headers):
                if int(h["status"]) != HDR_OK or (int(h["data"]) and int(h["tree"])):
                    slow.append(j)
                else:
                    hdr[i] = (int(h["type"]), int(h["count"]), int(h["first"]))
                    todo.append((i, j))
            # 5. the compare with the index, and the sorted order
            with stage("compare"):
                second = run_check_packs(d_ids, d_locs[:, 1], d_locs[:, 2], d_locs[:, 3], d_types,
                                         flat[3], hdr=(parsed, hdr), device=device,
                                         cap_findings=0, want_order=True)
            order = second.order.cpu().numpy()
        blobs = []   # (pack j, its IndexPack's blob) in sorted order, pack after pack
        for i, j in todo:
            k = live[j]
            if int(second.packs[i]["header_verdict"]) != EQUAL:
                out[k].append((ERROR, Finding("PackHeaderMismatchIndex",
                                              dict(id=bytes(packs[k].id)))))
                continue
            f0, c = flat[3][i]
            room = int(sizes[j]) - 4 - int(second.packs[i]["header_len"])
            mine = [packs[k].blobs[int(e) - f0] for e in order[f0:f0 + c]]
            if any(int(b.offset) + int(b.length) > room for b in mine):
                # not reachable with an equal header and the indexed size; never read past a pack
                out[k].append(_checking(bytes(packs[k].id), RusticError(
                    ErrorKind.Internal, "a blob lies outside its pack")))
                continue
            blobs += [(j, b) for b in mine]
        if blobs:
            _check_blobs(key, ctx, packs, live, base, arena, blobs, out, stage, s, dev)
    for j in slow:
        k = live[j]
        out[k] += _fallback(key, packs[k], arena[int(base[j]):int(base[j]) + int(sizes[j])], device)


def _check_blobs(key, ctx, packs, live, base, arena, blobs, out, stage, s, dev) -> None:
    """check.rs:789-811 for the blobs of every pack of a group at once."""
    import torch
    from .compress import DEC_OK, DECODE_MESSAGE, decompress_frames
    from .crypto import make_refs as aead_refs
    from .device import sha256_device
    from .dindex import _layout, _pad16
    n = len(blobs)
    owner = np.array([j for j, _ in blobs], np.int64)
    b_lens = np.array([int(b.length) for _, b in blobs], np.int64)
    b_in = np.array([int(base[j]) + int(b.offset) for j, b in blobs], np.int64)
    ulens = np.array([_ulen(b) for _, b in blobs], np.int64)
    p_lens = np.maximum(b_lens - 32, 0)
    p_offs = _layout(p_lens).astype(np.int64)
    buf = torch.empty(int(p_offs[-1]) + _pad16(int(p_lens[-1])) + 64, dtype=torch.uint8, device=dev)
    with stage("blob_open"):
        st = key.open_blobs(arena.data_ptr(), aead_refs(b_in, b_lens, p_offs), buf.data_ptr(), s,
                            ctx)
    # per blob: the error that ends its pack there, or None
    fail: List[Optional[RusticError]] = [None] * n
    for i in np.nonzero(st)[0]:
        fail[int(i)] = RusticError(ErrorKind.Cryptography,
                                   SHORT_MESSAGE if int(st[i]) == 2 else MAC_MESSAGE)
    # a pack ends at its first failing blob: the blobs behind it are not looked at
    def cut():
        dead, ended = np.zeros(n, bool), {}
        for i in range(n):
            j = int(owner[i])
            if j in ended:
                dead[i] = True
            elif fail[i] is not None:
                ended[j] = i
                dead[i] = True
        return dead
    dead = cut()
    # one decode, then read._decode's retry rule for the frames that did not fit
    offs, lens = p_offs.copy(), p_lens.copy()
    comp = [i for i in range(n) if ulens[i] and not dead[i]]
    parts = [buf]
    room = int(buf.numel())
    with stage("decode"):
        retry, cap = comp, 0
        first = True
        while retry:
            if first:
                caps = [int(ulens[i]) for i in retry]
            else:
                cap = max(2 * cap, 2 * max(int(ulens[i]) for i in retry) + (128 << 10))
                if cap > 1 << 32:
                    for i in retry:
                        fail[i] = RusticError(ErrorKind.Internal, DECODE_MESSAGE)
                    break
                caps = [cap] * len(retry)
            o_offs = _layout(np.array(caps, np.int64)).astype(np.int64)
            extra = torch.empty(int(o_offs[-1]) + _pad16(caps[-1]) + 64, dtype=torch.uint8,
                                device=dev)
            dst, ln = decompress_frames(ctx, buf.data_ptr(), [int(p_offs[i]) for i in retry],
                                        [int(p_lens[i]) for i in retry], extra.data_ptr(),
                                        [int(o) for o in o_offs], caps, s)
            again = []
            for q, i in enumerate(retry):
                if int(dst[q]) == DEC_OK:
                    offs[i], lens[i] = room + int(o_offs[q]), int(ln[q])
                elif int(dst[q]) == 2:
                    fail[i] = RusticError(ErrorKind.Internal, DECODE_MESSAGE)
                else:
                    again.append(i)
            parts.append(extra)
            room += int(extra.numel())
            retry, first = again, False
    dead = cut()
    alive = np.nonzero(~dead)[0]
    wrong = np.zeros(n, bool)
    comp_ids = {}
    if len(alive):
        with stage("blob_hash"):
            allb = torch.cat(parts) if len(parts) > 1 else buf
            refs = torch.from_numpy(np.stack([offs[alive], lens[alive]], 1)).to(dev)
            dig = sha256_device(ctx, allb, refs)
            want = torch.from_numpy(np.frombuffer(b"".join(bytes(blobs[i][1].id) for i in alive),
                                                  np.uint8).reshape(-1, 32).copy()).to(dev)
            bad = (dig != want).any(1)
            rows = torch.nonzero(bad).ravel()
            got = dig[rows].cpu().numpy()
        for r, g in zip(rows.cpu().numpy(), got):
            wrong[alive[int(r)]] = True
            comp_ids[int(alive[int(r)])] = g.tobytes()
    for i, (j, b) in enumerate(blobs):
        k = live[j]
        pid = bytes(packs[k].id)
        if fail[i] is not None:
            out[k].append(_checking(pid, fail[i]))
        if dead[i]:
            continue
        if ulens[i] and int(lens[i]) != int(ulens[i]):
            out[k].append((ERROR, Finding("PackBlobLengthMismatch",
                                          dict(id=pid, blob_id=bytes(b.id)))))
        if wrong[i]:
            out[k].append((ERROR, Finding("PackBlobHashMismatch",
                                          dict(id=pid, blob_id=bytes(b.id), comp_id=comp_ids[i]))))


def _check_pack_host(key, p: IndexPack, data: bytes, decode) -> List[Result]:
    """check_pack (check.rs:718-814) in plain Python."""
    from .pack import header_size, parse_header
    pid, size = bytes(p.id), int(p.pack_size())
    if len(data) != size:
        return [(ERROR, Finding("PackSizeMismatch", dict(id=pid, size=len(data), expected=size)))]
    comp_id = hashlib.sha256(data).digest()
    if comp_id != pid:
        return [(ERROR, Finding("PackHashMismatch", dict(id=pid, comp_id=comp_id)))]
    header_len = header_size(p.blobs) + 32
    if len(data) < 4:
        raise RusticError(ErrorKind.Internal,
                          f"Error reading pack header length `{header_len}` for `{pid.hex()}`")
    in_pack = int.from_bytes(data[-4:], "little")
    if in_pack != header_len:
        return [(ERROR, Finding("PackHeaderLengthMismatch",
                                dict(id=pid, length=in_pack, computed=header_len)))]
    if header_len + 4 > len(data):
        raise RusticError(ErrorKind.Internal, f"Error reading pack header for id `{pid.hex()}`")
    header = key.decrypt_data(data[len(data) - 4 - header_len:len(data) - 4])
    pack_blobs = [(bytes(b.id), b.type, b.offset, b.length, b.uncompressed_len or None)
                  for b in parse_header(header)]
    blobs = _sorted_blobs(p.blobs)
    if pack_blobs != [(bytes(b.id), b.type, b.offset, b.length, _ulen(b) or None) for b in blobs]:
        return [(ERROR, Finding("PackHeaderMismatchIndex", dict(id=pid)))]
    out: List[Result] = []
    at = 0
    for b in blobs:
        plain = key.decrypt_data(data[at:at + int(b.length)])
        at += int(b.length)
        if _ulen(b):
            if decode is None:
                from .compress import decode_all
                plain = decode_all(plain)
            else:
                plain = decode(plain)
            if len(plain) != _ulen(b):
                out.append((ERROR, Finding("PackBlobLengthMismatch",
                                           dict(id=pid, blob_id=bytes(b.id)))))
        comp = hashlib.sha256(plain).digest()
        if comp != bytes(b.id):
            out.append((ERROR, Finding("PackBlobHashMismatch",
                                       dict(id=pid, blob_id=bytes(b.id), comp_id=comp))))
    return out


# ---- check_repository (check.rs:225-321) --------------------------------------------------

class CheckResults(List[Result]):
    """CheckResults: the findings with their levels."""

    def is_ok(self) -> None:
        """Raises ErrorKind.Repository "check found errors!" when a finding's
        level is Error (check.rs:962-974)."""
        if any(level == ERROR for level, _ in self):
            raise RusticError(ErrorKind.Repository, "check found errors!")


def check_repository(key, list_with_size: Callable, read_full: Callable, read_partial: Callable,
                     snap_trees: Sequence[bytes], read_data: bool = False,
                     read_data_subset: ReadSubset = ReadSubset(), device: Optional[int] = 0,
                     budget: int = DEFAULT_BUDGET, decode: Optional[Callable] = None,
                     rng: Optional[random.Random] = None, node_facts: Optional[str] = None,
                     stats: Optional[dict] = None) -> CheckResults:
    """check_repository (check.rs:225-321) without the cache and hot-file
    passes.  ``list_with_size(file_type)`` lists [(id, size)] of "index" or
    "pack" files, ``read_full(file_type, id)`` returns a file's bytes,
    ``read_partial(pack_id, offset, length)`` a part of a pack;
    ``snap_trees`` are the trees of the snapshots to check.

    ``check_packs`` over every index file; the collected packs into a
    ``DeviceIndex`` (``HostIndex`` with ``device=None``); ``check_trees``,
    whose error becomes ErrorCheckingTrees with an empty pack set; then, with
    ``read_data``, the collected packs that are not missing and that the trees
    refer to -- tree packs first, each with its id and blobs only, as the
    reference's ``into_index().into_iter()`` gives them -- through
    ``read_data_subset.apply`` and ``check_pack_batch``.  ``node_facts`` and
    ``stats`` are ``check_trees``'s."""
    results = CheckResults()
    index_files = [IndexFile.from_json(_decrypt_file(key, read_full("index", bytes(i)), device,
                                                     decode))
                   for i, _ in list_with_size("index")]
    found, collected, missing = check_packs(index_files, list_with_size("pack"), None, device)
    results += found
    tree = [p for p in collected if _blob_type(p) == TREE]
    data = [p for p in collected if _blob_type(p) == DATA]
    if device is None:
        index = HostIndex(collected)
    else:
        from .dindex import DeviceIndex
        index = DeviceIndex(int(device))
        index.extend(collected)
    try:
        try:
            _, used = check_trees(key, index, snap_trees, read_partial, device, budget, decode,
                                  results, node_facts, stats)
        except RusticError as e:
            results.append((ERROR, Finding("ErrorCheckingTrees", dict(source=e))))
            used = set()
    finally:
        if device is not None:
            index.close()
    if read_data:
        packs = [p for p in _collected_packs(tree, data)
                 if bytes(p.id) not in missing and bytes(p.id) in used]
        packs = read_data_subset.apply(packs, rng)
        if device is None:
            for p in packs:
                pid = bytes(p.id)
                try:
                    got = read_full("pack", pid)
                except Exception as e:
                    results.append((ERROR, Finding("ErrorReadingPack", dict(id=pid, source=e))))
                    continue
                try:
                    results += _check_pack_host(key, p, bytes(got), decode)
                except RusticError as e:
                    results.append(_checking(pid, e))
        else:
            results += check_pack_batch(key, packs, lambda pid: read_full("pack", pid),
                                        int(device), budget)
    return results
